"""-m gpu: RNNTModel.greedy_stream on the device (rnnt_engine_greedy_stream_decode) — the persistent launch resumed
from the stream's state block and the kernel-per-layer loop with its rings refilled from the last 7 tokens — against the reference's
token lists (tests/golden/decode_*.npz) and the numpy oracle (oracle/decode_oracle.py), for every way of chunking tried."""
import warnings

import numpy as np
import pytest
import torch

from oracle import decode_oracle
from oracle import predictor_oracle as po
from tests.helpers import DECODE_CASES, decode_case_arrays, load_decode_case
from tests.stream_models import StreamingCausalEncoder, engine_model, partitions, stream_frames

pytestmark = pytest.mark.gpu

GPU_CHUNKINGS = ("1", "3", "16", "17", "all", "random")


def _frames(frames):
    return torch.from_numpy(np.ascontiguousarray(frames.T)).cuda()  # (C, T)


def _stream(model, frames_ct, sizes, ml, persistent):
    s = model.greedy_stream(max_length=ml, persistent=persistent)
    got, pushes = stream_frames(s, frames_ct, sizes)
    want_path = "persistent" if persistent else "loop"
    assert all(path == want_path for _, path, k in pushes if k > 0), pushes
    return s, got, pushes


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_stream_paths_match_reference_token_lists(golden_dir, name):
    c = load_decode_case(golden_dir, name)
    model = engine_model(c["spec"], c["pred_sd"], c["joint_sd"])
    frames_ct = _frames(c["frames"])
    T = frames_ct.shape[1]
    parts = partitions(T, seed=len(name))
    for ml, want in c["tokens"].items():
        for persistent in (True, False):
            for pname in GPU_CHUNKINGS:
                s, got, _ = _stream(model, frames_ct, parts[pname], ml, persistent)
                assert got == want, (name, ml, persistent, pname)
                assert s.done == (len(want) + 1 >= ml)


@pytest.mark.parametrize("name,seeds", [("decode_small", range(4)), ("decode_small_proj", range(4)), ("decode_ref_widths_proj", range(1))])
def test_stream_matches_oracle_on_fresh_seeds(golden_dir, name, seeds):
    spec = DECODE_CASES[name]
    bias = float(np.load(f"{golden_dir}/{name}.npz")["blank_bias"])
    counted = 0
    for seed in seeds:
        frames, pred_sd, joint_sd = decode_case_arrays(spec, 4200 + seed, bias)
        T = frames.shape[0]
        model = engine_model(spec, pred_sd, joint_sd)
        frames_ct = _frames(frames)
        for ml in (spec["max_lengths"][0], None):
            want, margins = decode_oracle.greedy_decode(frames, pred_sd, joint_sd, max_length=T * 10 + 2 if ml is None else ml,
                                                        window=7 if spec["E"] > 64 else None)
            if margins.min() < 1e-3:
                continue
            counted += 1
            for persistent in (True, False):
                for pname in ("7", "random"):
                    _, got, _ = _stream(model, frames_ct, partitions(T, seed)[pname], ml, persistent)
                    assert got == want, (name, seed, ml, persistent, pname)
    assert counted >= len(seeds)


def _expect_paths(pushes, bad_rows, bad_frames):
    """Which path each push must have taken: a push that computes a text vector beyond +-30 (rows L0 .. L0 + c - 1 for c labels after
    L0) or holds a frame beyond it is redone on the loop; one that cannot meet either (row L0 + c included) stays persistent."""
    L0, t0, mid = 0, 0, False
    for new, path, k in pushes:
        c = len(new)
        rows_sure = range(L0, L0 + c)
        rows_maybe = range(L0, L0 + c + 1)
        frames_bad = any(t0 <= f < t0 + k for f in bad_frames)
        if k > 0 and (frames_bad or any(bad_rows[r] for r in rows_sure if r < len(bad_rows))):
            assert path == "loop", (L0, c, path)
            mid |= not bad_rows[L0] and not frames_bad
        elif k > 0 and not any(bad_rows[r] for r in rows_maybe if r < len(bad_rows)):
            assert path == "persistent", (L0, c, path)
        L0 += c
        t0 += k
    return mid


@pytest.mark.parametrize("where", ["frame", "text"])
def test_range_fallback_mid_stream_redoes_one_push_on_the_loop(golden_dir, where):
    """A persistent push that meets an audio frame (code 10) or a text vector (code 11, possibly after labels of the same push) beyond
    +-30 leaves the stream's state untouched; the same push is redone on the loop, silently, and the next push is persistent again."""
    c = load_decode_case(golden_dir, "decode_small")
    frames, pred_sd = c["frames"].copy(), dict(c["pred_sd"])
    bad_frames = []
    if where == "frame":  # frames 23 and 24 only: the third push of 10 (every text vector stays within +-30)
        frames[23, 5], frames[24, 6] = 40.0, -41.0
        bad_frames = [23, 24]
    else:  # one text feature scaled: some labels' text vectors pass 30, others do not
        w = pred_sd["output_layer_norm.weight"].copy()
        w[7] *= 20.0
        pred_sd["output_layer_norm.weight"] = w
    want, margins = decode_oracle.greedy_decode(frames, pred_sd, c["joint_sd"], max_length=60)
    assert margins.min() > 1e-3 and len(want) > 5
    text, _ = po.forward(np.asarray([[c["spec"]["V"] - 1] + want]), pred_sd)
    bad_rows = [bool(b) for b in (np.abs(text[0]) > 30).any(-1)]
    assert any(bad_rows) == (where == "text")
    model = engine_model(c["spec"], pred_sd, c["joint_sd"])
    frames_ct = _frames(frames)
    T = frames_ct.shape[1]
    mid, seen = False, set()
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # an exact path, not a degraded one: no warning
        for sizes in ([10] * 7 + [5], [3] * 25, [0, 4, 0, 21, 2, 48]):
            s = model.greedy_stream(max_length=60)
            got, pushes = stream_frames(s, frames_ct, sizes)
            assert got == want, (where, sizes)
            mid |= _expect_paths(pushes, bad_rows, bad_frames)
            paths = [p for _, p, k in pushes if k > 0]
            seen |= set(paths)
            if where == "frame" and sizes[0] == 10:
                assert paths[2] == "loop" and paths[3] == "persistent" and paths.count("loop") == 1, paths
    assert seen == {"persistent", "loop"} and T == 75
    if where == "text":
        assert mid, "no push met its first beyond-range text vector after labels of its own"


def test_unbounded_stream_beyond_the_lds_label_buffer(golden_dir):
    """More than 2048 labels in one stream (and in one push: the persistent kernel's global-memory label path), no cap."""
    spec = dict(DECODE_CASES["decode_cap"], T=210)
    bias = float(np.load(f"{golden_dir}/decode_cap.npz")["blank_bias"])
    frames, pred_sd, joint_sd = decode_case_arrays(spec, 4300, bias)
    T = frames.shape[0]
    want, margins = decode_oracle.greedy_decode(frames, pred_sd, joint_sd, max_length=T * 10 + 2, window=7)
    assert len(want) > 2048 and margins.min() > 1e-3
    model = engine_model(spec, pred_sd, joint_sd)
    frames_ct = _frames(frames)
    for persistent, sizes in ((True, [T]), (True, [50] * 4 + [10]), (True, [1] * T), (False, [64] * 3 + [18])):
        s, got, pushes = _stream(model, frames_ct, sizes, None, persistent)
        assert got == want and not s.done and s.frames == T, (persistent, sizes)


def test_max_length_reached_mid_push(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    model = engine_model(c["spec"], c["pred_sd"], c["joint_sd"])
    frames_ct = _frames(c["frames"])
    T = frames_ct.shape[1]
    for persistent in (True, False):
        s1, got, _ = _stream(model, frames_ct, [1] * T, 9, persistent)
        f = s1.frames  # the frame of the label that filled the cap
        assert got == c["tokens"][9] and s1.done and 2 <= f < T - 3, f
        s = model.greedy_stream(max_length=9, persistent=persistent)
        got = s.push_encoded(frames_ct[None, :, :f - 1])
        assert not s.done
        got += s.push_encoded(frames_ct[None, :, f - 1:f + 3])  # the cap is reached at the push's second frame
        assert got == c["tokens"][9] and s.done and s.frames == f, (persistent, s.frames)
        assert s.push_encoded(frames_ct[None, :, f + 3:]) == [] and s.tokens == c["tokens"][9] and s.frames == f


def test_two_streams_interleaved(golden_dir):
    c = load_decode_case(golden_dir, "decode_small_proj")
    model = engine_model(c["spec"], c["pred_sd"], c["joint_sd"])
    a = _frames(c["frames"])
    b = _frames(c["frames"][::-1].copy())
    lens = torch.tensor([a.shape[1]], device="cuda")
    wa = model.greedy_decode(a[None], lens, max_length=60)
    wb = model.greedy_decode(b[None], lens, max_length=60)
    assert wa == c["tokens"][60] and wa != wb
    for persistent in (True, False):
        sa, sb = model.greedy_stream(max_length=60, persistent=persistent), model.greedy_stream(max_length=60, persistent=persistent)
        ga, gb = [], []
        for t in range(0, a.shape[1], 6):
            ga += sa.push_encoded(a[None, :, t:t + 6])
            gb += sb.push_encoded(b[None, :, t:t + 6])
        assert ga == wa and gb == wb, persistent


def test_nan_workspace_and_repeat_runs_are_bit_identical(golden_dir):
    import rnnt_amd
    c = load_decode_case(golden_dir, "decode_ref_widths_proj")
    model = engine_model(c["spec"], c["pred_sd"], c["joint_sd"])
    frames_ct = _frames(c["frames"])
    dev = torch.device("cuda", torch.cuda.current_device())
    for persistent in (True, False):
        runs = []
        for _ in range(2):
            rnnt_amd.engine.workspace(dev, 1).fill_(255)  # every float in the stream's scratch buffer is a NaN
            torch.cuda.synchronize()
            runs.append(_stream(model, frames_ct, [13] * 9 + [3], 200, persistent)[1])
        assert runs[0] == runs[1] == c["tokens"][200], persistent


def test_push_mel_through_a_streaming_encoder_on_the_device(golden_dir):
    c = load_decode_case(golden_dir, "decode_small")
    model = engine_model(c["spec"], c["pred_sd"], c["joint_sd"], encoder=StreamingCausalEncoder())
    rng = np.random.default_rng(11)
    mel = torch.from_numpy(rng.standard_normal((1, c["spec"]["H"], 151)).astype(np.float32)).cuda()
    want = model.greedy_decode(mel, torch.tensor([151], device="cuda"), max_length=60)
    ref, margins = decode_oracle.greedy_decode(model.encoder(mel)[0].T.cpu().numpy(), c["pred_sd"], c["joint_sd"], max_length=60)
    assert margins.min() > 1e-3 and want == ref
    for step in (20, 7):
        s = model.greedy_stream(max_length=60)
        got = []
        for i in range(0, 151, step):
            got += s.push(mel[..., i:i + step])
        assert got == want and s.last_path == "persistent", step
