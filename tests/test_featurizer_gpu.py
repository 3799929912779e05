"""The featurizer's engine path (rnnt_amd/csrc/featurizer.hip) against the float64 oracle (tests/featurizer_oracle.py).  The bar of
every parity comparison is 4 x the torch fp32 path's own max error against that oracle on the same input (the encoder's rule,
tests/test_encoder_gpu.py; the margin covers a summation order that differs from an FFT's); both errors and the bar are printed
(profiles/featurizer_parity.txt is this module's output).  Inputs are broadband — Gaussian noise, optionally plus a sine —: a pure
tone's leakage-floor bins are ill-conditioned in fp32 for every implementation and are left out of a max-norm test.  Measured on an
MI355X: the engine's error is 0.64 - 2.1 x the torch fp32 path's over the module's 44 comparisons.
"""
import pytest
import torch

from tests import featurizer_oracle as fo
from tests.featurizer_cases import KINDS, STREAMS, e2e_audio_case, noise, per_bin, to_int16
from tests.featurizer_cases import as64 as _as64, check as _check, engine_run as _engine, oracle_kw as _kw, stream as _stream, torch32 as _torch32

pytestmark = pytest.mark.gpu

TILE = 32  # featurizer.hip: frames per workgroup tile (the MFMA's 32 columns)


def _ref_module(kind=1, scalar=False):
    import rnnt_amd
    mean, inv = (15.0, 0.25) if scalar else per_bin()
    if kind == 2:
        return rnnt_amd.TFJSOldPiecewiseSpectrogram(400, 160, 400, True, mean, inv)
    return rnnt_amd.TFJSSpectrogram(400, 160, 400, kind == 1, mean, inv)


@pytest.mark.parametrize("frames,rem", [(1, 0), (2, 1), (TILE - 1, 159), (TILE, 0), (TILE + 1, 1), (2 * TILE, 159)])
def test_shapes_at_reference_sizes(frames, rem):
    """Frame counts at the tile's edges, len - n_fft leaving 0, 1 and hop - 1, 201 bins (a partial bin tile), fp32 and int16, a batch of
    two views that start at an odd sample offset, (N, F, L) and time-major output, scalar and per-bin normalisation."""
    n = 400 + (frames - 1) * 160 + rem
    base = torch.stack([noise(n + 1, 100 + frames, tone=frames % 2 == 0), noise(n + 1, 200 + frames, sigma=0.03)])
    for pcm in (False, True):
        src = to_int16(base) if pcm else base
        x, xd = src[:, 1:], src.cuda()[:, 1:]
        assert xd.data_ptr() % (4 if pcm else 8) != 0 and not xd.is_contiguous()
        for scalar, time_major in ((False, False), (True, True)):
            mod = _ref_module(scalar=scalar)
            want = fo.features(_as64(x), **_kw(mod))
            assert want.shape == (2, 201, frames)
            got = _engine(mod, xd, time_major=time_major)
            assert got.dtype == torch.float32 and (got.stride(1) == 1) == (time_major or frames == 1)
            _check(f"400/160/400 {frames} frames, rem {rem}, {'int16' if pcm else 'fp32'}, {'scalar, time-major' if scalar else 'per-bin'}",
                   got, want, _torch32(mod, x))


def test_ragged_batch_and_zero_fill():
    """N = 3 ragged through the HOST length array, one utterance shorter than a frame: it gets 0 frames, and every frame behind an
    utterance's own count is stored as zero."""
    lens = [400 + TILE * 160 + 1, 400 + 9 * 160, 399]
    for pcm in (False, True):
        waves = [noise(n, 300 + i, tone=i == 0) for i, n in enumerate(lens)]
        if pcm:
            waves = [to_int16(w) for w in waves]
        mod = _ref_module()
        want, counts = fo.ragged([_as64(w) for w in waves], **_kw(mod))
        assert counts == [TILE + 1, 10, 0]
        got, got_counts = _engine(mod, [w.cuda() for w in waves])
        assert got_counts.tolist() == counts
        for i, c in enumerate(counts):
            assert not got[i, :, c:].any(), i
        _check(f"400/160/400 ragged {counts}, {'int16' if pcm else 'fp32'}", got, want, _torch32(mod, waves))
        # the same through the time-major store, and bit for bit what each utterance gives alone
        tm = _engine(mod, [w.cuda() for w in waves], time_major=True)[0]
        assert tm.stride(1) == 1 and torch.equal(tm, got)
        for i, c in enumerate(counts[:2]):
            assert torch.equal(got[i, :, :c], _engine(mod, waves[i].cuda()))


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_log_stages_and_both_piecewise_branches(kind):
    """Noise of deviation 0.01 puts about half of the cells on each side of PIECEWISE's 0.01 cutoff: at least 10 % of the oracle's cells lie
    on each side, so neither branch goes untested."""
    x = noise(400 + (2 * TILE - 1) * 160, 400)[None]
    p = fo.power(x, 400, 160, 400)
    frac = float((p > 0.01).double().mean())
    print(f"featurizer parity: {100 * frac:.1f} % of the cells above the piecewise cutoff")
    assert 0.1 <= frac <= 0.9
    mod = _ref_module(kind)
    _check(f"400/160/400 log kind {KINDS[kind]}", _engine(mod, x.cuda()), fo.features(x, **_kw(mod)), _torch32(mod, x))


@pytest.mark.parametrize("kind", (0, 1, 2))
def test_small_config_filterbank_centred(kind):
    """64 / 16 / 48: a window centred in n_fft with zeros, a 33 -> 10 filterbank, center = 1 (reflect) on utterances of 40 and 200 samples."""
    import rnnt_amd
    mod = rnnt_amd.NormalizedMelSpectrogram(True, 1.0, 0.5, sample_rate=16000, n_fft=64, win_length=48, hop_length=16, f_min=20.0,
                                            f_max=7600.0, n_mels=10)
    mod.log_kind = kind  # (the class ships GAIN; the kernels' other stages behind a filterbank are reached this way)
    kw = _kw(mod)
    for n in (40, 200):
        x = torch.stack([noise(n, 500 + n, tone=True), noise(n, 501 + n, sigma=0.05)])
        want = fo.features(x.double(), **kw)
        assert want.shape == (2, 10, n // 16 + 1)
        _check(f"64/16/48 mel 33->10 centred, {n} samples, log kind {KINDS[kind]}", _engine(mod, x.cuda()), want, _torch32(mod, x))
    waves = [noise(40, 540, tone=True), noise(200, 700, sigma=0.05)]
    want, counts = fo.ragged([w.double() for w in waves], **kw)
    got, got_counts = _engine(mod, [w.cuda() for w in waves])
    assert got_counts.tolist() == counts == [3, 13] and not got[0, :, 3:].any()
    _check(f"64/16/48 mel ragged centred, log kind {KINDS[kind]}", got, want, _torch32(mod, waves))
    with pytest.raises(ValueError, match="reflect"):
        _engine(mod, noise(32, 1).cuda())


@pytest.mark.parametrize("name", list(STREAMS))
def test_streamed_equals_whole_bit_for_bit(name):
    import rnnt_amd
    cfg, sizes, pcm = STREAMS[name]
    mean, inv = per_bin(cfg["n_fft"] // 2 + 1)
    mod = rnnt_amd.TFJSSpectrogram(cfg["n_fft"], cfg["hop"], cfg["win_length"], True, mean, inv)
    x = torch.stack([noise(sum(sizes), 600, tone=True), noise(sum(sizes), 601, sigma=0.03)])
    x = (to_int16(x) if pcm else x).cuda()
    whole = _engine(mod, x)
    _check(f"{cfg['n_fft']}/{cfg['hop']}/{cfg['win_length']} whole utterance of the streaming case {name}", whole,
           fo.features(_as64(x.cpu()), **_kw(mod)), _torch32(mod, x.cpu()))
    outs, state = _stream(mod, x, sizes)
    for y, k in zip(outs, sizes):
        assert tuple(y.shape[:2]) == (2, cfg["n_fft"] // 2 + 1)
    assert torch.equal(torch.cat(outs, dim=2), whole)
    assert torch.equal(state, _as64(x).float()[:, whole.shape[2] * cfg["hop"]:])


def test_state_crosses_between_the_paths():
    """A state the torch path left continues on the engine, and the other way round: held to the parity bar, not bitwise."""
    mod = _ref_module()
    x = noise(2720, 700, tone=True)[None]
    want, t32 = fo.features(x.double(), **_kw(mod)), _torch32(mod, x)
    xd = x.cuda()
    for first, second in (("torch", "engine"), ("engine", "torch")):
        a, state = _stream(mod, xd[:, :1000], [500, 500], backend=first)
        b, _ = _stream(mod, xd[:, 1000:], [700, 1020], backend=second, state=state)
        _check(f"400/160/400 streamed, {first} path then {second} path", torch.cat(a + b, dim=2), want, t32)


def test_nan_stays_in_its_frames_and_calls_repeat():
    """A NaN at one sample: exactly the frames that cover it are NaN, in every bin; every other frame has the clean run's bits.  Two calls
    on the same input give the same bits."""
    mod = _ref_module()
    x = noise(400 + (2 * TILE - 1) * 160, 800, tone=True)[None].cuda()
    clean = _engine(mod, x)
    assert torch.equal(clean, _engine(mod, x))
    s = TILE * 160 + 80  # inside the last frame of the first tile and the first of the second
    bad = x.clone()
    bad[0, s] = float("nan")
    got = _engine(mod, bad)
    covering = [f for f in range(2 * TILE) if f * 160 <= s < f * 160 + 400]
    assert covering == [TILE - 1, TILE]
    for f in range(2 * TILE):
        if f in covering:
            assert torch.isnan(got[0, :, f]).all(), f
        else:
            assert torch.equal(got[0, :, f], clean[0, :, f]), f


def test_batches_beyond_one_launch_slice():
    """The utterances' lengths travel in the kernel arguments, 64 to a launch: 70 utterances, ragged and not, give each utterance's own bits."""
    mod = _ref_module()
    T = 400 + 2 * 160 + 5
    x = torch.stack([noise(T, 900 + i) for i in range(70)]).cuda()
    y = _engine(mod, x)
    assert y.shape == (70, 201, 3)
    for i in (0, 63, 64, 69):
        assert torch.equal(y[i], _engine(mod, x[i]))
    lens = [T - (i % 3) * 160 for i in range(70)]  # 3, 2 and 1 frames
    yr, counts = _engine(mod, [x[i, :n] for i, n in enumerate(lens)])
    assert counts.tolist() == [3 - i % 3 for i in range(70)]
    for i in (0, 1, 2, 63, 64, 65, 69):
        c = int(counts[i])
        assert torch.equal(yr[i, :, :c], y[i, :, :c]) and not yr[i, :, c:].any()


def test_where_the_engine_does_not_apply():
    mod = _ref_module()
    x = noise(2000, 1000)[None].cuda()
    mod.backend = "engine"
    try:
        with pytest.raises(RuntimeError, match="does not apply"):
            mod(x.double())
        with pytest.raises(RuntimeError, match="does not apply"):
            mod(x.cpu())
    finally:
        mod.backend = "auto"
    assert mod(x.double()).dtype == torch.float64 and mod.last_backend == "torch"
    assert mod(x).dtype == torch.float32 and mod.last_backend == "engine"
    with pytest.raises(ValueError):
        mod(x[:, :399])


def _push_all(stream, pcm, sizes):
    t, held = 0, 0
    for k in sizes:
        stream.push_audio(pcm[t:t + k])
        t += k
        held += stream._pending is not None
    assert t >= len(pcm)
    return held


def test_samples_to_tokens_end_to_end():
    """push_audio over int16 chunks of 1280, over an uneven chunking and over 100-sample pushes (which the stride-2 prologue makes wait)
    gives greedy_decode of the whole utterance's features; BeamStream.push_audio gives beam_search's n-best list."""
    from oracle import decode_oracle
    from tests import beam_oracle
    from tests.stream_models import engine_model
    spec, enc, feat, pcm, pred_sd, joint_sd = e2e_audio_case()
    with torch.no_grad():
        frames = enc(feat(pcm[None]))[0].T.numpy()
    ref, margins = decode_oracle.greedy_decode(frames, pred_sd, joint_sd, max_length=60)
    assert margins.min() >= 1e-3 and 10 < len(ref) < 59  # the decode fixtures' MIN_MARGIN; the utterance ends by its frames
    want_beam, _, gap = beam_oracle.beam_search(beam_oracle.Model(frames, pred_sd, joint_sd), 4, 60)
    assert gap > 1e-3
    model = engine_model(spec, pred_sd, joint_sd, encoder=enc)
    model.featurizer = feat
    pcm = pcm.cuda()
    mel = feat(pcm[None])
    assert feat.last_backend == "engine" and mel.shape == (1, 201, 100)
    lens = torch.tensor([100], device="cuda")
    whole = model.greedy_decode(mel, lens, max_length=60)
    assert whole == ref
    n = len(pcm)
    for sizes in ([1280] * 13, [399, 1, 160, 159, 1, 0, 2000, 5000, 3, n - 7723], [100] * 163):
        s = model.greedy_stream(max_length=60)
        held = _push_all(s, pcm, sizes)
        assert s.tokens == whole, sizes[:3]
        assert feat.last_backend == "engine" and s.frames == 50 and s._pending is None
        if sizes[0] == 100:
            assert held > 0  # pushes that completed a frame the encoder could not take yet
    nbest = model.beam_search(mel, lens, beam_size=4, max_length=60, return_nbest=True)
    assert [y for y, _ in nbest] == [list(y) for y, _ in want_beam]
    b = model.beam_stream(beam_size=4, max_length=60)
    _push_all(b, pcm, [1280] * 13)
    assert [y for y, _ in b.nbest] == [y for y, _ in nbest] and b.tokens == nbest[0][0]
    for (_, gs), (_, ws) in zip(b.nbest, nbest):
        assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws))
    # without a featurizer there is nothing to push samples into
    model.featurizer = None
    with pytest.raises(TypeError, match="featurizer"):
        model.greedy_stream().push_audio(pcm[:1280])


def test_instance_norm_encoder_runs():
    """An instance-norm encoder depends on the chunking by definition: push_audio is only checked to run, holding single frames back."""
    from tests.stream_models import engine_model
    spec, enc, feat, pcm, pred_sd, joint_sd = e2e_audio_case("instance")
    model = engine_model(spec, pred_sd, joint_sd, encoder=enc)
    model.featurizer = feat
    s = model.greedy_stream(max_length=60)
    _push_all(s, pcm.cuda(), [1280] * 13)
    assert (s.done or s.frames > 40) and all(isinstance(t, int) for t in s.tokens)  # (done: the 60-label cap came first)
    s = model.greedy_stream(max_length=60)
    _push_all(s, pcm.cuda(), [160] * 102)  # one frame a push: the prologue gives one output frame every other push, which the norms refuse
    assert s.frames > 0
