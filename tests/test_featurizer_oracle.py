"""CPU tests of the featurizer's definition: the float64 oracle (tests/featurizer_oracle.py) against an independent O(n^2) DFT, the
GAIN log stage against the reference's three-branch in-place statement, the frame and state arithmetic, chunked == whole, the
modules' torch paths against the oracle, and push_audio's host path."""
import numpy as np
import pytest
import torch

from tests import featurizer_oracle as fo

CHUNKINGS = {"edges": [399, 1, 160, 159, 1, 0, 2000], "1280": [1280] * 4, "one": [1] * 401 + [2999], "100": [100] * 50}


def _wave(n, seed=0, sigma=0.01, tone=True):
    g = torch.Generator().manual_seed(seed)
    x = sigma * torch.randn(n, generator=g, dtype=torch.float64)
    if tone:
        x = x + 0.5 * sigma * torch.sin(2 * np.pi * 440.0 / 16000.0 * torch.arange(n, dtype=torch.float64))
    return x


@pytest.mark.parametrize("n_fft,hop,win,center,n", [(400, 160, 400, False, 1200), (64, 16, 48, False, 200), (64, 16, 48, True, 40),
                                                   (64, 16, 48, True, 200)])
def test_oracle_power_is_the_dft(n_fft, hop, win, center, n):
    x = _wave(n, seed=1, sigma=1.0)
    got = fo.power(x, n_fft, hop, win, center).numpy()
    want = fo.power_dft(x.numpy(), n_fft, hop, win, center)
    assert got.shape == want.shape == (n_fft // 2 + 1, fo.frame_count(n, n_fft, hop, center))
    assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()


def test_gain_stage_is_the_three_branch_statement():
    """(p + 1e-6) * 32767^2 >= 1073 > e^e: the reference's in-place statement takes its log branch only, and its second assignment
    (values <= e) finds none.  Float64 over p in [0, 1e12]: the difference is exactly 0."""
    p = torch.cat([torch.zeros(1, dtype=torch.float64), torch.logspace(-30, 12, 4001, dtype=torch.float64),
                   torch.rand(1000, dtype=torch.float64, generator=torch.Generator().manual_seed(0)) * 1e-5])
    assert float(((p + 1e-6) * fo.INT16_GAIN).min()) > np.e ** np.e
    assert torch.equal(fo.log_stage(p, fo.GAIN), fo.gain_three_branch(p))


def test_frame_and_state_arithmetic():
    import rnnt_amd.featurizer as F
    want = {0: (0, 0), 399: (0, 399), 400: (1, 240), 559: (1, 399), 560: (2, 240), 5000: (29, 360)}
    for n, (frames, left) in want.items():
        assert fo.frame_count(n, 400, 160) == F.frame_count(n, 400, 160) == frames
        assert fo.stream_step(0, n, 400, 160) == F.stream_lengths(0, n, 400, 160) == (frames, left)
        assert fo.frame_count(n, 400, 160, True) == F.frame_count(n, 400, 160, True) == n // 160 + 1
        if frames:  # the last frame ends inside the utterance, the next one would not
            assert (frames - 1) * 160 + 400 <= n < frames * 160 + 400
    # carried from push to push, the counts add up to the whole utterance's
    for sizes in CHUNKINGS.values():
        s, total = 0, 0
        for k in sizes:
            f, s = F.stream_lengths(s, k, 400, 160)
            total += f
            assert 0 <= s < 400
        assert total == fo.frame_count(sum(sizes), 400, 160)


@pytest.mark.parametrize("name", list(CHUNKINGS))
def test_oracle_chunked_equals_whole(name):
    sizes = CHUNKINGS[name]
    x = _wave(sum(sizes), seed=2)
    mean, inv = [0.1 * k for k in range(201)], 0.25
    whole = fo.features(x, 400, 160, 400, fo.PIECEWISE, mean, inv)
    outs, carry = fo.streamed(x, sizes, 400, 160, 400, fo.PIECEWISE, mean, inv)
    assert torch.equal(torch.cat(outs, dim=1), whole)
    assert torch.equal(carry, x[whole.shape[1] * 160:])


def _modules():
    import rnnt_amd
    mean, inv = [0.05 * k - 3 for k in range(201)], [0.2 + 0.001 * k for k in range(201)]
    return [
        (rnnt_amd.TFJSSpectrogram(400, 160, 400, True, mean, inv), dict(n_fft=400, hop=160, win_length=400, kind=fo.PIECEWISE, mean=mean, invstd=inv)),
        (rnnt_amd.TFJSSpectrogram(400, 160, 400, False), dict(n_fft=400, hop=160, win_length=400, kind=fo.PLAIN, mean=15.0, invstd=0.25)),
        (rnnt_amd.TFJSOldPiecewiseSpectrogram(64, 16, 48, True, 2.0, 0.5), dict(n_fft=64, hop=16, win_length=48, kind=fo.GAIN, mean=2.0, invstd=0.5)),
        (rnnt_amd.NormalizedMelSpectrogram(True, 1.0, 0.5, sample_rate=16000, n_fft=64, win_length=48, hop_length=16, f_min=20.0, f_max=7600.0,
                                           n_mels=10),
         dict(n_fft=64, hop=16, win_length=48, kind=fo.GAIN, mean=1.0, invstd=0.5, center=True, fbank=fo.htk_fbank(33, 20.0, 7600.0, 10, 16000))),
    ]


@pytest.mark.parametrize("i", range(4))
def test_module_torch_path_in_float64_is_the_oracle(i):
    mod, kw = _modules()[i]
    x = _wave(1500, seed=3 + i)
    assert mod.backend == "auto"
    got = mod(x)
    assert mod.last_backend == "torch" and got.dtype == torch.float64
    want = fo.features(x, **kw)
    assert got.shape == want.shape
    assert float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))
    # batched, and ragged with an utterance shorter than a frame (0 frames; centred: no such utterance)
    short = 70 if kw.get("center") else 30
    waves = [x, x[:901], x[:short]]
    got_r, counts = mod(waves)
    want_r, want_counts = fo.ragged(waves, **kw)
    assert counts.tolist() == want_counts and got_r.shape == want_r.shape
    assert float((got_r - want_r).abs().max()) <= 1e-11 * max(1.0, float(want_r.abs().max()))
    for j, c in enumerate(want_counts):
        assert not got_r[j, :, c:].any()
    mod.time_major = True
    tm = mod(torch.stack([x, x.flip(0)]))
    mod.time_major = False
    assert tm.stride(1) == 1 and torch.equal(tm, mod(torch.stack([x, x.flip(0)])))


def test_mel_filterbank_is_the_published_formula():
    import rnnt_amd.featurizer as F
    got = F.mel_filterbank(201, 0.0, 8000.0, 80, 16000)
    want = fo.htk_fbank(201, 0.0, 8000.0, 80, 16000)
    assert got.shape == (201, 80) and float((got - want).abs().max()) < 1e-12
    assert (got >= 0).all() and float(got.max()) <= 1.0 and (got.sum(0) > 0).all()


def test_module_streaming_torch_path():
    import rnnt_amd
    mod = rnnt_amd.TFJSSpectrogram(400, 160, 400)
    x = _wave(2720, seed=9)[None]
    whole = mod(x)
    for sizes in (CHUNKINGS["edges"], [1280, 1280, 160]):
        state, outs, t = mod.streaming_init_state(1).double(), [], 0
        assert tuple(state.shape) == (1, 0)
        for k in sizes:
            y, new = mod.streaming_forward(x[:, t:t + k], state)
            assert tuple(y.shape[:2]) == (1, 201) and new.shape[1] == rnnt_amd.featurizer.stream_lengths(state.shape[1], k, 400, 160)[1]
            outs.append(y)
            state, t = new, t + k
        assert torch.equal(torch.cat(outs, dim=2), whole)
    with pytest.raises(ValueError):
        rnnt_amd.NormalizedMelSpectrogram(n_fft=64, hop_length=16, n_mels=10).streaming_init_state(1)
    # int16 samples are scaled by 1 / 32768 on the way in
    pcm = (x * 32768 * 20).round().clamp(-32768, 32767).to(torch.int16)
    assert torch.equal(mod(pcm), mod(pcm.float() / 32768.0)) and mod(pcm).dtype == torch.float32


def _audio_model(encoder=None):
    import rnnt_amd
    from tests.helpers import DECODE_CASES, decode_case_arrays
    from tests.stream_models import StreamingCausalEncoder, cpu_model
    spec = DECODE_CASES["decode_small"]
    _, pred_sd, joint_sd = decode_case_arrays(spec, 7301, 16.0)
    model = cpu_model(spec, pred_sd, joint_sd, encoder=encoder or StreamingCausalEncoder())
    # 126 / 40: 64 bins, the model's frame width; normalised to frames of the decode cases' scale
    model.featurizer = rnnt_amd.TFJSSpectrogram(126, 40, 126, True, -2.6, 0.8)
    return model


@pytest.mark.parametrize("pcm16", (False, True))
def test_push_audio_host_path_equals_offline(pcm16):
    model = _audio_model()
    x = _wave(40 * 150 + 126, seed=11, sigma=0.05).float()
    if pcm16:
        x = (x * 32768).round().to(torch.int16)
    mel = model.featurizer(x[None])
    want = model.greedy_decode(mel, torch.tensor([mel.shape[2]]), max_length=200)
    assert 5 < len(want) < 199
    want_beam = model.beam_search(mel, torch.tensor([mel.shape[2]]), beam_size=3, max_length=200, return_nbest=True)
    for sizes in ([1280] * 5, [125, 1, 40, 39, 1, 0, 3000, 2920], [100] * 62):
        assert sum(sizes) >= len(x)
        s, b, got, t = model.greedy_stream(max_length=200), model.beam_stream(beam_size=3, max_length=200), [], 0
        for k in sizes:
            got += s.push_audio(x[t:t + k])
            b.push_audio(x[None, t:t + k])
            t += k
        assert got == want == s.tokens and s.last_path == "host"
        assert [y for y, _ in b.nbest] == [y for y, _ in want_beam]
        assert max(abs(a - c) for (_, a), (_, c) in zip(b.nbest, want_beam)) < 1e-9
        assert s._pending is None and s._audio_state.shape[1] == len(x) - mel.shape[2] * 40


def test_push_audio_needs_a_featurizer_and_keeps_frames_when_the_encoder_raises():
    from tests.stream_models import StreamingCausalEncoder
    model = _audio_model()
    feat, model.featurizer = model.featurizer, None
    assert model.featurizer is None
    for s in (model.greedy_stream(), model.beam_stream()):
        with pytest.raises(TypeError, match="featurizer"):
            s.push_audio(torch.zeros(200))
    model.featurizer = feat

    class Flaky(StreamingCausalEncoder):
        fail = True

        def streaming_forward(self, x, state):
            if self.fail:
                raise RuntimeError("not now")
            return super().streaming_forward(x, state)

    flaky = _audio_model(Flaky())
    x = _wave(3000, seed=12, sigma=0.05).float()
    s = flaky.greedy_stream(max_length=200)
    with pytest.raises(RuntimeError, match="not now"):
        s.push_audio(x[:1500])
    kept = s._pending.clone()
    assert kept.shape[2] == (1500 - 126) // 40 + 1
    flaky.encoder.fail = False
    got = s.push_audio(x[1500:])
    mel = flaky.featurizer(x[None])
    assert torch.equal(kept, mel[..., :kept.shape[2]])
    assert got == flaky.greedy_decode(mel, torch.tensor([mel.shape[2]]), max_length=200)


def test_push_audio_holds_frames_back_for_an_audio_encoder():
    """An rnnt_amd.AudioEncoder refuses a push that gives its prologue no output frame; push_audio asks its length arithmetic first
    and waits (host ints only), so 1-frame trickles decode to the whole utterance's tokens."""
    import rnnt_amd
    from tests.encoder_cases import e2e_case
    from tests.stream_models import cpu_model
    spec, enc, _, pred_sd, joint_sd = e2e_case()
    model = cpu_model(spec, pred_sd, joint_sd, encoder=enc)
    model.featurizer = rnnt_amd.TFJSSpectrogram(16, 8, 16, True, -6.0, 1.0)  # 9 bins: the small encoder's input width
    x = _wave(8 * 100 + 16, seed=13, sigma=0.05).float()
    mel = model.featurizer(x[None])
    want = model.greedy_decode(mel, torch.tensor([mel.shape[2]]), max_length=60)
    s, got, held = model.greedy_stream(max_length=60), [], 0
    for t in range(0, len(x), 8):
        got += s.push_audio(x[t:t + 8])
        held += s._pending is not None
    assert held > 0 and s.frames > 0  # the stride-2 prologue left single frames waiting
    assert got == want
