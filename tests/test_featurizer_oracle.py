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


def _dft_cases():
    """The tested geometries, each with 3 frames and half a hop; the reference's mel sizes centred at the shortest legal length
    and at 6 frames."""
    from tests.featurizer_cases import GEOMETRIES, REF_MEL
    cases = [(400, 160, 400, False, 1200), (64, 16, 48, False, 200), (64, 16, 48, True, 40), (64, 16, 48, True, 200)]
    cases += [(g.n_fft, g.hop, g.win, False, g.n_fft + 2 * g.hop + g.hop // 2) for g in GEOMETRIES.values()]
    cases += [(REF_MEL["n_fft"], REF_MEL["hop_length"], REF_MEL["win_length"], True, n) for n in (257, 800)]
    cases += [(65, 16, 49, True, 160), (65, 16, 49, True, 170)]
    return cases


@pytest.mark.parametrize("n_fft,hop,win,center,n", _dft_cases())
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


@pytest.mark.parametrize("n_fft", (64, 65, 400, 401, 512))
@pytest.mark.parametrize("hop", (1, 16, 17, 160))
def test_frame_counts_are_the_frames_torch_stft_returns(n_fft, hop):
    """The module's and the oracle's frame arithmetic against the frames torch.stft gives, centred and not.  Centred lengths start
    just above the reflect pad and include len % hop in {0, 1, hop - 1}: for an odd n_fft the padded signal has len + n_fft - 1
    samples, one frame fewer than len // hop + 1 whenever len % hop == 0."""
    import rnnt_amd.featurizer as F
    pad = n_fft // 2
    window = torch.hann_window(n_fft, dtype=torch.float64)

    def stft_frames(n, center):
        return torch.stft(torch.zeros(n, dtype=torch.float64), n_fft, hop, n_fft, window=window, center=center, pad_mode="reflect",
                          return_complex=True).shape[1]

    first = (pad // hop + 1) * hop  # the first multiple of the hop above the pad
    centred = {pad + 1, pad + 2, first, first + 1, first + hop - 1, first + hop, first + 5 * hop, first + 5 * hop + 1,
               first + 6 * hop - 1, n_fft - 1, n_fft, n_fft + 1, 3 * n_fft}
    assert {n % hop for n in centred} >= {0, 1 % hop, hop - 1}
    for n in sorted(centred):
        assert n > pad
        assert F.frame_count(n, n_fft, hop, True) == fo.frame_count(n, n_fft, hop, True) == stft_frames(n, True), (n, n_fft, hop)
    for n in (n_fft, n_fft + 1, n_fft + hop - 1, n_fft + hop, n_fft + 5 * hop, n_fft + 6 * hop - 1, 3 * n_fft):
        assert F.frame_count(n, n_fft, hop) == fo.frame_count(n, n_fft, hop) == stft_frames(n, False), (n, n_fft, hop)
    assert F.frame_count(n_fft - 1, n_fft, hop) == fo.frame_count(n_fft - 1, n_fft, hop) == 0


def test_odd_n_fft_centred_ragged_torch_path():
    """65 / 16 / 49 centred with 10 mels: 160 samples (len % hop == 0) give the 10 frames torch.stft returns, and the ragged call
    runs and equals the oracle."""
    import rnnt_amd
    mod = rnnt_amd.NormalizedMelSpectrogram(True, 1.0, 0.5, sample_rate=16000, n_fft=65, win_length=49, hop_length=16, f_min=20.0,
                                            f_max=7600.0, n_mels=10)
    kw = dict(n_fft=65, hop=16, win_length=49, kind=fo.GAIN, mean=1.0, invstd=0.5, center=True, fbank=fo.htk_fbank(33, 20.0, 7600.0, 10, 16000))
    waves = [_wave(160, seed=20), _wave(170, seed=21), _wave(33, seed=22), _wave(800, seed=23)]
    got, counts = mod(waves)
    want, want_counts = fo.ragged(waves, **kw)
    assert mod.last_backend == "torch" and counts.tolist() == want_counts == [10, 11, 3, 50]
    assert got.shape == want.shape and float((got - want).abs().max()) <= 1e-11 * max(1.0, float(want.abs().max()))
    for j, c in enumerate(want_counts):
        assert not got[j, :, c:].any()
    for w, c in zip(waves, want_counts):
        assert mod(w[None]).shape == (1, 10, c)
    # 401 / 160 / 401 with 800 samples, the reference's spectrogram sizes made odd
    mod = rnnt_amd.NormalizedMelSpectrogram(n_fft=401, hop_length=160, n_mels=20)
    got, counts = mod([_wave(800, seed=24), _wave(801, seed=25)])
    assert counts.tolist() == [5, 6] and got.shape == (2, 20, 6) and not got[0, :, 5:].any()


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
        # the reference's main configuration, as config/basic_sp.yaml states it
        (rnnt_amd.NormalizedMelSpectrogram(n_fft=512, win_length=400, hop_length=160, n_mels=80, f_min=0, f_max=8000, mean=15.0, invstddev=0.25),
         dict(n_fft=512, hop=160, win_length=400, kind=fo.GAIN, mean=15.0, invstd=0.25, center=True, fbank=fo.htk_fbank(257, 0, 8000, 80, 16000))),
    ]


@pytest.mark.parametrize("i", range(5))
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
    short = kw["n_fft"] // 2 + 38 if kw.get("center") else 30
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


def test_reference_mel_filterbank():
    """The filterbank of the reference's main configuration (257 bins, 0 - 8000 Hz, 80 mels): the published formula, no empty filter."""
    from tests.featurizer_cases import ref_mel_module
    mod = ref_mel_module()
    want = fo.htk_fbank(257, 0, 8000, 80, 16000)
    assert (mod.n_fft, mod.win_length, mod.hop_length, mod.center, mod.n_features) == (512, 400, 160, True, 80)
    assert mod.fbank.shape == (257, 80) and mod.fbank.dtype == torch.float64
    assert float((mod.fbank - want).abs().max()) < 1e-12
    assert int((mod.fbank.sum(0) == 0).sum()) == 0 and (mod.fbank >= 0).all() and float(mod.fbank.max()) <= 1.0


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
