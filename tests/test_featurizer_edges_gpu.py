"""The featurizer's engine path (rnnt_amd/csrc/featurizer.hip) at the reference's mel configuration (config/basic_sp.yaml: 512 / 160 /
400, 80 mels, centred) and at the geometry edges of tests/featurizer_cases.py, against the float64 oracle (tests/featurizer_oracle.py).

The bar is the one of tests/test_featurizer_gpu.py: the engine's max |y - fp64| is at most 4 x the torch fp32 path's own max error
against the same oracle on the same input; the torch error is computed here and never taken from the engine.  One addition: at the tiny
geometries (a dozen samples a frame) the torch fp32 path lands within about one fp32 spacing of the oracle, luck that no fp32 pipeline
can be held to, so the torch error that enters the bar is taken as at least ONE fp32 spacing of the largest oracle value,
2^-23 max|want|.  Both errors and the bar are printed (profiles/featurizer_edges_parity.txt is this module's output).  Measured on an
MI355X: the engine's error is 0.52 - 2.2 x that reference error over the module's 41 comparisons.

Inputs are broadband as in tests/test_featurizer_gpu.py.  At the geometry edges the noise's deviation follows the window, so that the
mean power sits at PIECEWISE's cutoff of 0.01 for the first utterance (both branches) and nine times above it for the second.
"""
import pytest
import torch

from tests import featurizer_oracle as fo
from tests.featurizer_cases import (FBANK_BLOCK, FEAT_SLICE, FRAME_TILE, GEOMETRIES, OFFLINE, REF_MEL, STREAMED, STREAMS, KINDS,
                                    as64, bins, check, engine_run, geometry_module, noise, oracle_kw, per_bin, ref_mel_module, stream,
                                    tiles, to_int16, torch32)

pytestmark = pytest.mark.gpu

HOP, PAD = REF_MEL["hop_length"], REF_MEL["n_fft"] // 2
# samples -> frames at the reference mel sizes: the shortest legal utterance; exactly one filterbank block and two power tiles; a second
# filterbank block and a third power tile, each with one frame
MEL_LENGTHS = {PAD + 1: 2, HOP * 63 + HOP - 1: FBANK_BLOCK, HOP * 64: FBANK_BLOCK + 1}


def _pcm_name(pcm):
    return "int16" if pcm else "fp32"


# ---------------------------------------------------------------------------------------------------- the reference mel configuration
@pytest.mark.parametrize("n", list(MEL_LENGTHS))
def test_reference_mel_configuration(n):
    frames = MEL_LENGTHS[n]
    assert fo.frame_count(n, REF_MEL["n_fft"], HOP, True) == frames
    if frames == 2:  # the second (last) frame reads reflected samples at both ends: it starts inside the front pad and ends in the rear one
        assert n == PAD + 1 and HOP < PAD and HOP + REF_MEL["n_fft"] > PAD + n
    elif frames == FBANK_BLOCK:
        assert tiles(frames, FBANK_BLOCK) == 1 and tiles(frames, FRAME_TILE) == 2 and frames % FRAME_TILE == 0
    else:
        assert tiles(frames, FBANK_BLOCK) == 2 and frames % FBANK_BLOCK == 1 and tiles(frames, FRAME_TILE) == 3 and frames % FRAME_TILE == 1
    base = torch.stack([noise(n, 1100 + frames, tone=True), noise(n, 1200 + frames, sigma=0.03)])
    for pcm in (False, True):
        x = to_int16(base) if pcm else base
        mod = ref_mel_module()
        want = fo.features(as64(x), **oracle_kw(mod))
        assert want.shape == (2, REF_MEL["n_mels"], frames)
        got = engine_run(mod, x.cuda())
        assert got.dtype == torch.float32
        check(f"512/160/400 mel 257->80 centred, {n} samples, {_pcm_name(pcm)}", got, want, torch32(mod, x), floor=True)
        if frames == FBANK_BLOCK + 1:
            tm = engine_run(mod, x.cuda(), time_major=True)
            assert tm.stride(1) == 1 and torch.equal(tm, got)
    for kind in (0, 1):  # (the class ships GAIN; the kernels' other stages behind this filterbank are reached this way)
        mod = ref_mel_module()
        mod.log_kind = kind
        check(f"512/160/400 mel 257->80 centred, {n} samples, log kind {KINDS[kind]}", engine_run(mod, base.cuda()),
              fo.features(base.double(), **oracle_kw(mod)), torch32(mod, base), floor=True)


def test_reference_mel_ragged():
    """Counts, zeros behind each count, parity, and every utterance's frames bit for bit what it gives alone."""
    lens = [HOP * 64, HOP * 9 + 1, PAD + 1]
    mod = ref_mel_module()
    for pcm in (False, True):
        waves = [noise(n, 1300 + i, tone=i == 0) for i, n in enumerate(lens)]
        if pcm:
            waves = [to_int16(w) for w in waves]
        want, counts = fo.ragged([as64(w) for w in waves], **oracle_kw(mod))
        assert counts == [65, 10, 2]
        got, got_counts = engine_run(mod, [w.cuda() for w in waves])
        assert got_counts.tolist() == counts and got.shape == (3, 80, 65)
        for i, c in enumerate(counts):
            assert not got[i, :, c:].any(), i
        check(f"512/160/400 mel ragged {counts}, {_pcm_name(pcm)}", got, want, torch32(mod, waves), floor=True)
        for i, c in enumerate(counts):
            assert torch.equal(got[i, :, :c], engine_run(mod, waves[i].cuda())), i


def test_reference_mel_beyond_one_launch_slice():
    """66 utterances of 3 frames: the second launch slice indexes the power workspace at n_base + blockIdx.z, so utterances 64 and 65
    must give their own bits; then ragged, 3, 2 and 2 frames."""
    mod = ref_mel_module()
    N, T = FEAT_SLICE + 2, 2 * HOP + 5
    assert fo.frame_count(T, REF_MEL["n_fft"], HOP, True) == 3 and T > PAD
    x = torch.stack([noise(T, 1400 + i) for i in range(N)])
    xd = x.cuda()
    y = engine_run(mod, xd)
    assert y.shape == (N, 80, 3)
    check(f"512/160/400 mel, {N} utterances of 3 frames", y, fo.features(x.double(), **oracle_kw(mod)), torch32(mod, x), floor=True)
    for i in (0, FEAT_SLICE - 1, FEAT_SLICE, FEAT_SLICE + 1):
        assert torch.equal(y[i], engine_run(mod, xd[i])), i
    lens = [(T, T - 60, PAD + 1)[i % 3] for i in range(N)]
    yr, counts = engine_run(mod, [xd[i, :n] for i, n in enumerate(lens)])
    assert counts.tolist() == [(3, 2, 2)[i % 3] for i in range(N)]
    for i in (0, 1, 2, FEAT_SLICE - 1, FEAT_SLICE, FEAT_SLICE + 1):
        c = int(counts[i])
        assert torch.equal(yr[i, :, :c], engine_run(mod, xd[i, :lens[i]])) and not yr[i, :, c:].any(), i


# ---------------------------------------------------------------------------------------------------- the geometry table, offline
def _sigma(g):
    """The deviation at which white noise under a periodic Hann window of g.win samples (sum w^2 = 3 win / 8) has a mean power of 0.01."""
    return (0.01 / (0.375 * g.win)) ** 0.5


@pytest.mark.parametrize("name", OFFLINE)
def test_geometry_offline(name):
    """33 frames and half a hop: two frame tiles, the second with one frame; a batch of two views that start at sample 1 of a longer
    buffer; parity against the oracle; two calls give the same bits."""
    g = GEOMETRIES[name]
    n = g.n_fft + FRAME_TILE * g.hop + g.hop // 2
    assert fo.frame_count(n, g.n_fft, g.hop) == FRAME_TILE + 1
    s = _sigma(g)
    base = torch.stack([noise(n + 1, 1500, sigma=s, tone=True), noise(n + 1, 1501, sigma=3 * s)])
    for pcm in ((False, True) if name in ("odd_hop", "odd_nfft") else (False,)):
        src = to_int16(base) if pcm else base
        x, xd = src[:, 1:], src.cuda()[:, 1:]
        assert not xd.is_contiguous()
        mod = geometry_module(g)
        want = fo.features(as64(x), **oracle_kw(mod))
        assert want.shape == (2, bins(g.n_fft), FRAME_TILE + 1)
        got = engine_run(mod, xd)
        check(f"{g.n_fft}/{g.hop}/{g.win} {name}, 33 frames, {_pcm_name(pcm)}", got, want, torch32(mod, x), floor=True)
        assert torch.equal(got, engine_run(mod, xd))
        if name == "stage_limit":  # the largest stage check_desc accepts launches, and "auto" takes it
            assert torch.equal(mod(xd), got) and mod.last_backend == "engine"


def test_stage_over_is_refused():
    g = GEOMETRIES["stage_over"]
    mod = geometry_module(g)
    x = noise(g.n_fft + 3 * g.hop, 1600, sigma=_sigma(g))[None]
    mod.backend = "engine"
    try:
        with pytest.raises(RuntimeError, match="does not apply"):
            mod(x.cuda())
    finally:
        mod.backend = "auto"
    y = mod(x.cuda())
    assert mod.last_backend == "torch" and y.shape == (1, bins(g.n_fft), 4)
    assert float((y.double().cpu() - fo.features(x.double(), **oracle_kw(mod))).abs().max()) < 1e-4


# ---------------------------------------------------------------------------------------------------- the geometry table, streaming
@pytest.mark.parametrize("name", STREAMED)
def test_geometry_streamed_equals_whole_bit_for_bit(name):
    """STREAMS["edges"] scaled to the geometry: n_fft - 1, 1, hop, hop - 1, 1, 0 and a long rest.  The final state is the samples no
    frame has consumed."""
    g = GEOMETRIES[name]
    ref_sizes = STREAMS["edges"][1]
    sizes = [g.n_fft - 1, 1, g.hop, g.hop - 1, 1, 0, 12 * g.hop + g.hop // 2 + g.n_fft]
    assert ref_sizes[:6] == [400 - 1, 1, 160, 160 - 1, 1, 0] and len(sizes) == len(ref_sizes)
    s = _sigma(g)
    base = torch.stack([noise(sum(sizes), 1700, sigma=s, tone=True), noise(sum(sizes), 1701, sigma=3 * s)])
    for pcm in (False, True):
        x = (to_int16(base) if pcm else base).cuda()
        mod = geometry_module(g)
        whole = engine_run(mod, x)
        check(f"{g.n_fft}/{g.hop}/{g.win} {name}, whole utterance of the streaming case, {_pcm_name(pcm)}", whole,
              fo.features(as64(x.cpu()), **oracle_kw(mod)), torch32(mod, x.cpu()), floor=True)
        outs, state = stream(mod, x, sizes)
        for y in outs:
            assert tuple(y.shape[:2]) == (2, bins(g.n_fft))
        assert [y.shape[2] for y in outs[:2]] == [0, 1]
        assert torch.equal(torch.cat(outs, dim=2), whole)
        assert torch.equal(state, as64(x).float()[:, whole.shape[2] * g.hop:])
        assert state.shape[1] == sum(sizes) - whole.shape[2] * g.hop < g.n_fft


def test_no_carry_pushes_of_one_frame():
    """hop == n_fft and pushes of exactly n_fft samples: the state is empty going in and coming out (null state pointers on both
    sides), and every push gives its frame's bits."""
    g = GEOMETRIES["no_carry"]
    mod = geometry_module(g)
    x = torch.stack([noise(5 * g.n_fft, 1800, sigma=_sigma(g), tone=True), noise(5 * g.n_fft, 1801, sigma=3 * _sigma(g))]).cuda()
    whole = engine_run(mod, x)
    assert whole.shape == (2, bins(g.n_fft), 5)
    mod.backend = "engine"
    try:
        state = mod.streaming_init_state(2).cuda()
        for f in range(5):
            assert state.shape == (2, 0)
            y, state = mod.streaming_forward(x[:, f * g.n_fft:(f + 1) * g.n_fft], state)
            assert mod.last_backend == "engine" and torch.equal(y, whole[:, :, f:f + 1])
        assert state.shape == (2, 0)
    finally:
        mod.backend = "auto"


def test_gap_does_not_stream():
    """hop > n_fft: samples between frames would be skipped, not carried — refused on the engine as on the torch path."""
    g = GEOMETRIES["gap"]
    mod = geometry_module(g)
    for backend in ("engine", "torch"):
        mod.backend = backend
        try:
            with pytest.raises(ValueError, match="hop_length exceeds n_fft"):
                mod.streaming_init_state(1)
            with pytest.raises(ValueError, match="hop_length exceeds n_fft"):
                mod.streaming_forward(noise(200, 1900)[None].cuda(), torch.zeros(1, 0, device="cuda"))
        finally:
            mod.backend = "auto"


def test_streaming_through_the_filterbank():
    """The ABI allows n_filters > 0 with center = 0 and no shipped class uses it: 64 / 16 / 48 with the 33 -> 10 filterbank, whole against
    the oracle and streamed equal to whole bit for bit."""
    from rnnt_amd.featurizer import LOG_GAIN, _Featurizer, mel_filterbank
    mean, inv = per_bin(10)

    class MelStream(_Featurizer):
        def __init__(self):
            super().__init__()
            self._setup(64, 16, 48, False, LOG_GAIN, mean, inv, fbank=mel_filterbank(33, 20.0, 7600.0, 10, 16000))

    mod = MelStream()
    cfg, sizes, _ = STREAMS["small"]
    assert (cfg["n_fft"], cfg["hop"], cfg["win_length"]) == (64, 16, 48)
    kw = dict(n_fft=64, hop=16, win_length=48, kind=fo.GAIN, mean=mean, invstd=inv, center=False, fbank=fo.htk_fbank(33, 20.0, 7600.0, 10, 16000))
    base = torch.stack([noise(sum(sizes), 2000, tone=True), noise(sum(sizes), 2001, sigma=0.03)])
    for pcm in (False, True):
        x = (to_int16(base) if pcm else base).cuda()
        whole = engine_run(mod, x)
        want = fo.features(as64(x.cpu()), **kw)
        assert want.shape == (2, 10, fo.frame_count(sum(sizes), 64, 16))
        check(f"64/16/48 mel 33->10 not centred, whole utterance, {_pcm_name(pcm)}", whole, want, torch32(mod, x.cpu()), floor=True)
        outs, state = stream(mod, x, sizes)
        for y in outs:
            assert tuple(y.shape[:2]) == (2, 10)
        assert torch.equal(torch.cat(outs, dim=2), whole)
        assert torch.equal(state, as64(x).float()[:, whole.shape[2] * 16:])


# ---------------------------------------------------------------------------------------------------- odd n_fft, centred
def test_odd_n_fft_centred():
    """65 / 16 / 49 with 10 mels: the padded signal has len + 64 samples, so 160 samples (len % hop == 0) give 10 frames, not 11."""
    import rnnt_amd
    mod = rnnt_amd.NormalizedMelSpectrogram(True, 1.0, 0.5, sample_rate=16000, n_fft=65, win_length=49, hop_length=16, f_min=20.0,
                                            f_max=7600.0, n_mels=10)
    kw = oracle_kw(mod)
    for n, frames in ((160, 10), (170, 11)):
        x = torch.stack([noise(n, 2100 + n, tone=True), noise(n, 2101 + n, sigma=0.05)])
        t32 = torch32(mod, x)
        got = engine_run(mod, x.cuda())
        assert tuple(got.shape) == tuple(t32.shape) == (2, 10, frames)
        check(f"65/16/49 mel 33->10 centred, {n} samples", got, fo.features(x.double(), **kw), t32, floor=True)
    waves = [noise(160, 2260, tone=True), noise(170, 2271, sigma=0.05)]
    want, counts = fo.ragged([w.double() for w in waves], **kw)
    t32 = torch32(mod, waves)
    got, got_counts = engine_run(mod, [w.cuda() for w in waves])
    assert got_counts.tolist() == counts == [10, 11] and tuple(got.shape) == tuple(t32.shape) == (2, 10, 11)
    assert not got[0, :, 10:].any()
    check("65/16/49 mel ragged centred [10, 11]", got, want, t32, floor=True)
    for i, c in enumerate(counts):
        assert torch.equal(got[i, :, :c], engine_run(mod, waves[i].cuda())), i
