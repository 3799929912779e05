"""Inputs shared by the featurizer tests: seeded broadband waveforms, the parity check and the drivers of the GPU modules
(tests/test_featurizer_gpu.py, tests/test_featurizer_edges_gpu.py), the geometry edges of rnnt_amd/csrc/featurizer.hip with their
premises, and a waveform-to-tokens model — the reference's featurizer sizes (400 / 160 / 400, 201 bins, per-bin normalisation) in
front of a small AudioEncoder and the decode_small predictor / joint.  Every geometry states what it is there for as an assert, so
that a later change of a tile size fails the premise instead of silently leaving the path untested."""
import collections

import numpy as np
import torch

from tests import featurizer_oracle as fo

REF = dict(n_fft=400, hop=160, win_length=400)
SMALL = dict(n_fft=64, hop=16, win_length=48)


def noise(n, seed, sigma=0.01, tone=False, dtype=torch.float32):
    """Gaussian noise of deviation `sigma`, optionally plus a 440 Hz sine (at 16 kHz) of half that amplitude: broadband, so no bin sits
    on a leakage floor."""
    x = sigma * torch.randn(n, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
    if tone:
        x = x + 0.5 * sigma * torch.sin(2 * np.pi * 440.0 / 16000.0 * torch.arange(n, dtype=torch.float64))
    return x.to(dtype)


def to_int16(x):
    return (x.double() * 32768.0).round().clamp(-32768, 32767).to(torch.int16)


def per_bin(F=201):
    """A per-bin (mean, invstddev) pair, as basic_sp_convjs_globalfeat.yaml holds one."""
    return [-6.0 + 0.01 * k for k in range(F)], [0.5 + 0.002 * k for k in range(F)]


E2E_SEED, E2E_BLANK_BIAS, E2E_SAMPLES = 11, 7.0, 160 * 99 + 400  # chosen on the CPU (tests/test_featurizer_gpu.py asserts the margins they give)


def e2e_audio_case(norm_type="batch", seed=None, blank_bias=None):
    """(spec, encoder on the CPU in eval(), featurizer, int16 samples (E2E_SAMPLES,), pred_sd, joint_sd): 100 frames of 201 bins."""
    import rnnt_amd
    from tests.helpers import DECODE_CASES, decode_case_arrays
    seed = E2E_SEED if seed is None else seed
    blank_bias = E2E_BLANK_BIAS if blank_bias is None else blank_bias
    spec = DECODE_CASES["decode_small"]
    torch.manual_seed(8000 + seed)
    blocks = [rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, norm_type), rnnt_amd.JasperBlock(7, 20, 24, 0.1, 3, norm_type)]
    enc = rnnt_amd.AudioEncoder(input_features=201, prologue_kernel_size=5, prologue_stride=2, blocks=blocks, epilogue_features=28,
                                epilogue_kernel_size=7, epilogue_dilation=2, output_features=spec["H"], norm_type=norm_type).eval()
    g = torch.Generator().manual_seed(8100 + seed)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
        enc.blocks[-1].weight.mul_(6.0)  # frames of the scale the decode cases use
    # noise of deviation 0.01 under a 400-sample Hann window: power around 0.015, both sides of the piecewise cutoff
    mean = [-4.6 + 0.001 * k for k in range(201)]
    feat = rnnt_amd.TFJSSpectrogram(400, 160, 400, True, mean, [0.9] * 201)
    # (a slow envelope: the frames differ along the utterance, so the decode does not settle on one label)
    env = 0.6 + 0.5 * torch.sin(2 * np.pi * torch.arange(E2E_SAMPLES, dtype=torch.float64) / 2900.0) ** 3
    pcm = to_int16(noise(E2E_SAMPLES, 8300 + seed, tone=True, dtype=torch.float64) * env)
    _, pred_sd, joint_sd = decode_case_arrays(spec, 8200 + seed, blank_bias)
    return spec, enc, feat, pcm, pred_sd, joint_sd


# ---- the parity check and the drivers of the GPU modules ----------------------------------------------------------------------
FACTOR = 4.0
KINDS = {0: fo.PLAIN, 1: fo.PIECEWISE, 2: fo.GAIN}  # RNNT_FEAT_LOG_*


def check(label, got, want64, torch32, floor=False):
    """max |got - fp64| <= 4 x the torch fp32 path's own max error against the same oracle.  `floor`: the torch error is taken as at
    least one fp32 spacing of the largest oracle value (tests/test_featurizer_edges_gpu.py says why)."""
    want64 = torch.as_tensor(want64)
    assert tuple(got.shape) == tuple(want64.shape), (label, got.shape, want64.shape)
    err = float((got.double().cpu() - want64).abs().max())
    ref = float((torch32.double().cpu() - want64).abs().max())
    if floor:
        ref = max(ref, 2.0 ** -23 * float(want64.abs().max()))
    print(f"featurizer parity {label}: engine max|y - fp64| = {err:.3e}, torch fp32 error = {ref:.3e}, bar = {FACTOR * ref:.3e}")
    assert torch.isfinite(got).all() and err <= FACTOR * ref, label
    return err, ref


def oracle_kw(mod):
    """The oracle's arguments for a module."""
    mean = mod.mean if isinstance(mod.mean, float) else mod.mean.tolist()
    inv = mod.invstddev if isinstance(mod.invstddev, float) else mod.invstddev.tolist()
    kw = dict(n_fft=mod.n_fft, hop=mod.hop_length, win_length=mod.win_length, kind=KINDS[mod.log_kind], mean=mean, invstd=inv)
    if mod.center:
        kw["center"] = True
    if mod.fbank is not None:
        kw["fbank"] = fo.htk_fbank(mod.n_fft // 2 + 1, mod.f_min, mod.f_max, mod.n_mels, mod.sample_rate)
    return kw


def as64(x):
    return x.double() / 32768.0 if x.dtype == torch.int16 else x.double()


def torch32(mod, x):
    """The module's torch path in fp32 on the CPU (list: ragged)."""
    mod.backend = "torch"
    try:
        y = mod(x)
        assert mod.last_backend == "torch"
        return y[0] if isinstance(x, list) else y
    finally:
        mod.backend = "auto"


def engine_run(mod, x, **attrs):
    mod.backend = "engine"
    for k, v in attrs.items():
        setattr(mod, k, v)
    try:
        y = mod(x)
        assert mod.last_backend == "engine"
        return y
    finally:
        mod.backend = "auto"
        for k in attrs:
            setattr(mod, k, False)


def stream(mod, x, sizes, backend="engine", state=None):
    """Push x (N, time) chunk by chunk; ([feature blocks], final state).  Every input state is checked to be left as it was."""
    mod.backend = backend
    try:
        if state is None:
            state = mod.streaming_init_state(x.shape[0]).to(x.device)
        outs, t = [], 0
        for k in sizes:
            before = state.clone()
            y, new = mod.streaming_forward(x[:, t:t + k], state)
            assert mod.last_backend == backend
            assert torch.equal(state, before)  # never written in place
            assert new.shape[1] == 0 or new.data_ptr() != state.data_ptr()
            outs.append(y)
            state, t = new, t + k
        return outs, state
    finally:
        mod.backend = "auto"


STREAMS = {"edges": (REF, [399, 1, 160, 159, 1, 0, 2000], False), "1280": (REF, [1280] * 4, True),
           "small": (SMALL, [47, 1, 16, 15, 1, 0, 300, 17], False), "trickle": (REF, [100] * 30, True)}


# ---- geometry edges ----------------------------------------------------------------------------------------------------------
# the kernels' sizes restated (rnnt_amd/csrc/featurizer.hip): a change there fails a premise here, which is the point
BIN_TILE = 32          # k_feat_power: bins per workgroup (the MFMA's 32 rows)
FRAME_TILE = 32        # k_feat_power: frames per workgroup (the MFMA's 32 columns)
CHUNK = 4              # samples per basis chunk (one 16-byte load per lane)
WAVES = 4              # waves of a workgroup; wave w takes the chunks w, w + 4, ...
FBANK_BLOCK = 64       # k_feat_fbank: frames per workgroup
FEAT_SLICE = 64        # batch entries per launch
STAGE_WORDS = 16384    # FEAT_LDS_MAX / 4: floats of LDS a workgroup may stage


def tiles(n, tile):
    return -(-n // tile)


def bins(n_fft):
    return n_fft // 2 + 1


def chunks(n_fft):
    """Q of featurizer.hip: basis chunks of a bin tile."""
    return tiles(n_fft, CHUNK)


def stage_words(n_fft, hop):
    """Floats k_feat_power stages for one frame tile, restated from the kernel's addressing: sample c of the span lies at word
    c + (c // hop if the hop is even else 0); the host sizes the stage for c = span, one word beyond the last sample."""
    span = (FRAME_TILE - 1) * hop + n_fft
    last = span + (span // hop if hop % 2 == 0 else 0)
    return last + 1


Geometry = collections.namedtuple("Geometry", "name n_fft hop win")


def _geometry(name, n_fft, hop, win, premise):
    assert 1 <= win <= n_fft and (n_fft - win) % 2 == 0 and hop >= 1, name  # check_desc
    assert premise(n_fft, hop, win), name
    return Geometry(name, n_fft, hop, win)


GEOMETRIES = {g.name: g for g in [
    # an odd hop: no pad words (padw == 0), the staged span and the operand reads address plain c; n_fft ends half a chunk early
    # (the n0 < n_fft guard is true for one lane half and false for the other); a second bin tile with 2 live bins; the window
    # sits 8 samples inside n_fft
    _geometry("odd_hop", 66, 17, 50, lambda n, h, w: h % 2 == 1 and n % CHUNK == 2 and bins(n) == BIN_TILE + 2
              and tiles(bins(n), BIN_TILE) == 2 and (n - w) // 2 == 8),
    # an odd n_fft: the last chunk holds one sample, n1 < n_fft is false where n0 < n_fft is true
    _geometry("odd_nfft", 401, 160, 401, lambda n, h, w: n % CHUNK == 1 and bins(n) == 201),
    # fewer chunks than waves: waves 2 and 3 have none and still go through the LDS reduction with zero tiles
    _geometry("q_lt_4", 6, 3, 4, lambda n, h, w: chunks(n) == 2 < WAVES and bins(n) == 4),
    _geometry("hop1", 12, 1, 12, lambda n, h, w: h == 1 and chunks(n) == 3 < WAVES),
    # the smallest even hop: a pad word every 2 samples
    _geometry("hop2", 14, 2, 14, lambda n, h, w: h == 2 and stage_words(n, h) == (FRAME_TILE - 1) * h + n + ((FRAME_TILE - 1) * h + n) // 2 + 1),
    # exactly one full bin tile
    _geometry("bins32", 62, 16, 62, lambda n, h, w: bins(n) == BIN_TILE and tiles(bins(n), BIN_TILE) == 1),
    # samples between frames are skipped: offline only
    _geometry("gap", 32, 80, 32, lambda n, h, w: h > n),
    # a push can leave a state of length 0
    _geometry("no_carry", 32, 32, 32, lambda n, h, w: h == n),
    # the largest even hop at n_fft = 1024 whose stage fits, and the first geometry of the table that does not
    _geometry("stage_limit", 1024, 494, 1024, lambda n, h, w: stage_words(n, h) == 16372 <= STAGE_WORDS < stage_words(n, h + 2)),
    _geometry("stage_over", 512, 512, 512, lambda n, h, w: stage_words(n, h) == 16417 > STAGE_WORDS),
]}
OFFLINE = ("odd_hop", "odd_nfft", "q_lt_4", "hop1", "hop2", "bins32", "gap", "no_carry", "stage_limit")
STREAMED = ("odd_hop", "odd_nfft", "q_lt_4", "hop1", "no_carry")
assert all(stage_words(GEOMETRIES[k].n_fft, GEOMETRIES[k].hop) <= STAGE_WORDS for k in OFFLINE)

# the reference's main configuration (config/basic_sp.yaml, basic_sp_conv.yaml): NormalizedMelSpectrogram, centred, 80 mels
REF_MEL = dict(n_fft=512, win_length=400, hop_length=160, n_mels=80, f_min=0, f_max=8000, mean=15.0, invstddev=0.25)
assert bins(REF_MEL["n_fft"]) == 8 * BIN_TILE + 1                    # nine bin tiles, the ninth with one live bin
assert (REF_MEL["n_fft"] - REF_MEL["win_length"]) // 2 == 56         # zeros on each side of the window
assert REF_MEL["hop_length"] < REF_MEL["n_fft"] // 2 < 2 * REF_MEL["hop_length"]  # the first and last two frames read reflected samples


def ref_mel_module():
    import rnnt_amd
    return rnnt_amd.NormalizedMelSpectrogram(**REF_MEL)


def geometry_module(g, kind=1):
    """TFJSSpectrogram of a geometry: non-centred, PIECEWISE (kind 1) or PLAIN (0), per-bin normalisation."""
    import rnnt_amd
    mean, inv = per_bin(bins(g.n_fft))
    return rnnt_amd.TFJSSpectrogram(g.n_fft, g.hop, g.win, kind == 1, mean, inv)
