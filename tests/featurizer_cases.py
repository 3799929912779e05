"""Inputs shared by the featurizer tests: seeded broadband waveforms, and a waveform-to-tokens model — the reference's featurizer sizes
(400 / 160 / 400, 201 bins, per-bin normalisation) in front of a small AudioEncoder and the decode_small predictor / joint."""
import numpy as np
import torch

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
