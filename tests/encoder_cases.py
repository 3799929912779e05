"""Shared by tests/test_encoder_*.py: the small encoder of tests/golden/make_golden_encoder.py built from rnnt_amd's classes, the
reference-width encoder (basic_sp_convjs.yaml without look-ahead), and the fixtures (loaded once per process)."""
import functools
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NORM_TYPES = ("batch", "instance", "instance_affine")


def small_encoder(norm_type):
    import rnnt_amd
    blocks = [rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, norm_type), rnnt_amd.JasperBlock(7, 20, 24, 0.1, 3, norm_type)]
    return rnnt_amd.AudioEncoder(input_features=9, prologue_kernel_size=5, prologue_stride=2, prologue_dilation=1, blocks=blocks,
                                 epilogue_features=28, epilogue_kernel_size=7, epilogue_stride=1, epilogue_dilation=2,
                                 output_features=36, norm_type=norm_type)


def reference_width_encoder(norm_type="instance_affine", seed=0):
    """The widths of the reference's basic_sp_convjs.yaml (F = 201; 256 / 384 / 512 channels, k = 11 / 13 / 25, 4 sub-blocks each;
    epilogue 512, k = 29, dilation 2; output 1024), seeded init, norm parameters and running statistics drawn."""
    import rnnt_amd
    torch.manual_seed(seed)
    blocks = [rnnt_amd.JasperBlock(11, 256, 256, 0.2, 4, norm_type), rnnt_amd.JasperBlock(13, 256, 384, 0.2, 4, norm_type),
              rnnt_amd.JasperBlock(25, 384, 512, 0.3, 4, norm_type)]
    enc = rnnt_amd.AudioEncoder(input_features=201, prologue_kernel_size=11, prologue_stride=2, blocks=blocks, epilogue_features=512,
                                epilogue_kernel_size=29, epilogue_dilation=2, output_features=1024, norm_type=norm_type)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.InstanceNorm1d)):
                if m.weight is not None:
                    m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                if getattr(m, "running_mean", None) is not None:
                    m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                    m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
    return enc.eval()


@functools.lru_cache(maxsize=None)
def fixture(norm_type):
    with np.load(os.path.join(GOLDEN, f"encoder_{norm_type}.npz")) as z:
        return {k: z[k] for k in z.files}


def state_dict_of(fx):
    return {k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd/")}


def loaded_small_encoder(norm_type):
    enc = small_encoder(norm_type)
    res = enc.load_state_dict(state_dict_of(fixture(norm_type)), strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    return enc.eval()


def out64(fx, name=None):
    """The reference's float64 output: whole (N = 3) or streamed with chunking `name` (utterance 0)."""
    if name is None:
        return fx["out32"].astype(np.float64) + fx["out64_corr"].astype(np.float64)
    return fx["stream32_" + name].astype(np.float64) + fx["stream64_corr_" + name].astype(np.float64)


def running(fx):
    """Names of the chunkings on which the reference runs for this fixture's norm type."""
    return [n for n in fx["chunkings"].tolist() if n not in fx["raising"].tolist()]


@torch.no_grad()
def stream_all(enc, mel, chunks, state=None):
    """Push `mel` (N, F, L) chunk by chunk from `state` (None: streaming_init_state on mel's device); (output, final state,
    prologue state length after each chunk)."""
    if state is None:
        state = [s.to(device=mel.device, dtype=mel.dtype) for s in enc.streaming_init_state(mel.shape[0])]
    outs, lens0, t = [], [], 0
    for k in chunks:
        y, state = enc.streaming_forward(mel[:, :, t:t + k], state)
        outs.append(y)
        lens0.append(state[0].shape[2])
        t += k
    return torch.cat(outs, dim=2), state, lens0


E2E_SEED, E2E_BLANK_BIAS = 1, 6.0  # chosen on the CPU (tests/test_encoder_gpu.py asserts the margin they give)


def e2e_case(seed=None, blank_bias=None):
    """A small batch-norm encoder (F = 9 -> 64 features, the decode_small model's width) with a seeded mel (1, 9, 101) and that model's
    seeded predictor / joint state dicts: (spec, encoder on the CPU, mel, pred_sd, joint_sd)."""
    import rnnt_amd
    from tests.helpers import DECODE_CASES, decode_case_arrays
    seed = E2E_SEED if seed is None else seed
    blank_bias = E2E_BLANK_BIAS if blank_bias is None else blank_bias
    spec = DECODE_CASES["decode_small"]
    torch.manual_seed(7000 + seed)
    blocks = [rnnt_amd.JasperBlock(5, 12, 20, 0.1, 2, "batch"), rnnt_amd.JasperBlock(7, 20, 24, 0.1, 3, "batch")]
    enc = rnnt_amd.AudioEncoder(input_features=9, prologue_kernel_size=5, prologue_stride=2, blocks=blocks, epilogue_features=28,
                                epilogue_kernel_size=7, epilogue_dilation=2, output_features=spec["H"], norm_type="batch").eval()
    g = torch.Generator().manual_seed(7100 + seed)
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)
        enc.blocks[-1].weight.mul_(6.0)  # frames of the scale the decode cases use
    mel = torch.randn(1, 9, 101, generator=g)
    _, pred_sd, joint_sd = decode_case_arrays(spec, 7200 + seed, blank_bias)
    return spec, enc, mel, pred_sd, joint_sd
