"""Generate tests/golden/encoder_{batch,instance,instance_affine}.npz from the REFERENCE's own `rnnt.jasper.AudioEncoder`
(reference rnnt/jasper.py, rnnt/causalconv.py) in eval mode.

Run in the build container only (the reference never travels to the GPU box):
    PYTHONPATH=/root/reference python tests/golden/make_golden_encoder.py

Small config: F = 9; prologue k = 5, stride 2 -> 12 channels; blocks (k = 5, 12 -> 20, 2 sub-blocks) and (k = 7, 20 -> 24,
3 sub-blocks); epilogue 28 channels, k = 7, dilation 2; output 36.  Norm weights / biases and running statistics are drawn
(not 1 / 0).  Per fixture:
  sd/<key>            the fp32 state dict
  mel                 seeded (3, 9, 101) fp32
  lens, out_lens      calc_output_lens of a few lengths
  out32, out64_corr   the fp32 module's output (3, 36, 50) and float32(float64 output - out32): the output of the .double() copy
                      is out32 + out64_corr to ~1e-13 (12 bytes per element did not fit the 256 KB a fixture may have)
  err_whole           max|fp32 - fp64|: the reference's own fp32 error
  chunkings           names; chunks_<name> the chunk lengths
  raising             names of the chunkings on which the reference raises for this norm type, raise_at_<name> the chunk index
  per chunking that runs, streamed through streaming_forward from streaming_init_state:
    stream32_<name>, stream64_corr_<name>, err_<name>   as above, utterance 0 only (N = 1: the file size again)
    state_shapes_<name>                                  the final state's shapes, [n_states, 3]
    state0_lens_<name>                                   the prologue state's length after every chunk (it is not constant)
  stream_vs_whole_<name>                                 max|streamed fp64 - whole fp64| of utterance 0 (0 for batch norm, not
                                                         for instance norm: the statistics are the chunk's)
Fixtures are data; no reference source is copied.
"""
import os

import numpy as np
import torch

from rnnt.jasper import AudioEncoder, JasperBlock  # reference, via PYTHONPATH=/root/reference

HERE = os.path.dirname(os.path.abspath(__file__))

CHUNKINGS = {
    "whole": [101],
    "halves": [50, 51],
    "sevens": [7] * 14 + [3],
    "twos": [2] * 50,  # batch norm only: instance norm refuses one output frame
    "ragged": [3, 4, 5, 9, 2, 6, 72],
}


def build(norm_type):
    blocks = [JasperBlock(5, 12, 20, 0.1, 2, norm_type), JasperBlock(7, 20, 24, 0.1, 3, norm_type)]
    return AudioEncoder(input_features=9, prologue_kernel_size=5, prologue_stride=2, prologue_dilation=1, blocks=blocks,
                        epilogue_features=28, epilogue_kernel_size=7, epilogue_stride=1, epilogue_dilation=2, output_features=36,
                        norm_type=norm_type)


def randomise_norms(enc, g):
    with torch.no_grad():
        for m in enc.modules():
            if isinstance(m, (torch.nn.BatchNorm1d, torch.nn.InstanceNorm1d)):
                if m.weight is not None:
                    m.weight.copy_(torch.rand(m.weight.shape, generator=g) + 0.5)
                    m.bias.copy_(torch.randn(m.bias.shape, generator=g) * 0.3)
                if getattr(m, "running_mean", None) is not None:
                    m.running_mean.copy_(torch.randn(m.running_mean.shape, generator=g) * 0.2)
                    m.running_var.copy_(torch.rand(m.running_var.shape, generator=g) + 0.5)


@torch.no_grad()
def stream(enc, mel, chunks):
    """(output, final state, prologue state length after each chunk) or the index of the chunk that raises."""
    state = [s.to(mel.dtype) for s in enc.streaming_init_state(mel.shape[0])]
    outs, lens0, t = [], [], 0
    for i, k in enumerate(chunks):
        try:
            y, state = enc.streaming_forward(mel[:, :, t:t + k], state)
        except (ValueError, RuntimeError):
            return i
        outs.append(y)
        lens0.append(state[0].shape[2])
        t += k
    return torch.cat(outs, dim=2), state, lens0


def main():
    for idx, norm_type in enumerate(("batch", "instance", "instance_affine")):
        torch.manual_seed(100 + idx)
        g = torch.Generator().manual_seed(200 + idx)
        enc = build(norm_type).eval()
        randomise_norms(enc, g)
        enc64 = build(norm_type).double().eval()
        enc64.load_state_dict({k: v.double() for k, v in enc.state_dict().items()}, strict=True)
        mel = torch.randn(3, 9, 101, generator=g)
        with torch.no_grad():
            out32, out64 = enc(mel), enc64(mel.double())
        lens = torch.tensor([101, 77, 2, 1, 50], dtype=torch.int64)
        fx = {"mel": mel.numpy(), "out32": out32.numpy(), "out64_corr": (out64 - out32.double()).float().numpy(),
              "err_whole": np.float64((out64 - out32.double()).abs().max().item()),
              "lens": lens.numpy(), "out_lens": enc.calc_output_lens(lens).numpy(),
              "chunkings": np.array(list(CHUNKINGS)), "norm_type": np.array(norm_type)}
        for k, v in enc.state_dict().items():
            fx["sd/" + k] = v.numpy()
        raising = []
        for name, chunks in CHUNKINGS.items():
            fx["chunks_" + name] = np.array(chunks, dtype=np.int64)
            r32, r64 = stream(enc, mel[:1], chunks), stream(enc64, mel[:1].double(), chunks)
            if isinstance(r32, int):
                assert r64 == r32
                raising.append(name)
                fx["raise_at_" + name] = np.int64(r32)
                continue
            (y32, st, lens0), (y64, _, _) = r32, r64
            fx["stream32_" + name] = y32.numpy()
            fx["stream64_corr_" + name] = (y64 - y32.double()).float().numpy()
            fx["err_" + name] = np.float64((y64 - y32.double()).abs().max().item())
            fx["state_shapes_" + name] = np.array([list(s.shape) for s in st], dtype=np.int64)
            fx["state0_lens_" + name] = np.array(lens0, dtype=np.int64)
            fx["stream_vs_whole_" + name] = np.float64((y64 - out64[:1]).abs().max().item())
        fx["raising"] = np.array(raising, dtype="U16")
        path = os.path.join(HERE, f"encoder_{norm_type}.npz")
        np.savez(path, **fx)
        print(norm_type, "err_whole %.3g" % fx["err_whole"], "|out| %.3g" % out32.abs().max().item(), "raising", raising,
              {n: "%.3g" % fx["err_" + n] for n in CHUNKINGS if n not in raising},
              {n: "%.3g" % fx["stream_vs_whole_" + n] for n in CHUNKINGS if n not in raising}, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
