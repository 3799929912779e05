"""Generate tests/golden/encoder_train_<case>_n<N>.npz: parameter gradients of the REFERENCE's own `rnnt.jasper.AudioEncoder`
(reference rnnt/jasper.py, rnnt/causalconv.py) in eval() with grad on.

Run where the reference is (it never travels to the GPU box):
    PYTHONPATH=<reference checkout> python tests/golden/make_golden_encoder_train.py

Cases: batch, instance, instance_affine (the small config, state dict and mel (3, 9, 101) of encoder_<norm>.npz, which are read, not
stored again) and instance_affine_la2: instance_affine with additional_context = 2 on the EPILOGUE conv (the reference's CausalConv1d
put in the built module's place; parameter shapes do not depend on look-ahead, so it loads encoder_instance_affine.npz's state
dict).  Look-ahead on a JasperBlock cannot be recorded: the reference's whole-utterance forward raises there (its sub-blocks each
lose `additional_context` frames, the residual branch keeps the input's length, and `x + residual_x` fails on the sizes);
main() asserts that it still does.  Each case at N = 3 and at N = 1 (utterance 0), one file each
(a fixture may have 256 KB).  Per file:
  G                    seeded cotangent (N, 36, L_out) fp32; the scalar differentiated is sum(out * G)
  g32/<key>            the fp32 module's gradient of every parameter
  g64_corr/<key>       float32(float64 gradient - g32): the .double() copy's gradient is g32 + g64_corr to ~1e-13 relative
  err/<key>            max|g32 - g64|: the reference's own fp32 error for that tensor
  dyabs/<bias key>     for each conv that feeds an instance norm: sum over (n, t) of |d loss / d conv output| per channel, float64 (a
                       hook on the conv's output in the float64 copy); the bias gradient of such a conv is exactly zero, and this is
                       what bounds the rounding noise both sides return there
and, for the look-ahead case, encoder_train_<case>_out.npz: out32, out64_corr, err_out, the forward output (N = 3) as in
encoder_<norm>.npz (the other cases' outputs are those files').
Fixtures are data; no reference source is copied.
"""
import os

import numpy as np
import torch

from rnnt.causalconv import CausalConv1d  # reference, via PYTHONPATH
from rnnt.jasper import AudioEncoder, JasperBlock

HERE = os.path.dirname(os.path.abspath(__file__))
CASES = {"batch": ("batch", 0), "instance": ("instance", 0), "instance_affine": ("instance_affine", 0),
         "instance_affine_la2": ("instance_affine", 2)}


def build(norm_type, la, block_la=0):
    blocks = [JasperBlock(5, 12, 20, 0.1, 2, norm_type, additional_context=block_la), JasperBlock(7, 20, 24, 0.1, 3, norm_type)]
    enc = AudioEncoder(input_features=9, prologue_kernel_size=5, prologue_stride=2, prologue_dilation=1, blocks=blocks,
                       epilogue_features=28, epilogue_kernel_size=7, epilogue_stride=1, epilogue_dilation=2, output_features=36,
                       norm_type=norm_type)
    if la:
        at = len(enc.blocks) - 4  # the epilogue conv: ..., conv, norm, GELU, output 1x1
        assert isinstance(enc.blocks[at], CausalConv1d)
        enc.blocks[at] = CausalConv1d(24, 28, 7, 1, 2, additional_context=la)
    return enc


def grads(enc, mel, G, hooks=False):
    enc.zero_grad()
    dyabs, handles = {}, []
    if hooks:
        def feeds_instance_norm(name):
            return name.endswith(".conv") or "residual_conv" in name  # every conv but the output 1x1 (`blocks.<last>`)
        for name, m in enc.named_modules():
            if isinstance(m, torch.nn.Conv1d) and feeds_instance_norm(name):
                def hook(mod, gin, gout, name=name):
                    dyabs[name + ".bias"] = gout[0].abs().sum(dim=(0, 2)).double().numpy()
                handles.append(m.register_full_backward_hook(hook))
    out = enc(mel)
    (out * G).sum().backward()
    for h in handles:
        h.remove()
    return out.detach(), {k: p.grad.detach().clone() for k, p in enc.named_parameters()}, dyabs


def main():
    try:  # look-ahead on a block: the reference cannot run a whole utterance
        build("instance_affine", 0, block_la=2).eval()(torch.zeros(1, 9, 101))
        raise SystemExit("the reference now runs look-ahead on a block: record that case")
    except RuntimeError as e:
        print("look-ahead on a block, reference forward:", e)
    for ci, (case, (norm_type, la)) in enumerate(CASES.items()):
        with np.load(os.path.join(HERE, f"encoder_{norm_type}.npz")) as z:
            sd = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
            mel3 = torch.from_numpy(z["mel"])
        enc = build(norm_type, la).eval()
        enc.load_state_dict(sd, strict=True)
        enc64 = build(norm_type, la).double().eval()
        enc64.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
        with torch.no_grad():
            L_out = enc(mel3).shape[2]
        G3 = torch.randn(3, 36, L_out, generator=torch.Generator().manual_seed(900 + ci))
        for N in (3, 1):
            mel, G = mel3[:N], G3[:N]
            out32, g32, _ = grads(enc, mel, G)
            out64, g64, dyabs = grads(enc64, mel.double(), G.double(), hooks=norm_type != "batch")
            fx = {"G": G.numpy(), "case": np.array(case), "additional_context": np.int64(la)}
            for k in g32:
                d = g64[k] - g32[k].double()
                fx["g32/" + k] = g32[k].numpy()
                fx["g64_corr/" + k] = d.float().numpy()
                fx["err/" + k] = np.float64(d.abs().max().item())
            for k, v in dyabs.items():
                fx["dyabs/" + k] = v
            if la and N == 3:
                d = out64 - out32.double()
                np.savez(os.path.join(HERE, f"encoder_train_{case}_out.npz"), out32=out32.numpy(), out64_corr=d.float().numpy(),
                         err_out=np.float64(d.abs().max().item()))
            path = os.path.join(HERE, f"encoder_train_{case}_n{N}.npz")
            np.savez(path, **fx)
            worst = max(g32, key=lambda k: fx["err/" + k])
            print(case, "N", N, "L_out", L_out, "params", len(g32), "hooks", len(dyabs), "worst err %.3g (%s)" % (fx["err/" + worst], worst),
                  os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
