"""Generate tests/golden/lstm_predictor_*.npz by importing the REFERENCE's own rnnt.predictor.LSTMPredictor
(reference rnnt/predictor.py:11-186).

Run on the CPU where the reference is checked out (it never travels to the GPU box):
    PYTHONPATH=<reference checkout> python tests/golden/make_golden_lstm_predictor.py

Stored per case, in three files so that each stays under the repository's size limit.  <case>.npz: ids (with the leading blank the
model prepends), the second call's ids, the module's state_dict (LayerNorm affines perturbed away from the identity) and
`ref_err__<tensor>`: the fp32 module's error against float64, relative to the float64 tensor's largest entry, for the outputs, the
states and every parameter gradient of sum(out * G).  <case>_out.npz: the upstream gradient G (float32 values), the eval-mode
output and final state of the float64 module, and the outputs of a SECOND call fed the first call's state and three more tokens.
<case>_grads.npz: the float64 parameter gradients.  The fp32 module's tensors themselves are not kept, only their errors: the
parity bar of a case is 4 x the largest `ref_err__*` of the case.  Fixtures are data (arrays); no reference source is copied.
"""
import os

import numpy as np
import torch

from rnnt.predictor import LSTMPredictor  # reference, via PYTHONPATH

OUT = os.path.dirname(os.path.abspath(__file__))

CASES = {
    # name: (num_symbols, output_dim, symbol_embedding_dim, num_lstm_layers, lstm_hidden_dim, layer_norm, B, U1, seed)
    "lstm_predictor_small_ln": (40, 48, 32, 2, 32, True, 3, 40, 1),
    "lstm_predictor_noln": (40, 48, 20, 1, 36, False, 5, 7, 2),       # E != Hd, a column tail (4 Hd = 144), x2g bias
    "lstm_predictor_one": (16, 8, 8, 1, 8, True, 1, 1, 3),            # one token from zero state: d p2g == 0
    "lstm_predictor_rows33": (64, 64, 64, 3, 64, True, 33, 24, 4),    # a second 32-row GEMM tile, three layers
}
EPS = 1e-3  # the reference configuration's lstm_layer_norm_epsilon


def rel(a, b):
    m = np.abs(b).max()
    return float(np.abs(a.astype(np.float64) - b).max() / m) if m > 0 else float(np.abs(a).max())


def flat(state):
    return np.stack([np.stack([h.detach().numpy(), c.detach().numpy()]) for h, c in state])  # [L,2,B,Hd]


def make(name, S, O, E, L, Hd, ln, B, U1, seed):
    torch.manual_seed(seed)
    kw = dict(lstm_layer_norm=ln, lstm_layer_norm_epsilon=EPS, lstm_dropout=0.3)
    m = LSTMPredictor(S, O, E, L, Hd, **kw).eval()
    with torch.no_grad():
        for n_, p in m.named_parameters():
            if "norm" in n_:
                p.add_(torch.randn_like(p) * 0.2)
    ids = torch.randint(0, S, (B, U1))
    ids[:, 0] = S - 1
    ids2 = torch.randint(0, S, (B, 3))
    lens, lens2 = torch.full((B,), U1), torch.full((B,), 3)
    G = torch.randn(B, U1, O).double()  # float32 values: stored as float32
    m64 = LSTMPredictor(S, O, E, L, Hd, **kw).double().eval()
    m64.load_state_dict({k: v.double() for k, v in m.state_dict().items()})

    o32, _, s32 = m(ids, lens)
    (o32 * G.float()).sum().backward()
    p32, _, t32 = m(ids2, lens2, [[h.detach(), c.detach()] for h, c in s32])
    o64, _, s64 = m64(ids, lens)
    (o64 * G).sum().backward()
    p64, _, t64 = m64(ids2, lens2, [[h.detach(), c.detach()] for h, c in s64])

    outs = {"G": G.float().numpy()}
    out = {"ids": ids.numpy(), "ids2": ids2.numpy(),
           "dims": np.array([S, O, E, L, Hd, int(ln), B, U1]), "eps": np.array(EPS),
           "keys": np.array(list(m.state_dict().keys()))}
    pairs = {"out": (o32, o64), "state": (flat(s32), flat(s64)), "out2": (p32, p64), "state2": (flat(t32), flat(t64))}
    for k, (a, b) in pairs.items():
        a = a.detach().numpy() if torch.is_tensor(a) else a
        b = b.detach().numpy() if torch.is_tensor(b) else b
        outs[k + "_f64"] = b
        out["ref_err__" + k] = np.array(rel(a, b))
    for k, v in m.state_dict().items():
        out["sd__" + k.replace(".", "__")] = v.numpy()
    grads = {}
    g32 = dict(m.named_parameters())
    for k, p in m64.named_parameters():
        grads["grad__" + k.replace(".", "__")] = p.grad.numpy()
        out["ref_err__grad__" + k.replace(".", "__")] = np.array(rel(g32[k].grad.numpy(), p.grad.numpy()))
    np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
    np.savez_compressed(os.path.join(OUT, name + "_out.npz"), **outs)
    np.savez_compressed(os.path.join(OUT, name + "_grads.npz"), **grads)
    errs = {k[9:]: float(v) for k, v in out.items() if k.startswith("ref_err__")}
    print(name, "worst fp32 error of the reference: %.2e (%s)" % max((v, k) for k, v in errs.items()))


if __name__ == "__main__":
    for k, v in CASES.items():
        make(k, *v)
    for f in sorted(os.listdir(OUT)):
        if f.startswith("lstm_predictor_"):
            print(f, os.path.getsize(os.path.join(OUT, f)))
