"""Fixtures, error measure and edge shapes of the LSTMPredictor tests (rnnt_amd/lstm_predictor.py, rnnt_amd/csrc/lstm.hip).  Shared
by tests/test_lstm_predictor_oracle.py (CPU) and tests/test_lstm_predictor_gpu.py.  Every edge case states its premise as an
assert, so that a later edit of the kernels' tile or pass sizes cannot silently leave the path the case is there for."""
import collections
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURES = ("small_ln", "noln", "one", "rows33")  # tests/golden/make_golden_lstm_predictor.py

# the kernels' sizes restated (rnnt_amd/csrc/lstm.hip, smallgemm.hip): a change there fails a premise here, which is the point
ROW_TILE = 32        # k_sgemm_nt / k_sgemm_nn / k_rec_gemm: rows of a workgroup tile
COL_TILE = 128       # k_sgemm_nt (x2g, linear): columns of a workgroup tile
REC_TILE = 32        # k_rec_gemm (the recurrent products): columns of a workgroup tile
K_CHUNK = 8          # contraction elements per chunk
UNIT_PASS = 256      # k_lstm_step_*: hidden units per pass of a workgroup (unit j = tid + 256 k)
MAX_HIDDEN, MAX_EMBED, MAX_LAYERS = 1024, 2048, 8


def load(name):
    """A fixture as one dict: the three files of tests/golden/lstm_predictor_<name>*.npz merged."""
    out = {}
    for suffix in ("", "_out", "_grads"):
        with np.load(os.path.join(GOLDEN, f"lstm_predictor_{name}{suffix}.npz")) as z:
            out.update({k: z[k] for k in z.files})
    S, O, E, L, Hd, ln, B, U1 = (int(v) for v in out["dims"])
    out["spec"] = dict(S=S, O=O, E=E, L=L, Hd=Hd, ln=bool(ln), B=B, U1=U1, eps=float(out["eps"]))
    return out


def fixture_bar(fx):
    """4 x the largest relative error the REFERENCE's fp32 module shows in the case (over its outputs, states and gradients)."""
    return 4.0 * max(float(v) for k, v in fx.items() if k.startswith("ref_err__"))


def state_dict_of(fx, dtype):
    return {str(k): torch.from_numpy(fx["sd__" + str(k).replace(".", "__")]).to(dtype) for k in fx["keys"]}


def module_of(spec, dropout=0.3):
    import rnnt_amd
    return rnnt_amd.LSTMPredictor(spec["S"], spec["O"], spec["E"], spec["L"], spec["Hd"], lstm_layer_norm=spec["ln"],
                                  lstm_layer_norm_epsilon=spec["eps"], lstm_dropout=dropout)


def fixture_module(fx, dtype=torch.float64):
    m = module_of(fx["spec"]).to(dtype)
    m.load_state_dict(state_dict_of(fx, dtype), strict=True)
    return m.eval()


def seeded_module(spec, dtype=torch.float64, dropout=0.3):
    """The module with seeded parameters, its LayerNorm affines (and biases) moved away from the identity."""
    torch.manual_seed(spec["seed"])
    m = module_of(spec, dropout)
    with torch.no_grad():
        for n, p in m.named_parameters():
            if "norm" in n:
                p.add_(torch.randn_like(p) * 0.2)
    return m.to(dtype).eval()


def rel_err(got, ref):
    """max |got - ref| relative to ref's largest entry (ref float64); an identically zero ref demands exact zeros (error inf otherwise)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert np.isfinite(got).all(), "non-finite values"
    m = np.abs(ref).max() if ref.size else 0.0
    if m == 0.0:
        return 0.0 if not np.any(got) else float("inf")
    return float(np.abs(got - ref).max() / m)


def flat_state(state):
    return np.stack([np.stack([h.detach().cpu().numpy(), c.detach().cpu().numpy()]) for h, c in state])  # [L,2,B,Hd]


def run(m, ids, G, state=None, keep_masks=None):
    """Forward + backward of sum(out * G) on the module as it is (device, dtype, backend): {name: numpy array} of the output, the
    state and every parameter gradient."""
    m.zero_grad(set_to_none=True)
    dev, dtype = m.embedding.weight.device, m.embedding.weight.dtype
    ids = torch.as_tensor(ids).to(dev)
    lens = torch.full((ids.shape[0],), ids.shape[1], device=dev)
    if state is not None:
        state = [[torch.as_tensor(h).to(dev, dtype), torch.as_tensor(c).to(dev, dtype)] for h, c in state]
    if keep_masks is not None:
        keep_masks = torch.as_tensor(keep_masks).to(dev)
    out, lens_out, st = m(ids, lens, state, keep_masks=keep_masks)
    assert lens_out is lens
    (out * torch.as_tensor(G).to(dev, dtype)).sum().backward()
    res = {"out": out.detach().cpu().numpy(), "state": flat_state(st)}
    for n, p in m.named_parameters():
        res["grad__" + n.replace(".", "__")] = p.grad.detach().cpu().numpy()
    return res


# ---- edge shapes -------------------------------------------------------------------------------------------------------------
Edge = collections.namedtuple("Edge", "name spec with_state")


def _edge(name, premise, S=24, O=16, E=16, L=1, Hd=32, ln=True, B=2, U1=3, seed=0, with_state=False):
    assert E % 4 == 0 and Hd % 4 == 0 and O % 4 == 0 and Hd <= MAX_HIDDEN and E <= MAX_EMBED and L <= MAX_LAYERS, name
    spec = dict(S=S, O=O, E=E, L=L, Hd=Hd, ln=ln, B=B, U1=U1, eps=1e-3, seed=seed)
    assert premise(spec), name
    return Edge(name, spec, with_state)


def _tiles(n, tile):
    return -(-n // tile)


def rec_splits(K):
    """lstm.hip rec_splits: the contraction ranges of a recurrent product over K (K = Hd forward, 4 Hd backward); a wave of a range
    walks its chunks four at a time."""
    return min(16, max(1, -(-_tiles(K, K_CHUNK) // 16)))


def rec_groups(K):
    """Groups of four chunks the busiest wave of k_rec_gemm walks."""
    return -(-_tiles(K, K_CHUNK) // (16 * rec_splits(K)))


EDGES = [
    # 4 Hd = 144: one whole 128-column tile and a 16-column tail; E = 20: the x2g contraction ends inside a chunk of 8; E != Hd
    # the recurrent products: a 16-column tail forward, a 4-column tail backward, contractions that end inside a chunk
    _edge("hd36_e20", lambda s: (4 * s["Hd"]) % COL_TILE == 16 and _tiles(4 * s["Hd"], COL_TILE) == 2 and s["E"] % K_CHUNK == 4
          and s["E"] != s["Hd"] and (4 * s["Hd"]) % REC_TILE == 16 and s["Hd"] % REC_TILE == 4 and s["Hd"] % K_CHUNK == 4
          and rec_splits(4 * s["Hd"]) == 2, Hd=36, E=20, B=3, U1=5, seed=11),
    # Hd = 256: exactly one pass of the row kernels; 260: a second pass with 4 live threads, 4 Hd = 1040 beyond 1024 columns
    # (the recurrent products: 2 full contraction ranges forward at 256; 3 at 260, the third with one chunk and a half)
    _edge("hd256", lambda s: s["Hd"] == UNIT_PASS and rec_splits(s["Hd"]) == 2 and s["Hd"] % (16 * K_CHUNK) == 0, Hd=256, seed=12),
    _edge("hd260", lambda s: UNIT_PASS < s["Hd"] < UNIT_PASS + 64 and 4 * s["Hd"] > 1024 and rec_splits(s["Hd"]) == 3
          and s["Hd"] % K_CHUNK == 4, Hd=260, seed=13),
    # batch rows against the 32-row GEMM tile of the recurrent products
    _edge("b1", lambda s: s["B"] == 1, B=1, seed=14),
    _edge("b31", lambda s: s["B"] == ROW_TILE - 1, B=31, seed=15),
    _edge("b32", lambda s: s["B"] == ROW_TILE, B=32, seed=16),
    _edge("b33_state", lambda s: s["B"] == ROW_TILE + 1 and _tiles(s["B"], ROW_TILE) == 2, B=33, seed=17, with_state=True),
    # one step (no recurrent launch without a state) and two
    _edge("u1", lambda s: s["U1"] == 1, U1=1, seed=18),
    _edge("u1_state", lambda s: s["U1"] == 1, U1=1, seed=19, with_state=True),
    _edge("u2", lambda s: s["U1"] == 2, U1=2, seed=20),
    # layers: one, three (layer 0 reads E columns, the others Hd), without layer norm too
    _edge("l3", lambda s: s["L"] == 3 and s["E"] != s["Hd"], L=3, E=24, U1=4, seed=21),
    _edge("l3_noln_state", lambda s: s["L"] == 3 and not s["ln"], L=3, ln=False, U1=4, seed=22, with_state=True),
    # the limit of the hidden width: four full passes of the row kernels; the backward's recurrent product at its cap of 16 ranges,
    # each wave walking two groups of four chunks
    _edge("hd1024", lambda s: s["Hd"] == MAX_HIDDEN and s["B"] == 2 and s["U1"] == 2 and rec_splits(4 * s["Hd"]) == 16
          and rec_groups(4 * s["Hd"]) == 2 and rec_groups(s["Hd"]) == 1, Hd=1024, S=16, E=8, O=8, B=2, U1=2, seed=23),
]


def edge_inputs(e):
    """(ids, G, state or None) of an edge case, seeded."""
    s = e.spec
    g = torch.Generator().manual_seed(1000 + s["seed"])
    ids = torch.randint(0, s["S"], (s["B"], s["U1"]), generator=g)
    G = torch.randn(s["B"], s["U1"], s["O"], generator=g).double()
    state = None
    if e.with_state:
        state = [[torch.randn(s["B"], s["Hd"], generator=g).double() * 0.5, torch.randn(s["B"], s["Hd"], generator=g).double()]
                 for _ in range(s["L"])]
    return ids, G, state


# ---- a small model for the wiring tests --------------------------------------------------------------------------------------
DECODE_SPEC = dict(S=16, O=32, E=16, L=2, Hd=32, ln=True, eps=1e-3, seed=7)  # V = S = 16, joint width H = O
DECODE_FRAMES, DECODE_SEED, DECODE_MARGIN = 14, 5, 1e-3  # seed picked on the CPU: the float64 decode keeps a top-2 gap of 2.6e-2


def wiring_model(dtype=torch.float64):
    """RNNTModel(LSTMPredictor, PassThroughEncoder, JointNetwork) on the CPU with seeded parameters (eval mode)."""
    import rnnt_amd
    from tests.stream_models import PassThroughEncoder
    pred = seeded_module(DECODE_SPEC, dtype)
    torch.manual_seed(DECODE_SPEC["seed"] + 1)
    joint = rnnt_amd.JointNetwork(-1, -1, DECODE_SPEC["O"], DECODE_SPEC["S"])
    with torch.no_grad():
        joint.joint_ln.bias[-1] += 1.0  # blank often enough that the decode moves through the frames
    joint = joint.to(dtype)
    return rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint).eval()


def decode_frames(dtype=torch.float64):
    g = torch.Generator().manual_seed(DECODE_SEED)
    return (torch.randn(1, DECODE_SPEC["O"], DECODE_FRAMES, generator=g, dtype=torch.float64) * 2.0).to(dtype)


def greedy_with_margins(model, mel, max_length):
    """The greedy decode's control flow (at most 10 labels per frame) on the model as it is, recording the gap between the two largest
    logits of every decision: (tokens, smallest gap)."""
    audio = mel.permute(0, 2, 1)
    blank, tokens, gaps = model.joint.blank_idx, [model.joint.blank_idx], []
    one = torch.tensor([1])
    feats, _, state = model.predictor(torch.tensor([[blank]]), one)
    t, emitted = 0, 0
    while t < audio.shape[1] and len(tokens) < max_length:
        if emitted >= 10:
            t, emitted = t + 1, 0
            continue
        logits = model.joint.single_forward(audio[:, t, :], feats[:, -1, :])[0]
        top = logits.topk(2).values
        gaps.append(float(top[0] - top[1]))
        tok = int(logits.argmax())
        if tok == blank:
            t, emitted = t + 1, 0
            continue
        tokens.append(tok)
        feats, _, state = model.predictor(torch.tensor([[tok]]), one, state)
        emitted += 1
    return tokens[1:], min(gaps)
