"""Cases, oracle and premises of the LSTM device-decode tests (rnnt_engine_greedy_decode_lstm, rnnt_amd/csrc/lstm.hip; DESIGN.md §4p
"Device decode").  Shared by tests/test_lstm_decode_oracle.py (CPU) and tests/test_lstm_decode_gpu.py.

The oracle is the float64 torch path of the same modules driven by the greedy control flow (`greedy_oracle`), which records the gap
between the two largest logits of every decision.  A case is valid only if its smallest gap exceeds lstm_predictor_cases.DECODE_MARGIN:
a condition on the INPUTS — every seed below was picked on the CPU so that it holds — asserted by `checked_oracle` in the CPU test
and again at the head of each GPU test, whose own assertion is then equality of token lists.  Every case states what it is there
for as a premise on its sizes or on the oracle's run, so that a later edit of a tile size or of a seed cannot silently leave the path."""
import collections
import functools
import os

import numpy as np
import torch

from tests import lstm_predictor_cases as lc

GOLDEN = lc.GOLDEN
MARGIN = lc.DECODE_MARGIN
SCAN_TILE = 32     # k_ld_scan: frames and vocabulary entries of a workgroup tile
MAX_UTT = 32       # rnnt_engine_greedy_decode_lstm: utterances per call = the rows of one product tile
# what greedy_decode(device_loop=None) takes for an LSTM model the device loop accepts (RNNTModel.greedy_decode; DESIGN.md §4p "Device decode")
DEFAULT_PATH = "lstm_loop"  # it beat the host loop at both timed lengths (profiles/lstm_decode_bench.txt)

Case = collections.namedtuple("Case", "name spec H V text blank T frame_seed max_length max_per_frame premise")


def _case(name, premise=None, S=None, O=16, E=16, L=1, Hd=32, ln=True, seed=0, H=None, V=16, text=False, blank=None, T=12, frame_seed=1,
          max_length=200, max_per_frame=10):
    H = O if H is None else H
    assert text or O == H, name
    assert E % 4 == 0 and Hd % 4 == 0 and O % 4 == 0 and H % 8 == 0 and V % 4 == 0, name
    spec = dict(S=V if S is None else S, O=O, E=E, L=L, Hd=Hd, ln=ln, eps=1e-3, seed=seed)
    return Case(name, spec, H, V, text, V - 1 if blank is None else blank, T, frame_seed, max_length, max_per_frame, premise)


def build_model(case, dtype=torch.float64):
    """RNNTModel(LSTMPredictor, PassThroughEncoder, JointNetwork) of a case on the CPU, seeded, in eval mode."""
    blank_bias = 50.0 if case.name == "all_blank" else 1.0
    import rnnt_amd
    from tests.stream_models import PassThroughEncoder
    pred = lc.seeded_module(case.spec, torch.float64)
    torch.manual_seed(case.spec["seed"] + 1)
    joint = rnnt_amd.JointNetwork(-1, case.spec["O"] if case.text else -1, case.H, case.V)
    joint.blank_idx = case.blank
    with torch.no_grad():
        joint.joint_ln.bias[case.blank] += blank_bias  # blank often enough that the decode moves through the frames
    return rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint.double()).to(dtype).eval()


def frames_of(H, T, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(1, H, T, generator=g, dtype=torch.float64) * 2.0).to(dtype)


def case_frames(case, dtype=torch.float64):
    return frames_of(case.H, case.T, case.frame_seed, dtype)


Oracle = collections.namedtuple("Oracle", "tokens gap state text per_frame")


@torch.no_grad()
def greedy_oracle(model, mel, max_length, max_per_frame=10):
    """The greedy decode's control flow on the model as it is (any dtype), one decision at a time.  Returns the tokens, the smallest gap
    between the two largest logits of a decision (inf if there was none), the LSTM state after the last label as [L,2,1,Hd], the
    joint's text input after the last label [H], and the labels emitted at each frame."""
    joint, pred = model.joint, model.predictor
    audio = mel.permute(0, 2, 1)
    blank, T = joint.blank_idx, audio.shape[1]
    tokens, gaps, per_frame = [blank], [], [0] * T
    one = torch.tensor([1])
    feats, _, state = pred(torch.tensor([[blank]]), one)
    t = emitted = 0
    while t < T and len(tokens) < max_length:
        if emitted >= max_per_frame:
            t, emitted = t + 1, 0
            continue
        logits = joint.single_forward(audio[:, t, :], feats[:, -1, :])[0]
        top = logits.topk(2).values
        gaps.append(float(top[0] - top[1]))
        tok = int(logits.argmax())
        if tok == blank:
            t, emitted = t + 1, 0
            continue
        tokens.append(tok)
        per_frame[t] += 1
        feats, _, state = pred(torch.tensor([[tok]]), one, state)
        emitted += 1
    text = feats[0, -1]
    if hasattr(joint, "text_ln"):
        text = joint.text_ln(text)
    return Oracle(tokens[1:], min(gaps) if gaps else float("inf"), lc.flat_state(state), text.numpy(), per_frame)


def checked_oracle(case, model=None, mel=None):
    """The float64 oracle of a case with its premises asserted: the margin, and what the case is there for."""
    model = build_model(case) if model is None else model
    mel = case_frames(case) if mel is None else mel
    o = greedy_oracle(model, mel, case.max_length, case.max_per_frame)
    assert o.gap > MARGIN, (case.name, o.gap)
    if case.premise is not None:
        assert case.premise(case, o), (case.name, o.tokens, o.per_frame)
    return o


@torch.no_grad()
def replay(model, tokens):
    """(state [L,2,1,Hd], text [H]) of the model's predictor (any dtype, CPU) fed the start blank and `tokens` from zero state."""
    ids = torch.tensor([[model.joint.blank_idx] + list(tokens)])
    feats, _, state = model.predictor(ids, torch.tensor([ids.shape[1]]))
    text = feats[0, -1]
    if hasattr(model.joint, "text_ln"):
        text = model.joint.text_ln(text)
    return lc.flat_state(state), text.numpy()


def _labels(lo, kinds=3):
    return lambda c, o: len(o.tokens) >= lo and len(set(o.tokens)) >= min(kinds, lo)


def _tiles(n, tile):
    return -(-n // tile)


# ---- the cases: the smallest shapes at which the loop can go wrong ----------------------------------------------------------------------
WIRING_TEXT = _case("wiring_text", lambda c, o: c.text and c.spec["O"] != c.H and _labels(6)(c, o), S=16, O=32, E=16, L=2, Hd=32, seed=7,
                    H=24, text=True, T=14, frame_seed=3)

WIDTHS = [
    # column tails of the 32-wide tiles (4 Hd = 144), contractions that end inside a chunk of 8 (E = 20, Hd = 36); V = 20: one vocabulary
    # tile with a tail
    _case("hd36_e20", lambda c, o: (4 * c.spec["Hd"]) % lc.REC_TILE == 16 and c.spec["E"] % lc.K_CHUNK == 4 and c.spec["Hd"] % lc.K_CHUNK == 4
          and c.V % SCAN_TILE == 20 and _labels(4)(c, o), Hd=36, E=20, V=20, seed=11, frame_seed=3),
    # one and two passes of the row kernel; V = 40: two vocabulary tiles, the second with 8 entries
    _case("hd256", lambda c, o: c.spec["Hd"] == lc.UNIT_PASS and lc.rec_splits(c.spec["Hd"]) == 2 and _tiles(c.V, SCAN_TILE) == 2
          and c.V % SCAN_TILE == 8 and _labels(4)(c, o), Hd=256, V=40, seed=12, frame_seed=1),
    _case("hd260", lambda c, o: lc.UNIT_PASS < c.spec["Hd"] < lc.UNIT_PASS + 64 and lc.rec_splits(c.spec["Hd"]) == 3 and _labels(4)(c, o),
          Hd=260, seed=13, frame_seed=1),
    # three layers without layer norm: layer 0 reads E columns, the others Hd; the x2g bias
    _case("l3_noln", lambda c, o: c.spec["L"] == 3 and not c.spec["ln"] and c.spec["E"] != c.spec["Hd"] and _labels(4)(c, o), L=3, ln=False,
          E=24, seed=22, frame_seed=2),
]

CONTROL = [
    # the cap: max_length = 2 ends after one label; a cap in the middle of an utterance that would go on
    _case("max_length_2", lambda c, o: len(o.tokens) == 1, L=2, seed=7, max_length=2, frame_seed=5),
    _case("cap_mid", lambda c, o: len(o.tokens) == c.max_length - 1
          and len(greedy_oracle(build_model(c), case_frames(c), 200).tokens) > len(o.tokens) + 1, L=2, seed=7, max_length=5,
          frame_seed=5),
    # max_per_frame = 2 reached: the oracle emits exactly that many at some frame (and never more)
    _case("per_frame_2", lambda c, o: max(o.per_frame) == 2, L=2, seed=7, max_per_frame=2, frame_seed=5),
    _case("t1", lambda c, o: c.T == 1, L=2, seed=7, T=1, frame_seed=5),
    # a blank other than V - 1 (JointNetwork.blank_idx is an attribute the decode paths read)
    _case("blank_5", lambda c, o: c.blank == 5 != c.V - 1 and _labels(4)(c, o) and 5 not in o.tokens, L=2, seed=7, blank=5, frame_seed=5),
]
ALL_BLANK = _case("all_blank", lambda c, o: o.tokens == [] and c.T > 1, L=2, seed=7, frame_seed=5)  # (build_model: blank's bias + 50)
SCAN_FRAMES = (1, 5, 32, 128)  # one frame per iteration; no divisor of T; the tile; the ABI's limit (beyond T)
BY_NAME = {c.name: c for c in [WIRING_TEXT, ALL_BLANK] + WIDTHS + CONTROL}

# ---- a batch: utterances of ONE model (lc.wiring_model), ragged lengths, T = 1 next to the longest
BATCH_T = [23, 1, 9, 14, 2, 17, 5, 11, 20, 3, 8, 13, 6, 19, 4, 10, 16, 7, 12, 15, 1, 22, 9, 18, 2, 21, 5, 14, 11, 3, 17, 23, 6]
BATCH_SEEDS = [101, 102, 105, 107, 108, 110, 111, 112, 113, 114, 115, 117, 118, 125, 126, 129, 131, 132, 140, 146, 147, 148, 149, 150, 151, 154,
               155, 156, 157, 158, 159, 161, 162]  # frames_of(H, BATCH_T[i], BATCH_SEEDS[i])
BATCH_SIZES = (1, 2, 31, 32)
assert len(BATCH_T) == len(BATCH_SEEDS) == MAX_UTT + 1 and BATCH_T[1] == 1 and BATCH_T[0] == max(BATCH_T) and BATCH_T[31] == max(BATCH_T)


def batch_mels(dtype=torch.float64):
    return [frames_of(lc.DECODE_SPEC["O"], T, s, dtype) for T, s in zip(BATCH_T, BATCH_SEEDS)]


@functools.lru_cache(maxsize=None)
def batch_oracles():
    """The 33 utterances' float64 oracles (computed once), every one above the margin; between them they emit labels and stay silent."""
    model = lc.wiring_model()
    out = [greedy_oracle(model, mel, 200) for mel in batch_mels()]
    assert all(o.gap > MARGIN for o in out), [o.gap for o in out]
    assert sum(len(o.tokens) > 0 for o in out) >= 24 and len({tuple(o.tokens) for o in out}) >= 16
    return out


# ---- the reference configuration's widths (config/basic_sp.yaml), four utterances
REF_CASE = _case("reference_widths", None, S=1024, O=1024, E=512, L=3, Hd=512, V=1024, seed=31, T=64)
REF_FRAME_SEEDS = (216, 205, 237, 204)  # of seeds 200 .. 239 the four with the largest float64 gaps (1.6e-3 .. 3.5e-3)


def load_golden(name):
    """tests/golden/decode_lstm_<name>.npz (tests/golden/make_golden_decode_lstm.py): the REFERENCE's modules' own decode."""
    with np.load(os.path.join(GOLDEN, f"decode_lstm_{name}.npz")) as z:
        return {k: z[k] for k in z.files}


GOLDENS = ("ln", "text_noln")


def golden_model(fx, dtype=torch.float64):
    """The project's modules with a golden's state dicts loaded (strict), and its frames (1, H, T)."""
    import rnnt_amd
    from tests.stream_models import PassThroughEncoder
    S, O, E, L, Hd, ln, H, V, text = (int(v) for v in fx["dims"])
    pred = rnnt_amd.LSTMPredictor(S, O, E, L, Hd, lstm_layer_norm=bool(ln), lstm_layer_norm_epsilon=float(fx["eps"]), lstm_dropout=0.3)
    pred.load_state_dict({str(k): torch.from_numpy(fx["pred__" + str(k).replace(".", "__")]) for k in fx["pred_keys"]}, strict=True)
    joint = rnnt_amd.JointNetwork(-1, O if text else -1, H, V)
    joint.load_state_dict({str(k): torch.from_numpy(fx["joint__" + str(k).replace(".", "__")]) for k in fx["joint_keys"]}, strict=True)
    model = rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint).to(dtype).eval()
    return model, torch.from_numpy(fx["frames"]).to(dtype)
