"""Decode cases with the blank moved away from V - 1, and the seeded cases built on them (TEST INFRASTRUCTURE ONLY).

Shared by tests/test_decode_relabel_oracle.py (CPU: the premises — the oracles commute with the relabelling, gaps, margins, which ids
appear where) and tests/test_decode_blank_gpu.py (the device paths at those blanks).  Everything here is a function of committed
fixtures and numpy seeds; nothing is stored.

The greedy decode and the beam search are functions of the logits' VALUES and of the order of the class indices (argmax and the label
lists take the lower index at equal values; the search breaks ties by token id).  tests.helpers.blank_index_map moves the blank and
keeps the order among the labels, so the relabelled problem's results are the mapped results of the original one — up to the rounding
of a float64 sum over the vocabulary in another order (log-sum-exp: ~1e-15).
"""
import numpy as np

from oracle import decode_oracle
from tests import beam_oracle
from tests.helpers import blank_index_map, decode_case_arrays

GAP = 1e-3     # tests/test_beam_gpu.py's bar: the smallest oracle gap for which identical n-best lists are demanded
MARGIN = 1e-3  # tests/test_decode_gpu.py's bar: the smallest top-2 logit gap for which identical greedy lists are demanded

# ---- section "blank position": (case, the blanks it is run at).  V = 32: one blank per position of a float4 quad
BLANKS = {"decode_small": (0, 5, 15, 30), "decode_cap": (0, 5, 15, 30), "decode_small_proj": (0, 129, 298)}
WIDE_BLANK = 1001        # decode_wide_vocab (V = 4000): the chunk of k_beam_reduce's wave 3 (768 .. 1023), quad position 1
REF_WIDTHS_BLANK = 0     # decode_ref_widths_proj, max_length 25 only
SMALL_BEAMS = (1, 4, 8)
BEAM_ML = {"decode_small": 60, "decode_small_proj": 60, "decode_cap": 37}  # the max_length of each case's beam configurations

# ---- section "beam widths that are not powers of two": (case, max_length, widths); every width's oracle gap is above GAP (asserted on the
# CPU).  7 and 15 of decode_small_proj and 15 of decode_cap fall below it on the oracle alone and are left out.
ODD_BEAMS = [("decode_small", 60, (3, 5, 7, 11, 13, 15)), ("decode_small_proj", 60, (3, 5, 6, 12, 13)), ("decode_cap", 37, (3, 5, 7, 13))]
ODD_BEAMS_MOVED = ("decode_small", 60, 5, (3, 13))  # (case, max_length, blank, widths): once at a moved blank


def _move(a, new_of_old):
    out = np.empty_like(a)
    out[new_of_old] = a
    return out


def relabel_decode_case(case, blank):
    """`case`: a tests.helpers.load_decode_case dict, or the (frames, pred_sd, joint_sd) triple of decode_case_arrays (blank = V - 1).
    Returns the same problem with the blank at `blank`: the rows of embedding.weight, joint_ln.weight and joint_ln.bias moved by
    blank_index_map (new[new_of_old] = old), every stored token list mapped; frames and margins as they are.  A dict gives a dict with
    `blank` and `new_of_old` added, a triple gives (frames, pred_sd, joint_sd, new_of_old)."""
    is_dict = isinstance(case, dict)
    frames, pred_sd, joint_sd = (case["frames"], case["pred_sd"], case["joint_sd"]) if is_dict else case
    V = joint_sd["joint_ln.weight"].shape[0]
    assert pred_sd["embedding.weight"].shape[0] == V
    new_of_old = blank_index_map(V, blank)
    blank = int(new_of_old[V - 1])
    pred, joint = dict(pred_sd), dict(joint_sd)
    pred["embedding.weight"] = _move(pred_sd["embedding.weight"], new_of_old)
    joint["joint_ln.weight"] = _move(joint_sd["joint_ln.weight"], new_of_old)
    joint["joint_ln.bias"] = _move(joint_sd["joint_ln.bias"], new_of_old)
    if not is_dict:
        return frames, pred, joint, new_of_old
    r = dict(case, pred_sd=pred, joint_sd=joint, blank=blank, new_of_old=new_of_old)
    r["tokens"] = {ml: map_tokens(t, new_of_old) for ml, t in case["tokens"].items()}
    return r


def map_tokens(tokens, new_of_old):
    return [int(new_of_old[k]) for k in tokens]


def map_nbest(nbest, new_of_old):
    return [(map_tokens(y, new_of_old), s) for y, s in nbest]


def map_phrases(phrases, new_of_old, blank):
    """A phrase list in the V - 1 labelling -> the labelling with the blank at `blank`, plus one phrase of the blank's neighbours
    (blank - 1, blank + 1, each where it exists)."""
    V = len(new_of_old)
    extra = tuple(k for k in (blank - 1, blank + 1) if 0 <= k < V)
    return [tuple(int(new_of_old[k]) for k in ph) for ph in phrases] + [extra]


def build_relabelled(spec, pred_sd, joint_sd, blank):
    """tests.test_decode_gpu.build_model of (already relabelled) state dicts, told where the blank is before its first decode."""
    from tests.test_decode_gpu import build_model
    model = build_model(spec, pred_sd, joint_sd)
    model.joint.blank_idx = int(blank)
    return model


def oracle_model(frames, pred_sd, joint_sd, blank):
    om = beam_oracle.Model(frames, pred_sd, joint_sd)
    om.blank = int(blank)  # (read by feat(), by beam_oracle.beam_search and by context_oracle.beam_search)
    return om


# ---- the oracles' results, computed once per process and never changed: (case, blank) with blank None = the fixture as stored (V - 1)
# context biasing: one configuration of tests/context_oracle.CONFIGS per small case — name: (max_length, phrases key, score)
CONTEXT = {"decode_small": (60, "decode_small", 1.5), "decode_cap": (37, "decode_cap", 1.5), "decode_small_proj": (60, "decode_small_proj", 3.0)}
CONTEXT_BEAMS = (1, 4, 8)
CONTEXT_LEFT_OUT = {("decode_small", 0, 8)}  # (case, blank, beam): the oracle's gap with that blank's phrase list is 2.1e-4, below GAP


def context_beams(name, blank):
    return tuple(b for b in CONTEXT_BEAMS if (name, blank, b) not in CONTEXT_LEFT_OUT)


_cases, _models, _beams, _contexts = {}, {}, {}, {}


def case_at(golden_dir, name, blank=None):
    from tests.helpers import load_decode_case
    if (name, None) not in _cases:
        c = load_decode_case(golden_dir, name)
        V = c["spec"]["V"]
        _cases[name, None] = dict(c, blank=V - 1, new_of_old=np.arange(V))
    if (name, blank) not in _cases:
        _cases[name, blank] = relabel_decode_case(_cases[name, None], blank)
    return _cases[name, blank]


def model_at(golden_dir, name, blank=None):
    if (name, blank) not in _models:
        c = case_at(golden_dir, name, blank)
        _models[name, blank] = oracle_model(c["frames"], c["pred_sd"], c["joint_sd"], c["blank"])
    return _models[name, blank]


def beam_at(golden_dir, name, blank, beam, ml):
    """-> (n-best, pruned, gap) of tests/beam_oracle.beam_search on the case relabelled to `blank`"""
    k = (name, blank, beam, ml)
    if k not in _beams:
        _beams[k] = oracle_search(model_at(golden_dir, name, blank), beam, ml)
    return _beams[k]


def oracle_search(om, beam, ml):
    """-> (n-best, pruned, gap) of tests/beam_oracle.beam_search; for a vocabulary in the thousands through its restatement with a shortlist
    per row (tests/context_oracle.beam_search without a graph: the same floats, tests/test_beam_context_oracle.py, in a tenth of the time)"""
    if om.V < 4000:
        return beam_oracle.beam_search(om, beam, ml)
    from tests import context_oracle as co
    r = co.beam_search(om, beam, ml)
    return r.nbest, r.pruned, r.gap


def context_at(golden_dir, name, blank, beam):
    """-> (tests/context_oracle's Result, the phrases, the score): CONTEXT[name] with its phrases mapped to the labelling with the blank at
    `blank` and one phrase of the blank's neighbours more"""
    from tests import context_oracle as co
    ml, key, score = CONTEXT[name]
    c = case_at(golden_dir, name, blank)
    phrases = map_phrases(co.PHRASES[key], c["new_of_old"], c["blank"])
    k = (name, blank, beam)
    if k not in _contexts:
        _contexts[k] = co.beam_search(model_at(golden_dir, name, blank), beam, ml, graph=co.Trie(phrases, score))
    return _contexts[k], phrases, score


# ---- section "a vocabulary beyond one pass of k_beam_reduce": a wave walks c0 = wave * 256, + 4096, ...: at V = 4100 wave 0 owns
# [0, 256) and, on its second trip, the four entries 4096 .. 4099; at V = 8196 it makes a third trip for 8192 .. 8195.  joint_ln.bias is
# raised on a HOT set with members in each of wave 0's trips by (max - mean) of the frame-0 logits, and on the blank (V - 1) by BLANK_SHARE
# of that.  Seeds (of 4400 .. 4407) and share (of 0.3 .. 1.03) were picked on the CPU, on the oracles alone;
# tests/test_decode_relabel_oracle.py asserts what they were picked for.
BEYOND = {
    4100: dict(spec=dict(V=4100, E=32, O=64, H=64, fa=-1, ft=-1, T=12, w_scale=30.0), seed=4401, hot=(2, 130, 4096, 4097, 4098),
               beams=(4, 7, 16), ml=60, windows=3),
    8196: dict(spec=dict(V=8196, E=32, O=64, H=64, fa=-1, ft=-1, T=12, w_scale=30.0), seed=4406, hot=(2, 130, 4096, 4097, 8192, 8193, 8194),
               beams=(4,), ml=60, windows=3),
}
BLANK_SHARE = 1.0
BEYOND_MOVED_BLANK = 4097  # V = 4100 once more: the blank inside the four-entry tail of the second trip


def beyond_one_pass_case(V, blank=None):
    """-> dict(spec, frames, pred_sd, joint_sd, blank, ml, beams, windows) of BEYOND[V], the blank at V - 1 or relabelled to `blank`."""
    cfg = BEYOND[V]
    frames, pred_sd, joint_sd = decode_case_arrays(cfg["spec"], cfg["seed"], 0.0)
    x = decode_oracle.single_forward(frames[0].astype(np.float64), oracle_model(frames, pred_sd, joint_sd, V - 1).feat([]),
                                     {k: np.asarray(v, dtype=np.float64) for k, v in joint_sd.items()})
    boost = np.float32(x.max() - x.mean())
    bias = joint_sd["joint_ln.bias"].copy()
    bias[list(cfg["hot"])] += boost
    bias[V - 1] += np.float32(BLANK_SHARE) * boost
    joint_sd = dict(joint_sd, **{"joint_ln.bias": bias})
    new_of_old = np.arange(V)
    if blank is not None:
        frames, pred_sd, joint_sd, new_of_old = relabel_decode_case((frames, pred_sd, joint_sd), blank)
    return dict(spec=cfg["spec"], frames=frames, pred_sd=pred_sd, joint_sd=joint_sd, blank=V - 1 if blank is None else blank,
                ml=cfg["ml"], beams=cfg["beams"], windows=cfg["windows"], new_of_old=new_of_old)


def beyond_windows(frames, n):
    """The first n utterances of beam_search_many's runs on a BEYOND case: all frames, the second half, the first third reversed."""
    T = frames.shape[0]
    return [frames.copy(), frames[T // 2:].copy(), frames[:T // 3][::-1].copy()][:n]


# ---- section "exact ties": decode_small with the blank at `blank` and two classes (a, b) given all-zero rows of joint_ln.weight and one
# bias TIE_BIAS — their logits are exactly that bias on every path, whatever its summation order (0 * finite = 0, acc + 0 = acc).
#   blank_first  blank 5, label 20:  the blank wins every tie (lower index): the frame ends
#   label_first  blank 20, label 5:  the label wins every tie, up to the 10-per-frame cap
#   two_labels   blank 12, labels 7 and 20: the tie never involves the blank — the one the label lists of k_beam_reduce (beam_before) see
TIES = {"blank_first": dict(blank=5, pair=(5, 20)), "label_first": dict(blank=20, pair=(5, 20)), "two_labels": dict(blank=12, pair=(7, 20))}
TIE_BIAS = 12.0  # of 9 .. 16 the value at which the pair leads 0.40 / 0.66 / 0.43 of the three variants' decisions (asserted on the CPU)


def tied_case(case, variant):
    """`case`: load_decode_case(golden_dir, "decode_small").  -> the relabelled dict with the tied pair written in and `pair` added."""
    cfg = TIES[variant]
    r = relabel_decode_case(case, cfg["blank"])
    W, b = r["joint_sd"]["joint_ln.weight"].copy(), r["joint_sd"]["joint_ln.bias"].copy()
    for k in cfg["pair"]:
        W[k] = 0.0
        b[k] = np.float32(TIE_BIAS)
    r["joint_sd"] = dict(r["joint_sd"], **{"joint_ln.weight": W, "joint_ln.bias": b})
    r["pair"] = cfg["pair"]
    r.pop("tokens")  # (another problem than the fixture's: its lists come from the oracle)
    return r


def tied_greedy(r, ml):
    """-> (tokens, margins to the best logit outside the pair, share of decisions at which the pair is the maximum)"""
    want, margins = decode_oracle.greedy_decode(r["frames"], r["pred_sd"], r["joint_sd"], max_length=ml, blank=r["blank"], tied=r["pair"])
    _, plain = decode_oracle.greedy_decode(r["frames"], r["pred_sd"], r["joint_sd"], max_length=ml, blank=r["blank"])
    return want, margins, float((plain == 0.0).mean())
