"""Record every byte the encoder's entries leave behind, for tests/test_encoder_bits_gpu.py: the inference and the training halves of
rnnt_amd/csrc/encoder.hip share one epilogue body, one conv launch and one pack kernel, and every sum in the file has a fixed order, so
its source can be rearranged freely as long as every case keeps every bit.

Run once on a GPU with the library whose output is the reference (RNNT_ENGINE_LIB = the build of the commit BEFORE the change):
    python tests/golden/make_golden_encoder_bits.py
writes tests/golden/encoder_bits.npz.  No shapes of its own: the cases are those of the layer tests, run by their abi_run helpers
(tests/test_encoder_layers_gpu.py, tests/test_encoder_train_layers_gpu.py), which own every buffer, size it by the size queries and
pre-fill it with signalling NaNs:
  layer/...   every (name, norm kind, layout) of encoder_layer_cases.case_ids(layouts_too=True) in every regime the case lists
  chain/...   the streaming chains of test_streaming_chain, push by push from zero state
  train/...   every (name, kind) of encoder_train_cases.case_ids(), forward and backward, the forward in both regimes
Per case: `out`, every new streaming state, the WHOLE workspace after the call (exactly the bytes the size query reports: slabs, parked
activations, the residual buffer), for training also the whole `saved` block, every gradient and the workspace after the backward; the
packed tables of rnnt_engine_encoder_pack / _train_pack; and the sizes the size queries return.  Sizes are kept as numbers, every buffer
as the SHA-256 of its bytes.

A case is written only if its result passes the float64 bar of the test it comes from (ec.bar, C.bars) and a second run gives the same
bytes.  So a broken build cannot be recorded.  This module is also the test's source of the cases and of the code that runs them.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import encoder_layer_cases as ec  # noqa: E402
from tests import encoder_train_cases as C  # noqa: E402
from tests.helpers import sha256_of_arrays  # noqa: E402

GOLDEN = os.path.join(HERE, "encoder_bits.npz")
CHAIN_NORMS = ("none", "batch")  # test_streaming_chain's


def cases():
    """{case id: (family, arguments)}"""
    out = {}
    for cid in ec.case_ids(layouts_too=True):
        for regime in ec.SHAPES[cid[0]][4]:
            out["layer/%s-%s" % ("-".join(cid), ec.REGIME_NAMES[regime])] = ("layer", (cid, regime))
    for name in ec.CHAIN_CASES:
        for norm in CHAIN_NORMS:
            for regime in (ec.AUTO, ec.MANY_ROWS):
                out["chain/%s-%s-%s" % (name, norm, ec.REGIME_NAMES[regime])] = ("chain", (name, norm, regime))
    for name, kind in C.case_ids():
        for regime in (ec.AUTO, ec.MANY_ROWS):
            out["train/%s-%s-%s" % (name, kind, ec.REGIME_NAMES[regime])] = ("train", (name, kind, regime))
    return out


CASES = cases()


def _sha(t):
    return sha256_of_arrays(t.contiguous().view(-1).cpu().numpy())


def _layer_fields(got, prefix=""):
    f = {prefix + "out": _sha(got.out), prefix + "workspace": _sha(got.workspace), prefix + "packed": _sha(got.packed)}
    for i, s in enumerate(got.states or []):
        if s is not None:
            f["%sstate%d" % (prefix, i)] = _sha(s)
    f.update({prefix + k: str(v) for k, v in got.sizes.items()})
    return f


def run_case(cid, check=False):
    """One run of a case -> {field: SHA-256 of a buffer, or a size as a decimal string}.  check: hold the result to the float64 bar of
    the test the case comes from (the recorder does; the bits test compares bytes, which is the stronger statement)."""
    from tests import test_encoder_layers_gpu as TL
    from tests import test_encoder_train_layers_gpu as TT
    family, args = CASES[cid]
    if family == "layer":
        c, regime = args
        case, want, bars = ec.prepared(*c)
        got = TL.abi_run(case, regime)
        if check:
            TL._check(case, want, bars, got, regime)
        return _layer_fields(got)
    if family == "chain":
        import torch
        name, norm, regime = args
        whole, states, push = ec.chain(name, norm)
        fields, outs = {}, []
        for k in range(len(ec.CHAIN_CHUNKS)):
            got = TL.abi_run(push(states, k), regime)
            fields.update(_layer_fields(got, "push%d/" % k))
            states = [s.cpu().numpy() for s in got.states]
            outs.append(got.out)
        if check:
            want = ec.oracle(whole)
            got.out, got.states = torch.cat(outs, dim=1), None
            TL._check(whole, want, ec.bar(whole, want), got, regime, label=cid)
        return fields
    name, kind, regime = args
    case, want, bars = C.prepared(name, kind)
    got = TT.abi_run(case, regime)
    if check:
        TT._compare(case, want, bars, got, cid)
    f = {"out": sha256_of_arrays(got.out), "saved": _sha(got.saved), "workspace_fwd": _sha(got.workspace_fwd),
         "workspace_bwd": _sha(got.workspace_bwd), "packed": _sha(got.packed)}
    for i, g in enumerate(got.grads):
        f.update({"grad%d/%s" % (i, k): sha256_of_arrays(a) for k, a in g.items() if a is not None})
    f.update({k: str(v) for k, v in got.sizes.items()})
    return f


def load():
    """{case id: {field: value}} of the recording."""
    with np.load(GOLDEN) as z:
        out = {}
        for key, val in zip(z["keys"].tolist(), z["values"].tolist()):
            cid, field = key.split("|")
            out.setdefault(cid, {})[field] = val
    return out


def main():
    import rnnt_amd
    rnnt_amd.engine.lib()
    print("recording from %s" % rnnt_amd.engine.LIB_PATH, flush=True)
    keys, values = [], []
    for cid in CASES:
        first, second = run_case(cid, check=True), run_case(cid)
        assert first == second, (cid, [k for k in first if first[k] != second.get(k)])
        for k in sorted(first):
            keys.append("%s|%s" % (cid, k))
            values.append(first[k])
        print("%-70s ok, %d fields" % (cid, len(first)), flush=True)
    np.savez_compressed(GOLDEN, keys=np.array(keys), values=np.array(values))
    print("%d cases -> %s (%d bytes)" % (len(CASES), GOLDEN, os.path.getsize(GOLDEN)), flush=True)


if __name__ == "__main__":
    main()
