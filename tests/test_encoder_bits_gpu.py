"""The encoder's entries keep EVERY BIT they left before the inference and the training halves of rnnt_amd/csrc/encoder.hip were put on
one epilogue body (k_enc_norm<TRAIN>), one conv launch and one pack kernel: `out`, new streaming states, the calls' whole workspaces,
`saved`, every gradient and the packed tables as SHA-256, the size queries' answers as numbers, against tests/golden/encoder_bits.npz,
written by tests/golden/make_golden_encoder_bits.py from the build before that change.  That module also holds the cases (those of the
layer tests, no shapes of its own) and the code that runs them.  Every path is a fixed kernel sequence with fixed summation orders, so
the bar is equality, and every case is run twice."""
import importlib.util
import os

import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_encoder_bits", os.path.join(_HERE, "golden", "make_golden_encoder_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def golden():
    return G.load()


def test_recording_covers_exactly_the_case_lists(golden):
    from tests import encoder_layer_cases as ec
    from tests import encoder_train_cases as C
    assert set(golden) == set(G.CASES)
    fams = [f for f, _ in G.CASES.values()]
    assert fams.count("layer") == sum(len(ec.SHAPES[c[0]][4]) for c in ec.case_ids(layouts_too=True))
    assert fams.count("chain") == len(ec.CHAIN_CASES) * len(G.CHAIN_NORMS) * 2
    assert fams.count("train") == len(C.case_ids()) * 2


@pytest.mark.gpu
@pytest.mark.parametrize("cid", list(G.CASES))
def test_case_keeps_every_bit(golden, cid):
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    want = golden[cid]
    for run in range(2):
        got = G.run_case(cid)
        assert sorted(got) == sorted(want)
        diff = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
        assert not diff, "%s, run %d: differs from the recorded bytes: %s" % (cid, run, diff)
