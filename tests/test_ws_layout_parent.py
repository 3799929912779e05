"""Every workspace layout and size the engine reports equals what the library reported before the host sequencing of
rnnt_amd/csrc/engine.hip was split into one function per route (tests/golden/ws_layout_parent.json, written by
tests/golden/make_golden_ws_layout_parent.py, which also holds the cases): every field of rnnt_engine_workspace_layout and the
results of the four *_workspace_bytes entries, on the four dtypes.  No GPU needed."""
import importlib.util
import json
import os

import pytest

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_ws_layout_parent",
                                               os.path.join(_HERE, "golden", "make_golden_ws_layout_parent.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def golden():
    with open(G.GOLDEN) as f:
        return json.load(f)


def test_recording_covers_the_case_table(golden):
    assert sorted(golden) == sorted(G.key(c) for c in G.cases())
    assert len(golden) == 5 * 7 + 3 * 5 * 5


@pytest.mark.parametrize("case", G.cases(), ids=G.key)
def test_layout_and_sizes_equal_the_recording(golden, case):
    import rnnt_amd
    got, want = G.query(rnnt_amd.engine, case), golden[G.key(case)]
    assert got["layout"] == want["layout"], {k: (v, want["layout"][k]) for k, v in got["layout"].items() if v != want["layout"][k]}
    for entry in G.SIZES:
        assert got[entry] == want[entry], entry
