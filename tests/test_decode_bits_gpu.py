"""The decoders keep EVERY BIT they left before their shared device pieces — scan tile, candidate argmax, advance rule, block sum,
row LayerNorm — moved into rnnt_amd/csrc/decode_kernels.hpp: tokens, state words and scores raw, float buffers and the calls' whole
workspaces as SHA-256, against tests/golden/decode_bits.npz, written by tests/golden/make_golden_decode_bits.py, which also holds the
cases, what each one reaches and the code that runs them.  Every path is a fixed kernel sequence with fixed summation orders, so the
bar is equality."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
_spec = importlib.util.spec_from_file_location("make_golden_decode_bits", os.path.join(_HERE, "golden", "make_golden_decode_bits.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def engine():
    import rnnt_amd
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    rnnt_amd.engine.lib()
    return rnnt_amd.engine


@pytest.fixture(scope="module")
def golden():
    return np.load(G.GOLDEN)


def test_recording_covers_the_cases(golden):
    assert {k.rsplit("/", 1)[0] for k in golden.files} == set(G.CASES) == set(G.REACHES)


@pytest.mark.parametrize("name", list(G.CASES))
def test_case_reaches_its_branches(name):
    """Host code only: the sizes each case relies on (H / 8, V % 32, T against scan_frames, ...)."""
    G.check_reach(name)


def test_state_words_mirror_the_header():
    """engine.DECODE_* are include/rnnt_engine.h's RNNT_DECODE_* (as STREAM_* mirror RNNT_STREAM_*)."""
    from rnnt_amd import engine
    with open(os.path.join(os.path.dirname(_HERE), "include", "rnnt_engine.h")) as f:
        words = dict(re.findall(r"#define RNNT_DECODE_(\w+) (\d+)", f.read()))
    assert len(words) == 10
    for k, v in words.items():
        assert getattr(engine, "DECODE_" + k) == int(v), k
    assert engine.DECODE_LABELS == engine.DECODE_STATE_WORDS + 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(G.CASES))
def test_case_keeps_every_bit(engine, golden, name):
    got = G.run_checked(engine, name)
    assert sorted(got) == sorted(k.rsplit("/", 1)[1] for k in golden.files if k.rsplit("/", 1)[0] == name)
    for k, a in got.items():
        want = golden["%s/%s" % (name, k)]
        assert a.dtype == want.dtype and a.shape == want.shape, k
        assert np.array_equal(a, want), "%s differs from the recorded bytes: %s != %s" % (k, a, want)
