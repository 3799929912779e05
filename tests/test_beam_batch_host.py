"""CPU: RNNTModel.beam_search_many where the device path cannot be taken — the list of beam_search's results, in order."""
import numpy as np
import pytest
import torch

from tests.helpers import load_decode_case
from tests.test_beam_oracle import PassThroughEncoder, _cpu_model


def _mels(c):
    f = c["frames"]
    T = f.shape[0]
    return [torch.from_numpy(np.ascontiguousarray(x.T))[None] for x in (f[:12], f[T // 2:T // 2 + 3], f[T - 1:T], f[:12][::-1])]


@pytest.mark.parametrize("name", ["decode_small", "decode_small_proj"])
def test_cpu_model_gives_the_list_of_single_searches(golden_dir, name):
    c = load_decode_case(golden_dir, name)
    model = _cpu_model(c)
    mels = _mels(c)
    for kw in (dict(beam_size=4, max_length=20), dict(beam_size=2, max_length=9, max_symbols_per_frame=3)):
        want = [model.beam_search(m, torch.tensor([m.shape[-1]]), return_nbest=True, **kw) for m in mels]
        assert model.beam_search_many(mels, return_nbest=True, **kw) == want
        assert model.beam_search_many(mels, return_nbest=True, batch=3, **kw) == want
        assert model.beam_search_many(mels, **kw) == [w[0][0] for w in want]
    assert model.beam_search_many([]) == []
    assert model.beam_search_many(mels[:1], beam_size=20, max_length=9, return_nbest=True) == \
        [model.beam_search(mels[0], None, beam_size=20, max_length=9, return_nbest=True)]  # beam_size > 16: no device path anywhere


def test_refusals(golden_dir):
    import rnnt_amd

    class LSTMLike(torch.nn.Module):
        def forward(self, ids, lengths, state=None):
            raise AssertionError("never called")

    c = load_decode_case(golden_dir, "decode_small")
    model = _cpu_model(c)
    mels = _mels(c)
    stateful = rnnt_amd.RNNTModel(LSTMLike(), PassThroughEncoder(), model.joint)
    with pytest.raises(NotImplementedError):
        stateful.beam_search_many(mels)
    with pytest.raises(NotImplementedError):
        stateful.beam_search_many([])
    with pytest.raises(ValueError):
        model.beam_search_many(mels, beam_size=0)
    with pytest.raises(ValueError):
        model.beam_search_many(mels, batch=0)
    with pytest.raises(AssertionError):
        model.beam_search_many([torch.cat([mels[0], mels[0]])])
