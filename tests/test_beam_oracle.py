"""CPU: the beam-search oracle (tests/beam_oracle.py) pinned by the reference's greedy token lists (beam 1) and by the transducer
likelihood (nothing pruned), and RNNTModel.beam_search's plain-torch host loop held to the oracle."""
import itertools

import numpy as np
import pytest
import torch

from oracle.brute_force import nll_bruteforce
from tests import beam_oracle
from tests.helpers import DECODE_CASES, decode_case_arrays, load_decode_case


@pytest.mark.parametrize("name", list(DECODE_CASES))
def test_beam1_oracle_is_the_reference_greedy_decode(golden_dir, name):
    c = load_decode_case(golden_dir, name)
    om = beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])
    for ml, want in c["tokens"].items():
        nbest, _, _ = beam_oracle.beam_search(om, 1, ml, 10)
        assert nbest[0][0] == want, (name, ml)


@pytest.mark.parametrize("V,T,ml,seed", [(3, 1, 4, 0), (3, 4, 4, 1), (4, 3, 3, 2), (4, 4, 2, 3), (3, 2, 3, 4)])
def test_unpruned_search_gives_the_transducer_likelihood(V, T, ml, seed):
    spec = dict(V=V, E=8, O=8, H=8, fa=-1, ft=-1, T=T, w_scale=1.0, store=False)
    frames, pred_sd, joint_sd = decode_case_arrays(spec, 300 + seed, 0.0)
    om = beam_oracle.Model(frames, pred_sd, joint_sd)
    nbest, pruned, _ = beam_oracle.beam_search(om, 1000, ml, max_per_frame=ml)
    assert pruned == 0
    seqs = [list(y) for n in range(ml) for y in itertools.product(range(V - 1), repeat=n)]
    assert sorted(y for y, _ in nbest) == sorted(seqs)
    for y, s in nbest:
        want = -nll_bruteforce(beam_oracle.lattice_logits(om, y), y, T, len(y), om.blank)
        assert abs(s - want) <= 1e-10, (y, s, want)


class TorchConvPredictor(torch.nn.Module):
    """The reference's ConvPredictor (rnnt/predictor.py:189-229, rnnt/causalconv.py) in plain torch, with its state-dict keys."""

    class _Causal(torch.nn.Module):
        def __init__(self, c, k):
            super().__init__()
            self.k = k
            self.conv = torch.nn.Conv1d(c, c, k)

        def forward(self, x):
            return self.conv(torch.nn.functional.pad(x, (self.k - 1, 0)))

    def __init__(self, V, O, E):
        super().__init__()
        self.embedding = torch.nn.Embedding(V, E)
        self.input_layer_norm = torch.nn.LayerNorm(E)
        self.conv1 = self._Causal(E, 3)
        self.conv2 = self._Causal(E, 5)
        self.linear = torch.nn.Linear(E, O)
        self.output_layer_norm = torch.nn.LayerNorm(O)

    def forward(self, ids):
        x = self.input_layer_norm(self.embedding(ids)).permute(0, 2, 1)
        x = torch.nn.functional.gelu(self.conv1(x))
        x = torch.nn.functional.gelu(self.conv2(x)).permute(0, 2, 1)
        return self.output_layer_norm(self.linear(x))


class PassThroughEncoder(torch.nn.Module):
    def forward(self, x):
        return x

    def calc_output_lens(self, lens):
        return lens


def _cpu_model(c):
    import rnnt_amd
    spec = c["spec"]
    pred = TorchConvPredictor(spec["V"], spec["O"], spec["E"])
    joint = rnnt_amd.JointNetwork(spec["fa"], spec["ft"], spec["H"], spec["V"])
    for mod, sd in ((pred, c["pred_sd"]), (joint, c["joint_sd"])):
        mod.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    return rnnt_amd.RNNTModel(pred, PassThroughEncoder(), joint).eval()


@pytest.mark.parametrize("name,ml", [("decode_small", 60), ("decode_small_proj", 60)])
def test_host_loop_matches_the_oracle(golden_dir, name, ml):
    c = load_decode_case(golden_dir, name)
    model = _cpu_model(c)
    om = beam_oracle.Model(c["frames"], c["pred_sd"], c["joint_sd"])
    mel = torch.from_numpy(np.ascontiguousarray(c["frames"].T))[None]
    lens = torch.tensor([mel.shape[-1]])
    assert model.beam_search(mel, lens, beam_size=1, max_length=ml) == c["tokens"][ml]
    for beam in (1, 4):
        want, _, gap = beam_oracle.beam_search(om, beam, ml)
        assert gap > 1e-3
        got = model.beam_search(mel, lens, beam_size=beam, max_length=ml, return_nbest=True)
        assert [g[0] for g in got] == [w[0] for w in want], (name, beam)
        for (_, gs), (_, ws) in zip(got, want):
            assert abs(gs - ws) <= 1e-4 * max(1.0, abs(ws)), (name, beam, gs, ws)


def test_host_loop_refuses_stateful_predictors_and_batches(golden_dir):
    import rnnt_amd

    class LSTMLike(torch.nn.Module):
        def forward(self, ids, lengths, state=None):
            raise AssertionError("never called")

    c = load_decode_case(golden_dir, "decode_small")
    model = _cpu_model(c)
    mel = torch.from_numpy(np.ascontiguousarray(c["frames"].T))[None]
    with pytest.raises(AssertionError):
        model.beam_search(torch.cat([mel, mel]), torch.tensor([75, 75]))
    with pytest.raises(ValueError):
        model.beam_search(mel, torch.tensor([75]), beam_size=0)
    stateful = rnnt_amd.RNNTModel(LSTMLike(), PassThroughEncoder(), model.joint)
    with pytest.raises(NotImplementedError):
        stateful.beam_search(mel, torch.tensor([75]))
