"""CPU tests of the LSTM device decode's test premises and host-side wiring (tests/lstm_decode_cases.py): every case's float64
oracle keeps its margin and shows what the case is there for; the float64 module's decode is pinned to the REFERENCE's own modules'
token lists (tests/golden/decode_lstm_*.npz); RNNTModel reports the path a decode took and refuses the device loop off the device."""
import pytest
import torch

from tests import lstm_decode_cases as dc
from tests import lstm_predictor_cases as lc

CASES = [dc.WIRING_TEXT, dc.ALL_BLANK] + dc.WIDTHS + dc.CONTROL


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_case_premises(case):
    dc.checked_oracle(case)


def test_wiring_case_and_the_oracle_with_a_cap_per_frame():
    model, mel = lc.wiring_model(), lc.decode_frames()
    with torch.no_grad():
        want, gap = lc.greedy_with_margins(model, mel, 200)
    o = dc.greedy_oracle(model, mel, 200)
    assert o.tokens == want and o.gap == gap > dc.MARGIN and max(o.per_frame) <= 10
    capped = dc.greedy_oracle(model, mel, 200, max_per_frame=1)
    assert max(capped.per_frame) == 1 and capped.tokens != want
    state, text = dc.replay(model, o.tokens)  # the oracle's carried state is the predictor's state over the whole history
    assert lc.rel_err(o.state, state) < 1e-12 and lc.rel_err(o.text, text) < 1e-12


def test_batch_premises():
    oracles = dc.batch_oracles()
    assert len(oracles) == dc.MAX_UTT + 1 and oracles[1].per_frame in ([0], [len(oracles[1].tokens)])


def test_reference_width_premises():
    model = dc.build_model(dc.REF_CASE)
    for seed in dc.REF_FRAME_SEEDS:
        o = dc.greedy_oracle(model, dc.frames_of(dc.REF_CASE.H, dc.REF_CASE.T, seed), 200)
        assert o.gap > dc.MARGIN and len(set(o.tokens)) >= 8, (seed, o.gap)


@pytest.mark.parametrize("name", dc.GOLDENS)
def test_float64_decode_equals_the_reference_modules(name):
    fx = dc.load_golden(name)
    model, mel = dc.golden_model(fx)
    max_length = int(fx["max_length"])
    o = dc.greedy_oracle(model, mel, max_length)
    assert o.tokens == fx["tokens"].tolist()
    assert float(fx["gap"]) > dc.MARGIN and abs(o.gap - float(fx["gap"])) < 1e-9
    assert model.greedy_decode(mel, torch.tensor([mel.shape[-1]]), max_length=max_length) == o.tokens
    assert model.last_decode_path == "host"
    if name == "text_noln":
        assert len(o.tokens) == max_length - 1  # the cap binds


def test_host_side_of_the_wiring():
    """Off the device an LSTM model decodes on the host loop and says so; the device loop asked for by name is an error, not a fallback."""
    model, mel = lc.wiring_model(), lc.decode_frames()
    lens = torch.tensor([mel.shape[-1]])
    want = dc.greedy_oracle(model, mel, 200).tokens
    assert model.last_decode_path is None
    assert model.greedy_decode(mel, lens) == want and model.last_decode_path == "host"
    assert not model._device_loop_ok(mel.permute(0, 2, 1))
    with pytest.raises(RuntimeError, match="device_loop=True"):
        model.greedy_decode(mel, lens, device_loop=True)
    model.last_decode_path = None
    assert model.greedy_decode_many([mel, mel[:, :, :3]], batch=2) == [want, dc.greedy_oracle(model, mel[:, :, :3], 200).tokens]
    assert model.last_decode_path == "host"
    for batch in (0, 33):
        with pytest.raises(ValueError, match="batch"):
            model.greedy_decode_many([mel], batch=batch)
    assert model.greedy_decode_many([]) == []


def test_predictor_decode_bundle_reads_live_parameters():
    pred = lc.seeded_module(lc.DECODE_SPEC, torch.float32)
    params, (L, Hd, ln), eps = pred._decode_bundle()
    assert (L, Hd, ln) == (2, 32, True) and eps == (1e-5, 1e-3, 1e-5)
    assert all(a is b for a, b in zip(params, pred._params())) and not hasattr(pred, "_decode_cache")
    assert pred._decode_sizes() == (16, 16, 32, 32, 2, True)
