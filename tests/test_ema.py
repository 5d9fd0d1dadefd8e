"""``nequip_amd.train.EMAWeights`` on CPU tensors (the ATen form: host logic, state, swap) against the reference's recorded
``EMAWeights`` (``tests/golden/ref_ema.npz``) and the float64 restatement of ``tests/ema_restatement.py``."""
import copy
import os
import sys
import warnings

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ema_restatement as er  # noqa: E402

NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    return er.Fixture()


def _model(tensors):
    m = torch.nn.Module()
    m.p = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tensors])
    return m


def _set(tensors, values):
    with torch.no_grad():
        for t, v in zip(tensors, values):
            t.copy_(v)


def _before(k):
    """The recorded state before update ``k`` is the one after ``k - 1``."""
    return k - 1


def test_fixture_is_the_restatement_within_the_bound(fx):
    """The reference's own arithmetic, one recorded update at a time: pins the restatement and shows that the bound is not
    looser than the reference needs (worst error / bound is printed)."""
    from nequip_amd import _lib

    assert fx.chunk == _lib.load().nqa_ema_chunk_elems(), "rewrite the fixture: the chunk length of the library changed"
    worst = 0.0
    for decay, steps in er.CHECKED.items():
        for k in steps:
            params, after = fx.params(k), fx.ema(decay, k)
            before = fx.ema(decay, _before(k)) if k > 1 else [torch.full_like(p, NAN) for p in params]
            for i, (a, b, p) in enumerate(zip(after, before, params)):
                worst = max(worst, er.assert_update(a, b, p, k - 1, decay, f"decay {decay} update {k} tensor {i}"))
    print(f"worst error / bound of the reference: {worst:.3f}")
    assert 0.0 < worst <= 1.0


@pytest.mark.parametrize("decay", [0.5, 0.999])
def test_aten_form_step_by_step(fx, decay):
    from nequip_amd.train import EMAWeights

    model = _model(fx.params(1))
    ema = EMAWeights(model, decay)
    assert ema.num_ema_weights == 14 and [b.dtype for b in ema.ema_weights] == [torch.float32] * 7 + [torch.float64] * 7
    for b in ema.ema_weights:
        b.fill_(NAN)
    for k in er.CHECKED[decay]:
        params = fx.params(k)
        _set(model.parameters(), params)
        if k > 1:
            _set(ema.ema_weights, fx.ema(decay, _before(k)))
            ema.num_updates = k - 1
        before = [b.clone() for b in ema.ema_weights]
        ema.update_parameters(model)
        assert ema.num_updates == k
        for i, (a, b, p) in enumerate(zip(ema.ema_weights, before, params)):
            er.assert_update(a, b, p, k - 1, decay, f"update {k} tensor {i}")


def test_decay_sequence_switches_at_eight():
    """``decay=0.5``: (1 + n) / (10 + n) reaches 0.5 at n = 8.  A scalar EMA towards 1 from 0 shows the weight of every step."""
    from nequip_amd.train import EMAWeights

    model = _model([torch.zeros(1, dtype=torch.float64)])
    ema = EMAWeights(model, 0.5)
    ema.update_parameters(model)
    weights = []
    for n in range(1, 12):
        _set(ema.ema_weights, [torch.zeros(1, dtype=torch.float64)])
        _set(model.parameters(), [torch.ones(1, dtype=torch.float64)])
        ema.update_parameters(model)
        weights.append(float(ema.ema_weight_0))
    want = [1.0 - (1 + n) / (10 + n) for n in range(1, 8)] + [0.5] * 4
    assert weights == pytest.approx(want, abs=1e-15) and weights[6] > 0.5 and weights[7] == 0.5


def test_state_dict_matches_the_reference_and_round_trips(fx):
    from nequip_amd.train import EMAWeights

    model = _model(fx.params(1))
    ema = EMAWeights(model, 0.5)
    for k in range(1, er.N_STEPS + 1):
        _set(model.parameters(), fx.params(k))
        ema.update_parameters(model)
    assert list(ema.state_dict().keys()) == fx.state_keys
    assert ema.get_extra_state() == fx.extra_state and isinstance(ema.get_extra_state()["num_updates"], int)

    fresh = EMAWeights(_model(fx.params(1)), 0.5)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fresh.load_state_dict(copy.deepcopy(ema.state_dict()))
    assert fresh.num_updates == 12 and fresh.is_holding_ema_weights
    _set(model.parameters(), fx.params(1))
    ema.update_parameters(model)
    fresh.update_parameters(model)
    assert fresh.num_updates == 13
    for a, b in zip(fresh.ema_weights, ema.ema_weights):
        assert torch.equal(a, b)

    # a state written by the reference: its keys, its extra state, its buffers
    ref_state = {f"ema_weight_{i}": t for i, t in enumerate(fx.ema(0.5, 12))}
    ref_state["_extra_state"] = dict(fx.extra_state)
    loaded = EMAWeights(_model(fx.params(1)), 0.5)
    loaded.load_state_dict(ref_state)
    assert loaded.num_updates == 12 and torch.equal(loaded.ema_weight_13, fx.ema(0.5, 12)[13])


def test_loading_another_decay_warns_and_keeps_the_constructor_value(fx):
    from nequip_amd.train import EMAWeights

    model = _model([torch.zeros(3)])
    ema = EMAWeights(model, 0.5)
    ema.update_parameters(model)
    ema.update_parameters(model)
    other = EMAWeights(model, 0.25)
    with pytest.warns(UserWarning, match=r"loaded from state dict \(0.5\) is different .* set \(0.25\)"):
        other.load_state_dict(ema.state_dict())
    assert other.decay == 0.25 and other.num_updates == 2
    _set(other.ema_weights, [torch.zeros(3)])
    _set(model.parameters(), [torch.ones(3)])
    other.update_parameters(model)  # n = 2: min(0.25, 3 / 12) = 0.25 either way; n = 3 tells them apart
    _set(other.ema_weights, [torch.zeros(3)])
    other.update_parameters(model)  # n = 3: min(0.25, 4 / 13) = 0.25, with 0.5 it would be 4 / 13
    assert float(other.ema_weight_0[0]) == 0.75

    state = ema.state_dict()
    state["_extra_state"] = dict(state["_extra_state"], is_holding_ema_weights=False)
    with pytest.raises(AssertionError, match="does not contain EMA weights"):
        EMAWeights(model, 0.5).load_state_dict(state)


def test_swap(fx):
    from nequip_amd.train import EMAWeights

    model = _model(fx.params(1))
    ema = EMAWeights(model, 0.5)
    ema.update_parameters(model)
    _set(model.parameters(), fx.params(2))
    ema.update_parameters(model)
    p0, e0 = [p.detach().clone() for p in model.parameters()], [b.clone() for b in ema.ema_weights]
    versions = [t._version for t in list(model.parameters()) + ema.ema_weights]

    ema.swap_parameters(model)
    assert not ema.is_holding_ema_weights
    for p, b, pw, ew in zip(model.parameters(), ema.ema_weights, p0, e0):
        assert torch.equal(p, ew) and torch.equal(b, pw)
    assert all(t._version > v for t, v in zip(list(model.parameters()) + ema.ema_weights, versions))
    with pytest.raises(AssertionError, match="not holding EMA weights"):
        ema.update_parameters(model)
    ema.swap_parameters(model)
    assert ema.is_holding_ema_weights
    for p, b, pw, ew in zip(model.parameters(), ema.ema_weights, p0, e0):  # two swaps: the identity, bit for bit
        assert torch.equal(er.bits(p), er.bits(pw)) and torch.equal(er.bits(b), er.bits(ew))

    with pytest.raises(KeyError, match="inside"):
        with ema.average_parameters(model) as m:
            assert m is model and not ema.is_holding_ema_weights and torch.equal(model.p[3], e0[3])
            raise KeyError("inside")
    assert ema.is_holding_ema_weights
    for p, b, pw, ew in zip(model.parameters(), ema.ema_weights, p0, e0):
        assert torch.equal(p, pw) and torch.equal(b, ew)


def test_constructor_forward_and_integer_parameters():
    from nequip_amd.train import EMAWeights

    lin = torch.nn.Linear(2, 2)
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError, match=r"Invalid decay value .* in \[0,1\] range"):
            EMAWeights(lin, bad)
    ema = EMAWeights(lin, 1.0)
    with pytest.raises(RuntimeError, match="only carries EMA weights"):
        ema(torch.zeros(2))
    assert EMAWeights(torch.nn.Module(), 0.5).ema_weights == []
    with pytest.raises(ValueError, match="parameters"):
        ema.update_parameters(torch.nn.Linear(2, 2, bias=False))

    # integer parameters: e * d + p * (1 - d) element-wise, written back into the integer buffer (the reference's arithmetic)
    model = torch.nn.Module()
    model.i = torch.nn.Parameter(torch.tensor([10, 20, -30]), requires_grad=False)
    model.f = torch.nn.Parameter(torch.tensor([1.0, 2.0]))
    ema = EMAWeights(model, 0.5)
    ema.update_parameters(model)
    assert ema.ema_weight_0.dtype == torch.int64 and torch.equal(ema.ema_weight_0, model.i)
    _set(model.parameters(), [torch.tensor([20, 40, -60]), torch.tensor([2.0, 4.0])])
    ema.update_parameters(model)  # n = 1: d = 2 / 11
    d = 2 / 11
    want = (torch.tensor([10, 20, -30]) * d + torch.tensor([20, 40, -60]) * (1 - d)).to(torch.int64)
    assert torch.equal(ema.ema_weight_0, want) and ema.num_updates == 2
    torch.testing.assert_close(ema.ema_weight_1, torch.tensor([1.0, 2.0]) * d + torch.tensor([2.0, 4.0]) * (1 - d))
    ema.swap_parameters(model)
    assert torch.equal(model.i, want)
