"""``MetricsManager`` and the metric classes on CPU tensors: parsing / validation, naming, coefficients, and the ATen form of
the fused reduction (``nequip_amd/train/_metrics_ops.py::_aten_forward``) against ``tests/metrics_restatement.py``.

The reference (nequip/train/metrics_manager.py) cannot be imported here -- it needs ``torchmetrics``, which is not
installed -- so there are no reference-generated fixtures for this feature: every comparison is against the plain-torch
float64 restatement of its semantics (loops over types, boolean indexing).

Tolerance: rtol 1e-10 on values and on gradients (autograd through the restatement).  Both sides are float64 sums of fewer
than 1e5 terms in a different order, which differ by at most about n * 2^-53 ~ 1e-11 relative.
"""
import copy
import math

import pytest
import torch

import metrics_restatement as mr
from nequip_amd.data import MappedFieldModifier, PerAtomModifier
from nequip_amd.train import (EnergyForceLoss, EnergyForceMetrics, EnergyForceStressLoss, EnergyForceStressMetrics,
                              EnergyOnlyLoss, EnergyOnlyMetrics, HuberLoss, MaximumAbsoluteError, MeanAbsoluteError,
                              MeanSquaredError, MetricsManager, RootMeanSquaredError, StratifiedHuberForceLoss)

RTOL = 1e-10
TYPES = ["H", "O", "Cs"]
METRIC = {"mse": MeanSquaredError, "mae": MeanAbsoluteError, "rmse": RootMeanSquaredError, "max_ae": MaximumAbsoluteError}


def close(got, ref, what=""):
    got, ref = torch.as_tensor(got, dtype=torch.float64).detach().cpu(), torch.as_tensor(ref, dtype=torch.float64).detach()
    torch.testing.assert_close(got, ref, rtol=RTOL, atol=0.0, equal_nan=True, msg=lambda m: f"{what}: {m}")


def batch(sizes, seed=0, absent_type=2):
    """Frames of the given sizes, float32 predictions and float64 targets; atom types 0..2 without ``absent_type``."""
    g = torch.Generator().manual_seed(seed)
    n, b = sum(sizes), len(sizes)
    types = torch.randint(0, 3, (n,), generator=g)
    if absent_type is not None:
        types[types == absent_type] = 0
    preds = {"total_energy": torch.randn(b, 1, generator=g), "forces": torch.randn(n, 3, generator=g),
             "stress": torch.randn(b, 3, 3, generator=g), "num_atoms": torch.tensor(sizes), "atom_types": types}
    target = {"total_energy": torch.randn(b, 1, generator=g, dtype=torch.float64),
              "forces": 2.0 * torch.randn(n, 3, generator=g, dtype=torch.float64),
              "stress": torch.randn(b, 3, 3, generator=g, dtype=torch.float64), "num_atoms": torch.tensor(sizes)}
    return preds, target


def with_grad(preds):
    return {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in preds.items()}


def check_against_restatement(manager, entries, preds, target, grad_of="weighted_sum"):
    """Every name and value of the batch, and the gradient of ``grad_of`` w.r.t. every prediction: once with the predictions
    as given (float32: the gradient is rounded to float32, hence 1e-6 there) and once with float64 predictions, where the
    gradient is held to the same 1e-10 as the values.  Returns the values of the first run."""
    first = None
    for dtype in (None, torch.float64):
        cast = {k: (v.to(dtype) if dtype is not None and v.is_floating_point() else v) for k, v in preds.items()}
        p1, p2 = with_grad(cast), with_grad(cast)
        got, ref = manager(p1, target), mr.evaluate(entries, [(p2, target)], TYPES)
        assert list(got) == list(ref)
        for k in ref:
            close(got[k], ref[k], k)
        if grad_of is not None:
            keys = [k for k, v in p1.items() if v.requires_grad]
            g1 = torch.autograd.grad(got[grad_of], [p1[k] for k in keys], allow_unused=True)
            g2 = torch.autograd.grad(ref[grad_of], [p2[k] for k in keys], allow_unused=True)
            for k, a, b in zip(keys, g1, g2):
                if b is None:
                    assert a is None or not a.any(), k
                else:
                    assert a.dtype == cast[k].dtype
                    torch.testing.assert_close(a.double(), b.double(), rtol=1e-6 if a.dtype == torch.float32 else RTOL,
                                               atol=0.0, msg=lambda m: f"grad {k} ({a.dtype}): {m}")
        first = got if first is None else first
    return first


# ---- parsing and validation ---------------------------------------------------------------------------------------------------
def test_refusals():
    mse = MeanSquaredError
    with pytest.raises(AssertionError, match="unrecognized key"):
        MetricsManager([{"field": "forces", "metric": mse(), "weight": 1.0}])
    with pytest.raises(AssertionError, match="must contain a `metric` key"):
        MetricsManager([{"field": "forces"}])
    with pytest.raises(AssertionError, match="reserved"):
        MetricsManager([{"field": "forces", "metric": mse(), "name": "weighted_sum"}])
    with pytest.raises(AssertionError, match="Repeated names"):
        MetricsManager([{"field": "forces", "metric": mse()}, {"field": "forces", "metric": mse()}])
    with pytest.raises(AssertionError, match="type_names"):
        MetricsManager([{"field": "forces", "metric": mse(), "per_type": True}])
    with pytest.raises(RuntimeError, match="only supported for node fields"):
        MetricsManager([{"field": "total_energy", "metric": mse(), "per_type": True}], type_names=TYPES)
    with pytest.raises(AssertionError, match="ignore_nan` should be a bool"):
        MetricsManager([{"field": "forces", "metric": mse(), "ignore_nan": 1}])
    for key in ("per_type", "ignore_nan"):
        with pytest.raises(AssertionError, match="should not be provided"):
            MetricsManager([{"metric": torch.nn.Identity(), key: False}], type_names=TYPES)
    pt = {"field": "forces", "metric": mse(), "per_type": True}
    with pytest.raises(ValueError, match="require `per_type: true`"):
        MetricsManager([{"field": "forces", "metric": mse(), "per_type_coeffs": {"H": 1.0, "O": 1.0, "Cs": 1.0}}], type_names=TYPES)
    with pytest.raises(TypeError, match="must be a dict"):
        MetricsManager([dict(pt, per_type_coeffs=[1.0, 1.0, 1.0])], type_names=TYPES)
    with pytest.raises(ValueError, match="missing"):
        MetricsManager([dict(pt, per_type_coeffs={"H": 1.0, "O": 1.0})], type_names=TYPES)
    with pytest.raises(ValueError, match="not in `type_names`"):
        MetricsManager([dict(pt, per_type_coeffs={"H": 1.0, "O": 1.0, "Cs": 1.0, "Xe": 1.0})], type_names=TYPES)
    for bad in (0.0, -1.0):
        with pytest.raises(ValueError, match="must be positive"):
            MetricsManager([dict(pt, per_type_coeffs={"H": 1.0, "O": bad, "Cs": 1.0})], type_names=TYPES)
    with pytest.raises(AssertionError, match="At least two delta values"):
        StratifiedHuberForceLoss({0.0: 1.0})
    with pytest.raises(AssertionError):
        HuberLoss(reduction="median")
    with pytest.raises(ValueError, match="at most 16"):
        MetricsManager([pt], type_names=[f"T{i}" for i in range(17)])
    with pytest.raises(ValueError, match="at most 32"):
        MetricsManager([{"field": "forces", "metric": mse(), "name": f"m{i}"} for i in range(33)])
    with pytest.raises(KeyError, match="Unregistered field"):
        MetricsManager([dict(pt, field="not_a_field")], type_names=TYPES)
    with pytest.raises(ValueError, match="at most 8"):  # nine distinct prediction/target pairs
        MetricsManager([{"field": PerAtomModifier("total_energy", factor=float(i + 2)), "metric": mse(), "name": f"m{i}"}
                        for i in range(9)])
    with pytest.raises(ValueError, match="takes 2 to 8"):  # nine strata
        MetricsManager([{"field": "forces", "metric": StratifiedHuberForceLoss({float(i): 1.0 / (i + 1) for i in range(9)})}])
    MetricsManager([{"field": "forces", "metric": StratifiedHuberForceLoss({float(i): 1.0 / (i + 1) for i in range(8)})}])


def test_automatic_names():
    m = MetricsManager([
        {"field": "total_energy", "metric": MeanSquaredError()},
        {"field": PerAtomModifier("total_energy"), "metric": MeanAbsoluteError()},
        {"field": "forces", "metric": RootMeanSquaredError()},
        {"field": "forces", "metric": MaximumAbsoluteError()},
        {"field": "stress", "metric": HuberLoss(delta=0.5)},
        {"field": "forces", "metric": StratifiedHuberForceLoss({1.0: 0.1, 2.0: 0.05})},
        {"field": MappedFieldModifier("forces", "forces"), "metric": MeanSquaredError()},
        {"metric": torch.nn.Identity()},
    ])
    assert list(m.entries) == ["E_mse", "per_atom_E_mae", "F_rmse", "F_max_ae", "stress_huber", "F_stratified huber",
                               "pred_F_label_F_mse", "Identity()"]


def test_coefficients_and_extra_state():
    def build():
        return MetricsManager([{"field": "total_energy", "metric": MeanSquaredError(), "coeff": 3.0, "name": "e"},
                               {"field": "forces", "metric": MeanSquaredError(), "coeff": 1.0, "name": "f"},
                               {"field": "stress", "metric": MeanAbsoluteError(), "name": "s"}])

    m = build()
    assert {k: e.coeff for k, e in m.entries.items()} == {"e": 0.75, "f": 0.25, "s": None} and m.do_weighted_sum
    preds, target = batch([2, 3])
    out = m(preds, target)
    assert list(out) == ["e", "f", "s", "weighted_sum"]
    close(out["weighted_sum"], 0.75 * out["e"] + 0.25 * out["f"])
    m.set_coeffs({"s": 2.0})  # missing keys: None
    assert {k: e.coeff for k, e in m.entries.items()} == {"e": None, "f": None, "s": 1.0}
    close(m(preds, target)["weighted_sum"], out["s"])
    m.set_coeffs({})
    assert not m.do_weighted_sum and "weighted_sum" not in m(preds, target)

    m = build()
    assert m.metrics_values_step == {"e": None, "f": None, "s": None}
    out = m(preds, target)
    m.compute()
    state = copy.deepcopy(m.state_dict())
    extra = state["_extra_state"]
    assert extra["coeff_dict"] == {"e": 0.75, "f": 0.25, "s": None}
    assert extra["metrics_values_step"] == {k: float(out[k]) for k in "efs"} == extra["metrics_values_epoch"]
    m2 = MetricsManager([{"field": "total_energy", "metric": MeanSquaredError(), "name": "e"},
                         {"field": "forces", "metric": MeanSquaredError(), "name": "f", "coeff": 1.0},
                         {"field": "stress", "metric": MeanAbsoluteError(), "name": "s"}])
    m2.load_state_dict(state)
    assert {k: e.coeff for k, e in m2.entries.items()} == {"e": 0.75, "f": 0.25, "s": None}
    assert dict(m2.metrics_values_step) == extra["metrics_values_step"]


def test_builder_term_names():
    assert list(EnergyForceLoss().entries) == ["per_atom_energy_mse", "forces_mse"]
    assert list(EnergyForceLoss(per_atom_energy=False).entries) == ["total_energy_mse", "forces_mse"]
    assert list(EnergyForceStressLoss().entries) == ["per_atom_energy_mse", "forces_mse", "stress_mse"]
    assert list(EnergyOnlyLoss().entries) == ["per_atom_energy_mse"]
    assert {k: e.coeff for k, e in EnergyForceStressLoss().entries.items()} == dict.fromkeys(
        ["per_atom_energy_mse", "forces_mse", "stress_mse"], 1.0 / 3.0)
    eo = ["total_energy_rmse", "total_energy_mae", "per_atom_energy_rmse", "per_atom_energy_mae"]
    assert list(EnergyOnlyMetrics().entries) == eo + ["total_energy_maxabserr", "per_atom_energy_maxabserr"]
    ef = eo + ["forces_rmse", "forces_mae"]
    assert list(EnergyForceMetrics().entries) == ef + ["total_energy_maxabserr", "per_atom_energy_maxabserr", "forces_maxabserr"]
    efs = EnergyForceStressMetrics(ignore_nan={"stress": True})
    assert list(efs.entries) == ef + ["stress_rmse", "stress_mae", "total_energy_maxabserr", "per_atom_energy_maxabserr",
                                      "forces_maxabserr", "stress_maxabserr"]
    assert [k for k, e in efs.entries.items() if e.ignore_nan] == ["stress_rmse", "stress_mae", "stress_maxabserr"]
    assert {k for k, e in efs.entries.items() if e.coeff} == {"total_energy_rmse", "forces_rmse", "stress_rmse"}
    with pytest.raises(AssertionError, match="Unrecognized key"):
        EnergyForceMetrics(coeffs={"stress_rmse": 1.0})
    loss = EnergyForceLoss(per_type_forces_coeffs={"H": 5.0, "O": 1.0, "Cs": 0.5}, type_names=TYPES)
    assert loss.entries["forces_mse"].per_type and loss.entries["forces_mse"].per_type_coeffs == [5.0, 1.0, 0.5]


# ---- the ATen form against the restatement ------------------------------------------------------------------------------------
KINDS = [("mse", {}), ("mae", {}), ("rmse", {}), ("max_ae", {}), ("huber", {"delta": 0.7}),
         ("huber", {"delta": 0.7, "reduction": "sum"}), ("stratified huber", {"delta_dict": {1.0: 0.5, 3.0: 0.2}}),
         ("stratified huber", {"delta_dict": {0.0: 1.0, 2.0: 0.3, 4.0: 0.1}, "reduction": "sum"})]


def make_metric(kind, kw):
    if kind == "huber":
        return HuberLoss(**kw)
    if kind == "stratified huber":
        return StratifiedHuberForceLoss(**kw)
    return METRIC[kind]()


@pytest.mark.parametrize("kind,kw", KINDS, ids=[f"{k}-{i}" for i, (k, _) in enumerate(KINDS)])
@pytest.mark.parametrize("per_type", [None, "equal", "coeffs"])
def test_every_kind_against_the_restatement(kind, kw, per_type):
    """Forces of three frames with the last type absent: plain, per type, per type with coefficients; each term also as the
    loss (coefficient 1) so that its gradient is checked -- max-abs is a metric and gets none."""
    preds, target = batch([5, 64, 30])
    e = {"name": "m", "field": "forces", "kind": kind, "coeff": None if kind == "max_ae" else 1.0, **kw}
    d = {"name": "m", "field": "forces", "metric": make_metric(kind, kw), "coeff": e["coeff"]}
    if per_type:
        e["per_type"] = d["per_type"] = True
        if per_type == "coeffs":
            e["per_type_coeffs"], d["per_type_coeffs"] = [5.0, 1.0, 0.5], {"H": 5.0, "O": 1.0, "Cs": 0.5}
    m = MetricsManager([d], type_names=TYPES)
    got = check_against_restatement(m, [e], preds, target, grad_of=None if kind == "max_ae" else "weighted_sum")
    if per_type:
        absent = got["m_Cs"]
        assert (absent == -math.inf) if kind == "max_ae" else (absent == 0 if kw.get("reduction") == "sum" else torch.isnan(absent))
    if kind == "max_ae":
        assert not got["m"].requires_grad


def test_ignore_nan_some_and_all():
    preds, target = batch([4, 6, 5])
    target["stress"][1] = math.nan  # a frame without stress labels
    target["forces"][::4, 1] = math.nan
    entries = [{"name": "e", "field": "total_energy", "kind": "mse", "per_atom": True, "coeff": 1.0},
               {"name": "f", "field": "forces", "kind": "mse", "coeff": 1.0, "ignore_nan": True, "per_type": True},
               {"name": "s", "field": "stress", "kind": "rmse", "coeff": 1.0, "ignore_nan": True},
               {"name": "smax", "field": "stress", "kind": "max_ae", "ignore_nan": True}]
    dicts = [{"name": "e", "field": PerAtomModifier("total_energy"), "metric": MeanSquaredError(), "coeff": 1.0},
             {"name": "f", "field": "forces", "metric": MeanSquaredError(), "coeff": 1.0, "ignore_nan": True, "per_type": True},
             {"name": "s", "field": "stress", "metric": RootMeanSquaredError(), "coeff": 1.0, "ignore_nan": True},
             {"name": "smax", "field": "stress", "metric": MaximumAbsoluteError(), "ignore_nan": True}]
    m = MetricsManager(dicts, type_names=TYPES)
    got = check_against_restatement(m, entries, preds, target)
    assert torch.isfinite(got["weighted_sum"])
    p = with_grad(preds)
    m(p, target)["weighted_sum"].backward()
    assert (p["stress"].grad[1] == 0).all() and (p["forces"].grad[::4, 1] == 0).all()  # masked: exactly zero
    assert p["stress"].grad[0].abs().min() > 0

    target["stress"][:] = math.nan  # every target NaN: the term and weighted_sum are NaN, its gradient is zero
    p = with_grad(preds)
    got = m(p, target)
    assert torch.isnan(got["s"]) and torch.isnan(got["weighted_sum"]) and got["smax"] == -math.inf
    got["weighted_sum"].backward()
    assert (p["stress"].grad == 0).all()
    assert torch.isfinite(p["forces"].grad).all() and torch.isfinite(p["total_energy"].grad).all()
    assert p["forces"].grad.abs().max() > 0


def test_per_atom_modifier_with_frames_of_different_sizes():
    preds, target = batch([3, 17, 8])
    entries = [{"name": "a", "field": "total_energy", "kind": "mse", "per_atom": True, "coeff": 1.0},
               {"name": "b", "field": "total_energy", "kind": "mae", "per_atom": True, "factor": 1000.0, "coeff": 2.0},
               {"name": "c", "field": "total_energy", "kind": "rmse", "coeff": 1.0}]
    m = MetricsManager([{"name": "a", "field": PerAtomModifier("total_energy"), "metric": MeanSquaredError(), "coeff": 1.0},
                        {"name": "b", "field": PerAtomModifier("total_energy", factor=1000.0), "metric": MeanAbsoluteError(),
                         "coeff": 2.0},
                        {"name": "c", "field": "total_energy", "metric": RootMeanSquaredError(), "coeff": 1.0}])
    check_against_restatement(m, entries, preds, target)
    assert m.__dict__["_plan"].n_streams == 3
    # the modifier on its own (data statistics) does what the stream's row scale does; as in the reference its reciprocal of
    # the integer atom counts is float32, hence the float32 bound
    x = PerAtomModifier("total_energy", factor=2.0)(target)
    ref = 2.0 * target["total_energy"] / torch.tensor([[3.0], [17.0], [8.0]], dtype=torch.float64)
    torch.testing.assert_close(x, ref, rtol=2e-7, atol=0.0)


def test_huber_exactly_at_delta_and_strata_exactly_on_a_bound():
    # |x| == delta is the LINEAR branch (strict <): value delta^2 / 2 either way, but the derivative is delta * sign(x)
    t = torch.zeros(4, 1, dtype=torch.float64)
    p = torch.tensor([[0.5], [-0.5], [0.25], [2.0]], dtype=torch.float64, requires_grad=True)
    h = HuberLoss(delta=0.5, reduction="sum")
    v = h(p, t)
    close(v, 0.125 + 0.125 + 0.03125 + 0.5 * (2.0 - 0.25))
    (g,) = torch.autograd.grad(v, p)
    assert g.flatten().tolist() == [0.5, -0.5, 0.25, 0.5]
    # target rows of norm exactly 5 (3-4-0) sit in the stratum that STARTS at 5; first bound above 0: implicit {0: inf}
    target = torch.tensor([[3.0, 4.0, 0.0], [0.3, 0.4, 0.0], [6.0, 8.0, 0.0], [2.9999, 4.0, 0.0]], dtype=torch.float64)
    pred = (target + torch.tensor([[2.0, -0.05, 0.3]], dtype=torch.float64)).float()
    dd = {5.0: 0.1, 10.0: 1.0}
    e = [{"name": "m", "field": "forces", "kind": "stratified huber", "delta_dict": dd, "coeff": 1.0}]
    m = MetricsManager([{"name": "m", "field": "forces", "metric": StratifiedHuberForceLoss(dd), "coeff": 1.0}])
    assert m["m"].delta_dict == {0: math.inf, 5.0: 0.1, 10.0: 1.0}
    got = check_against_restatement(m, e, {"forces": pred}, {"forces": target})
    d = pred.double() - target
    rows = [mr.element_loss("huber", d[0], None, delta=0.1), 0.5 * d[1] ** 2, mr.element_loss("huber", d[2], None, delta=1.0),
            0.5 * d[3] ** 2]
    close(got["m"], torch.stack(rows).mean())


def test_two_batches_compute_and_reset():
    entries = [{"name": "e", "field": "total_energy", "kind": "rmse", "per_atom": True, "coeff": 1.0},
               {"name": "f", "field": "forces", "kind": "mae", "per_type": True, "per_type_coeffs": [1.0, 2.0, 3.0], "coeff": 1.0},
               {"name": "fmax", "field": "forces", "kind": "max_ae", "per_type": True},
               {"name": "h", "field": "forces", "kind": "huber", "delta": 0.3, "reduction": "sum"},
               {"name": "s", "field": "stress", "kind": "mse", "ignore_nan": True}]
    m = MetricsManager([
        {"name": "e", "field": PerAtomModifier("total_energy"), "metric": RootMeanSquaredError(), "coeff": 1.0},
        {"name": "f", "field": "forces", "metric": MeanAbsoluteError(), "per_type": True,
         "per_type_coeffs": {"H": 1.0, "O": 2.0, "Cs": 3.0}, "coeff": 1.0},
        {"name": "fmax", "field": "forces", "metric": MaximumAbsoluteError(), "per_type": True},
        {"name": "h", "field": "forces", "metric": HuberLoss(delta=0.3, reduction="sum")},
        {"name": "s", "field": "stress", "metric": MeanSquaredError(), "ignore_nan": True}], type_names=TYPES)
    b1, b2 = batch([5, 9], seed=1, absent_type=2), batch([7, 4, 11], seed=2, absent_type=None)
    b2[1]["stress"][0] = math.nan
    for b in (b1, b2):
        m(*b)
    got, ref = m.compute(prefix="val_", suffix="_x"), mr.evaluate(entries, [b1, b2], TYPES, epoch=True)
    assert list(got) == [f"val_{k}_x" for k in ref]
    for k in ref:
        close(got[f"val_{k}_x"], ref[k], k)
    assert list(m.metrics_values_epoch) == ["e", "f", "fmax", "h", "s"]
    for k, v in m.metrics_values_epoch.items():
        close(v, ref[k], k)
    # only the first batch: the absent type is NaN and, per EPOCH, makes the aggregate NaN
    m.reset()
    m(*b1)
    got, ref = m.compute(), mr.evaluate(entries, [b1], TYPES, epoch=True)
    assert torch.isnan(got["f_Cs"]) and torch.isnan(got["f"]) and got["fmax"] == -math.inf
    for k in ref:
        close(got[k], ref[k], k)
    m.reset()
    assert torch.isnan(m.compute()["e"])


def test_standalone_metric_and_custom_entry():
    g = torch.Generator().manual_seed(3)
    p, t = torch.randn(11, 3, generator=g), torch.randn(11, 3, generator=g, dtype=torch.float64)
    rmse = RootMeanSquaredError()
    close(rmse(p, t), (p.double() - t).square().mean().sqrt())
    rmse.update(2 * p, t)
    close(rmse.compute(), torch.cat([p.double() - t, 2 * p.double() - t]).square().mean().sqrt())
    rmse.reset()
    assert torch.isnan(rmse.compute())

    class EnergyGap(torch.nn.Module):  # a custom metric: takes the two data dicts
        def forward(self, preds, target):
            return (preds["total_energy"].double() - target["total_energy"]).abs().sum()

        def compute(self):
            return torch.tensor(-1.0, dtype=torch.float64)

    with pytest.raises(TypeError, match="custom modules go with `field: None`"):
        MetricsManager([{"field": "forces", "metric": EnergyGap()}])
    m = MetricsManager([{"metric": EnergyGap(), "name": "gap", "coeff": 1.0},
                        {"field": "forces", "metric": MeanSquaredError(), "coeff": 3.0}])
    preds, target = batch([2, 3])
    out = m(preds, target)
    gap = (preds["total_energy"].double() - target["total_energy"]).abs().sum()
    close(out["gap"], gap)
    close(out["weighted_sum"], 0.25 * gap + 0.75 * out["F_mse"])
    assert m.metrics_values_step["gap"] == float(gap)
    assert m.compute()["gap"] == -1.0
    # entry order, also with a custom entry in front of a fused one (the order of the checkpointed dicts)
    assert list(m.metrics_values_step) == list(m.metrics_values_epoch) == ["gap", "F_mse"]
    extra = m.get_extra_state()
    assert list(extra["metrics_values_step"]) == list(extra["metrics_values_epoch"]) == ["gap", "F_mse"]


def test_metric_constants_and_struct_sizes_agree_with_the_header_and_the_library():
    """Every ``NQA_METRICS_*`` constant of ``_lib.py`` equals the ``#define`` of ``include/nequip_amd.h``, the workgroup count
    equals what the built library reports, and the ctypes structs have the size of the C structs."""
    import ctypes
    import os
    import re

    from nequip_amd import _lib
    from nequip_amd.train import _metrics_ops

    header = open(os.path.join(os.path.dirname(__file__), "..", "include", "nequip_amd.h")).read()
    defined = {k: int(v) for k, v in re.findall(r"#define\s+(NQA_METRICS_[A-Z_]+)\s+(\d+)", header)}
    assert set(defined) == {"NQA_METRICS_MAX_STREAMS", "NQA_METRICS_MAX_TERMS", "NQA_METRICS_MAX_TYPES",
                            "NQA_METRICS_MAX_STRATA", "NQA_METRICS_GROUPS"}
    assert defined == {k: getattr(_lib, k) for k in dir(_lib) if k.startswith("NQA_METRICS_")}
    assert _metrics_ops.NUM_WORKGROUPS == _lib.NQA_METRICS_GROUPS == _lib.load().nqa_metrics_groups()
    assert ctypes.sizeof(_lib.MetricTerm) == 312 and ctypes.sizeof(_lib.MetricStream) == 64


def test_metric_kernels_do_not_spill():
    """Latency-bound kernels: no scratch, no spills, and at most 128 VGPRs (so that four waves fit a SIMD), read from the
    built code object (no GPU)."""
    import os
    import sys

    root = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
    sys.path.insert(0, os.path.join(root, "scripts"))
    import kernel_resources as kr

    obj = os.path.join(kr.BUILD, "metrics.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("build objects / ROCm LLVM tools not present (run python -m nequip_amd.csrc.build)")
    ks = kr.kernels_of(obj)
    for needle in ("metrics_partial_kernel", "metrics_final_kernel", "metrics_bwd_kernel"):
        (r,) = [v for n, v in ks.items() if needle in n]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 128, (needle, r)
