"""The fused loss / metric kernels (``csrc/metrics.hip``: ``nqa_metrics_fwd`` / ``nqa_metrics_bwd``) on the GPU against
``tests/metrics_restatement.py``, the plain-torch float64 restatement of the reference's semantics (evaluated on the CPU).

The reference (nequip/train/metrics_manager.py) cannot be imported here -- it needs ``torchmetrics``, which is not
installed -- so there are no reference-generated fixtures for this feature.

Tolerances.  Values: rtol 1e-10 (float64 sums of fewer than 1e5 terms in another order differ by about n * 2^-53).
``grad_pred``, compared in float64: float64 predictions 1e-10 * max|ref|; float32 predictions 1e-6 * max|ref| (one rounding
to float32, 6e-8, under the project's usual 2e-6 bar).  Elements masked by ``ignore_nan``: exactly 0.0.
"""
import ctypes
import math

import pytest
import torch

import metrics_restatement as mr
from nequip_amd import _lib
from nequip_amd.data import PerAtomModifier, _stats_ops, register_fields
from nequip_amd.train import (EnergyForceLoss, EnergyForceStressLoss, EnergyForceStressMetrics, HuberLoss,
                              MaximumAbsoluteError, MeanAbsoluteError, MeanSquaredError, MetricsManager,
                              RootMeanSquaredError, StratifiedHuberForceLoss, _metrics_ops)

pytestmark = pytest.mark.gpu

TYPES = ["H", "O", "Cs"]
G = _metrics_ops.NUM_WORKGROUPS
F32, F64 = torch.float32, torch.float64
register_fields(node_fields=["fnan", "fall"])  # per-atom fields with some / with all targets NaN


def to_dict(e):
    """The ``MetricsManager`` entry of a restatement entry."""
    kind = e["kind"]
    if kind == "huber":
        metric = HuberLoss(delta=e["delta"], reduction=e.get("reduction", "mean"))
    elif kind == "stratified huber":
        metric = StratifiedHuberForceLoss(e["delta_dict"], reduction=e.get("reduction", "mean"))
    else:
        metric = {"mse": MeanSquaredError, "mae": MeanAbsoluteError, "rmse": RootMeanSquaredError,
                  "max_ae": MaximumAbsoluteError}[kind]()
    d = {"name": e["name"], "metric": metric, "coeff": e.get("coeff"),
         "field": PerAtomModifier(e["field"], e.get("factor")) if e.get("per_atom") else e["field"]}
    if e.get("per_type"):
        d["per_type"] = True
        if e.get("per_type_coeffs"):
            d["per_type_coeffs"] = dict(zip(TYPES, e["per_type_coeffs"]))
    if e.get("ignore_nan"):
        d["ignore_nan"] = True
    return d


def close(got, ref, what):
    torch.testing.assert_close(got.detach().cpu().double(), torch.as_tensor(ref, dtype=F64).detach(), rtol=1e-10, atol=0.0,
                               equal_nan=True, msg=lambda m: f"{what}: {m}")


def check(manager, entries, preds_cpu, target_cpu, device, grad_of="weighted_sum", extra_grad=None):
    """Names, values and prediction gradients of one batch, kernel (GPU) against restatement (CPU)."""
    floats = [k for k, v in preds_cpu.items() if v.is_floating_point()]
    p_ref = {k: (v.clone().requires_grad_(True) if k in floats else v) for k, v in preds_cpu.items()}
    p_gpu = {k: (v.to(device).requires_grad_(True) if k in floats else v.to(device)) for k, v in preds_cpu.items()}
    t_gpu = {k: v.to(device) for k, v in target_cpu.items()}
    got, ref = manager(p_gpu, t_gpu), mr.evaluate(entries, [(p_ref, target_cpu)], TYPES)
    assert list(got) == list(ref)
    for k in ref:
        close(got[k], ref[k], k)
    grads = {}
    for name in [grad_of] + ([extra_grad] if extra_grad else []):
        g_got = torch.autograd.grad(got[name], [p_gpu[k] for k in floats], allow_unused=True, retain_graph=True)
        if ref[name].requires_grad:
            g_ref = torch.autograd.grad(ref[name], [p_ref[k] for k in floats], allow_unused=True, retain_graph=True)
        else:  # (no rows: a constant)
            g_ref = [None] * len(floats)
        for k, a, b in zip(floats, g_got, g_ref):
            grads[(name, k)] = a
            if b is None:
                assert a is None or not a.any(), (name, k)
                continue
            assert a.dtype == preds_cpu[k].dtype and a.shape == preds_cpu[k].shape
            bound = (1e-6 if a.dtype == F32 else 1e-10) * float(b.abs().max()) if b.numel() else 0.0
            torch.testing.assert_close(a.cpu().double(), b.double(), rtol=0.0, atol=bound,
                                       msg=lambda m: f"d {name} / d {k}: {m}")
    return got, grads


def entries_for_kernel_test():
    e = []
    for i, (kind, kw) in enumerate([("mse", {}), ("mae", {}), ("rmse", {}), ("max_ae", {}), ("huber", {"delta": 0.7}),
                                    ("huber", {"delta": 0.4, "reduction": "sum"}),
                                    ("stratified huber", {"delta_dict": {1.0: 0.5, 3.0: 0.2}}),
                                    ("stratified huber", {"delta_dict": {0.0: 1.0, 2.0: 0.3, 4.0: 0.1}, "reduction": "sum"})]):
        e.append({"name": f"plain{i}", "field": "forces", "kind": kind, "coeff": None if kind == "max_ae" else 1.0 + i, **kw})
    for kind in ("mse", "rmse", "mae", "max_ae", "huber"):  # T = 3, the last type absent
        e.append({"name": f"pt_{kind}", "field": "forces", "kind": kind, "per_type": True, "delta": 0.7,
                  "coeff": None if kind == "max_ae" else 2.0})
    e.append({"name": "ptc_mse", "field": "forces", "kind": "mse", "per_type": True, "per_type_coeffs": [5.0, 1.0, 0.5],
              "coeff": 1.5})
    for field in ("fnan", "fall"):  # about a quarter / all of the targets NaN
        for kind in ("mse", "rmse", "max_ae"):
            e.append({"name": f"{field}_{kind}", "field": field, "kind": kind, "ignore_nan": True,
                      "coeff": None if kind == "max_ae" else 1.0})
        e.append({"name": f"{field}_pt_mae", "field": field, "kind": "mae", "ignore_nan": True, "per_type": True, "coeff": 1.0})
    for x in e:
        if x["kind"] != "huber":
            x.pop("delta", None)
    return e


@pytest.mark.parametrize("rows", [0, 1, 3, 257, G * 256 + 5])
@pytest.mark.parametrize("cols", [1, 3, 9])
@pytest.mark.parametrize("pred_dtype,target_dtype", [(F32, F32), (F32, F64), (F64, F32), (F64, F64)])
def test_kernel_against_restatement(device, rows, cols, pred_dtype, target_dtype):
    """Every metric kind, plain and per type (T = 3 with the last type absent; equal and weighted aggregate), ``ignore_nan``
    with a quarter and with all targets NaN, a non-contiguous prediction; rows: none, one, a few, past one workgroup, past
    one sweep of the grid.  Gradients of ``weighted_sum`` (through every term with a coefficient) and of one per-type value."""
    g = torch.Generator().manual_seed(rows * 10 + cols)
    types = torch.randint(0, 2, (rows,), generator=g)
    types[:1] = 0
    preds = {"forces": torch.randn(rows, 2 * cols, generator=g, dtype=pred_dtype)[:, ::2],  # non-contiguous
             "fnan": torch.randn(rows, cols, generator=g, dtype=pred_dtype),
             "fall": torch.randn(rows, cols, generator=g, dtype=pred_dtype), "atom_types": types}
    assert rows < 2 or not preds["forces"].is_contiguous()
    target = {"forces": (2.0 * torch.randn(rows, cols, generator=g, dtype=F64)).to(target_dtype),
              "fnan": torch.randn(rows, cols, generator=g, dtype=F64).to(target_dtype),
              "fall": torch.full((rows, cols), math.nan, dtype=target_dtype)}
    target["fnan"][torch.rand(rows, cols, generator=g) < 0.25] = math.nan
    entries = entries_for_kernel_test()
    manager = MetricsManager([to_dict(e) for e in entries], type_names=TYPES)
    got, grads = check(manager, entries, preds, target, device, extra_grad="pt_rmse_H" if rows else None)
    if rows:
        assert torch.isnan(got["pt_mse_Cs"]) and got["pt_max_ae_Cs"] == -math.inf and torch.isnan(got["fall_mse"])
        assert torch.isnan(got["weighted_sum"])  # the all-NaN terms give it their NaN ...
        masked = torch.isnan(target["fnan"])
        assert (grads[("weighted_sum", "fnan")].cpu()[masked] == 0).all()  # ... masked elements get exactly zero ...
        assert (grads[("weighted_sum", "fall")] == 0).all()
        assert torch.isfinite(grads[("weighted_sum", "forces")]).all()  # ... and the other gradients stay finite


def efs_batch(sizes, seed, absent_type, nan_frames):
    g = torch.Generator().manual_seed(seed)
    n, b = sum(sizes), len(sizes)
    types = torch.randint(0, 3, (n,), generator=g)
    if absent_type is not None:
        types[types == absent_type] = (absent_type + 1) % 3
    preds = {"total_energy": torch.randn(b, 1, generator=g, dtype=F64), "forces": torch.randn(n, 3, generator=g),
             "stress": torch.randn(b, 3, 3, generator=g), "num_atoms": torch.tensor(sizes), "atom_types": types}
    target = {"total_energy": torch.randn(b, 1, generator=g, dtype=F64), "forces": torch.randn(n, 3, generator=g, dtype=F64),
              "stress": torch.randn(b, 3, 3, generator=g, dtype=F64), "num_atoms": torch.tensor(sizes)}
    for f in nan_frames:
        target["stress"][f] = math.nan
    return preds, target


EFS_ENTRIES = (
    [{"name": f"{q}_{k}", "field": "total_energy" if "energy" in q else q, "kind": kind, "per_atom": q == "per_atom_energy",
      "ignore_nan": q == "stress", "coeff": 1.0 if (k == "rmse" and q != "per_atom_energy") else None}
     for q in ("total_energy", "per_atom_energy", "forces", "stress") for k, kind in (("rmse", "rmse"), ("mae", "mae"))]
    + [{"name": f"{q}_maxabserr", "field": "total_energy" if "energy" in q else q, "kind": "max_ae",
        "per_atom": q == "per_atom_energy", "ignore_nan": q == "stress"}
       for q in ("total_energy", "per_atom_energy", "forces", "stress")]
    + [{"name": f"forces_{k}_per_type", "field": "forces", "kind": kind, "per_type": True}
       for k, kind in (("rmse", "rmse"), ("mae", "mae"), ("maxabserr", "max_ae"))])


def efs_metrics():
    extra = [to_dict(e) for e in EFS_ENTRIES[12:]]
    return EnergyForceStressMetrics(type_names=TYPES, ignore_nan={"stress": True}, extra_metrics=extra)


def test_fused_manager_energy_force_stress_metrics(device):
    """``EnergyForceStressMetrics`` with per-type forces and ``ignore_nan`` stress: 15 terms on 4 streams, frames of 5, 64 and
    300 atoms; every returned name and value, then ``compute()`` after two batches."""
    m = efs_metrics()
    plan = m.__dict__["_plan"]
    assert plan.n_streams == 4 and len(plan.terms) == 15
    b1 = efs_batch([5, 64, 300], seed=1, absent_type=2, nan_frames=[1])
    b2 = efs_batch([7, 33], seed=2, absent_type=None, nan_frames=[])
    check(m, EFS_ENTRIES, *b1, device)
    m(*[{k: v.to(device) for k, v in d.items()} for d in b2])
    got, ref = m.compute(), mr.evaluate(EFS_ENTRIES, [b1, b2], TYPES, epoch=True)
    assert list(got) == list(ref)
    for k in ref:
        close(got[k], ref[k], f"epoch {k}")
    for k, v in m.metrics_values_epoch.items():  # one copy to the host, on first access
        assert abs(v - float(ref[k])) <= 1e-10 * abs(float(ref[k]))
    m.reset()
    assert torch.isnan(m.compute()["forces_rmse"])


def test_bitwise_reproducible(device):
    preds, target = efs_batch([5, 64, 300, 4000], seed=3, absent_type=None, nan_frames=[2])
    runs = []
    for _ in range(2):
        loss = EnergyForceStressLoss(per_type_forces_coeffs={"H": 5.0, "O": 1.0, "Cs": 0.5}, type_names=TYPES,
                                     ignore_nan={"stress": True})
        p = {k: (v.to(device).requires_grad_(True) if v.is_floating_point() else v.to(device)) for k, v in preds.items()}
        out = loss(p, {k: v.to(device) for k, v in target.items()})
        out["weighted_sum"].backward()
        runs.append([v.detach().clone() for v in out.values()] + [p[k].grad for k in ("total_energy", "forces", "stress")])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_graph_capture_and_replay_with_new_contents(device):
    """Forward + backward of ``EnergyForceStressLoss`` (per-type forces, ``ignore_nan`` stress) captured once, replayed after
    the static buffers got new contents in which one type has become absent and the NaN pattern has changed: nothing in the
    path may depend on data the host has read."""
    sizes = [5, 64, 300]
    coeffs = {"H": 5.0, "O": 1.0, "Cs": 0.5}
    entries = [{"name": "per_atom_energy_mse", "field": "total_energy", "kind": "mse", "per_atom": True, "coeff": 1.0},
               {"name": "forces_mse", "field": "forces", "kind": "mse", "per_type": True, "per_type_coeffs": [5.0, 1.0, 0.5],
                "coeff": 1.0},
               {"name": "stress_mse", "field": "stress", "kind": "mse", "ignore_nan": True, "coeff": 1.0}]
    loss = EnergyForceStressLoss(per_type_forces_coeffs=coeffs, type_names=TYPES, ignore_nan={"stress": True})
    first = efs_batch(sizes, seed=4, absent_type=None, nan_frames=[0])
    second = efs_batch(sizes, seed=5, absent_type=1, nan_frames=[1, 2])
    floats = ("total_energy", "forces", "stress")
    p = {k: (v.to(device).requires_grad_(True) if k in floats else v.to(device)) for k, v in first[0].items()}
    t = {k: v.to(device) for k, v in first[1].items()}

    def step():
        out = loss(p, t)
        return out, torch.autograd.grad(out["weighted_sum"], [p[k] for k in floats])

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, grads = step()
    for batch in (first, second):
        with torch.no_grad():
            for k, v in batch[0].items():
                p[k].copy_(v)
            for k, v in batch[1].items():
                t[k].copy_(v)
        graph.replay()
        torch.cuda.synchronize()
        p_ref = {k: (v.clone().requires_grad_(True) if k in floats else v) for k, v in batch[0].items()}
        ref = mr.evaluate(entries, [(p_ref, batch[1])], TYPES)
        assert list(out) == list(ref)
        for k in ref:
            close(out[k], ref[k], k)
        g_ref = torch.autograd.grad(ref["weighted_sum"], [p_ref[k] for k in floats])
        for k, a, b in zip(floats, grads, g_ref):
            bound = (1e-6 if a.dtype == F32 else 1e-10) * float(b.abs().max())
            torch.testing.assert_close(a.cpu().double(), b.double(), rtol=0.0, atol=bound, msg=lambda m: f"grad {k}: {m}")
    assert torch.isnan(out["forces_mse_O"])  # the second contents: no oxygen
    assert (grads[2][1:] == 0).all() and (grads[2][0] != 0).all()


def test_energy_force_loss_on_the_model_equals_the_hand_written_expression(device):
    """``EnergyForceLoss()(out, target)["weighted_sum"].backward()`` gives every parameter of the small water model of
    ``tests/test_training_step.py`` the gradient of ``0.5 mean((E/N - Et/N)^2) + 0.5 mean((F - Ft)^2)`` on the same GPU model.
    Bound: the one ``test_deferred_parameter_gradients_equal_autograd`` uses for two passes through the same kernels."""
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=2, seed=7)
    data = AtomicDataDict.to_device(syn.make_data(pos, types, 4.0, cell), device)
    n = len(pos)
    model = NequIPGNNModel(seed=5, model_dtype="float32", type_names=names, r_max=4.0, num_layers=3, l_max=2, parity=False,
                           num_features=8, radial_mlp_depth=1, radial_mlp_width=16, num_bessels=8, polynomial_cutoff_p=6,
                           avg_num_neighbors=25.0).to(device).train()
    gen = torch.Generator().manual_seed(0)
    target = {"forces": torch.randn(n, 3, generator=gen, dtype=F64).to(device),
              "total_energy": torch.randn(1, 1, generator=gen, dtype=F64).to(device),
              "num_atoms": torch.tensor([n], device=device)}

    out = model(dict(data))
    e, f = out["total_energy"], out["forces"]
    ref_loss = 0.5 * ((e / n - target["total_energy"] / n) ** 2).mean() + 0.5 * ((f - target["forces"]) ** 2).mean()
    ref_loss.backward()
    ref = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    model.zero_grad(set_to_none=True)

    out = dict(model(dict(data)))
    out["num_atoms"] = target["num_atoms"]
    loss = EnergyForceLoss()(out, target)
    torch.testing.assert_close(loss["weighted_sum"].detach(), ref_loss.detach().double(), rtol=1e-6, atol=0.0)
    loss["weighted_sum"].backward()
    for k, p in model.named_parameters():
        assert p.grad is not None, f"no gradient for {k}"
        r = ref[k]
        torch.testing.assert_close(p.grad, r, atol=2e-6 * max(1e-3, float(r.abs().max())), rtol=2e-5,
                                   msg=lambda m, k=k: f"{k}: {m}")


def test_thirty_two_terms_on_one_stream(device):
    """The term limit on ONE stream: the first stage then keeps 32 x 256 float64 values in LDS, more than the 64 KiB a
    kernel gets without asking.  Every kind, four of the terms per type; 257 rows (past one workgroup)."""
    kinds = [("mse", {}), ("mae", {}), ("rmse", {}), ("max_ae", {}), ("huber", {"delta": 0.7}),
             ("huber", {"delta": 0.4, "reduction": "sum"}), ("stratified huber", {"delta_dict": {1.0: 0.5, 3.0: 0.2}})]
    entries = []
    for i in range(_metrics_ops.MAX_TERMS):
        kind, kw = kinds[i % len(kinds)]
        e = {"name": f"t{i}", "field": "forces", "kind": kind, "coeff": None if kind == "max_ae" else 1.0 + i, **kw}
        if i >= 28 and kind != "stratified huber":
            e["per_type"] = True
        entries.append(e)
    assert sum(bool(e.get("per_type")) for e in entries) == 4
    manager = MetricsManager([to_dict(e) for e in entries], type_names=TYPES)
    plan = manager.__dict__["_plan"]
    assert plan.n_streams == 1 and len(plan.terms) == 32 and plan.n_slots == 28 + 4 * 3
    g = torch.Generator().manual_seed(11)
    rows = 257
    types = torch.randint(0, 2, (rows,), generator=g)
    preds = {"forces": torch.randn(rows, 3, generator=g), "atom_types": types}
    target = {"forces": 2.0 * torch.randn(rows, 3, generator=g, dtype=F64)}
    check(manager, entries, preds, target, device, extra_grad="t30_O")


def test_coefficients_changed_between_forward_and_backward_are_refused(device):
    """``set_coeffs`` rewrites the device table in place; a backward whose forward saw the previous table would pair new
    coefficients with old values, so it raises.  The next step works."""
    preds, target = efs_batch([5, 9], seed=6, absent_type=None, nan_frames=[])
    loss = EnergyForceLoss()
    t = {k: v.to(device) for k, v in target.items()}

    def forward():
        p = {k: (v.to(device).requires_grad_(True) if v.is_floating_point() else v.to(device)) for k, v in preds.items()}
        return p, loss(p, t)

    p, out = forward()
    loss.set_coeffs({"per_atom_energy_mse": 1.0, "forces_mse": 3.0})
    with pytest.raises(RuntimeError, match="between this backward and its forward"):
        out["weighted_sum"].backward()
    p, out = forward()
    out["weighted_sum"].backward()
    entries = [{"name": "per_atom_energy_mse", "field": "total_energy", "kind": "mse", "per_atom": True, "coeff": 1.0},
               {"name": "forces_mse", "field": "forces", "kind": "mse", "coeff": 3.0}]
    p_ref = {k: (v.clone().requires_grad_(True) if v.is_floating_point() else v) for k, v in preds.items()}
    ref = mr.evaluate(entries, [(p_ref, target)], TYPES)
    close(out["weighted_sum"], ref["weighted_sum"], "weighted_sum")
    (g_ref,) = torch.autograd.grad(ref["weighted_sum"], [p_ref["forces"]])
    torch.testing.assert_close(p["forces"].grad.cpu().double(), g_ref.double(), rtol=0.0, atol=1e-6 * float(g_ref.abs().max()))


# (term streams, term slot0s, number of streams) that break one rule of the term table each, and the rule's message
BAD_LAYOUTS = {"terms out of stream order": ([1, 0], [0, 1], 2, "terms must be ordered by stream"),
               "a gap in slot0": ([0, 1], [0, 2], 2, "slots must be contiguous in term order"),
               "a stream without terms": ([0, 2], [0, 1], 3, "a stream without terms"),
               "nine streams": ([0, 8], [0, 1], 9, "1 to 8 streams")}


@pytest.mark.parametrize("rule", list(BAD_LAYOUTS))
def test_layout_checks_of_both_entry_points(device, rule):
    """``nqa_metrics_fwd`` and ``nqa_stats_update`` check the term table by the same code (csrc/slot_reduce.h): each refuses
    the table with ``NQA_ERR_INVALID`` and the rule's message under its own name, before any launch -- the streams hold four
    rows each, so a launch would write the workspace, the state and the values."""
    term_streams, slot0s, n_streams, message = BAD_LAYOUTS[rule]
    lib, n_terms = _lib.load(), len(term_streams)
    x = torch.randn(4, 1, dtype=F64, device=device)
    sentinel = lambda n: torch.full((n,), -12345, dtype=torch.int64, device=device)
    workspace, state, saved, values = sentinel(4096), sentinel(64), sentinel(64), sentinel(64).double()
    before = [t.clone() for t in (workspace, state, saved, values)]

    m_streams, m_terms = (_lib.MetricStream * n_streams)(), (_lib.MetricTerm * n_terms)()
    for c in m_streams:
        c.pred, c.target, c.rows, c.cols = x.data_ptr(), x.data_ptr(), 4, 1
        c.pred_dtype, c.target_dtype = _lib.NQA_F64, _lib.NQA_F64
    for k, c in enumerate(m_terms):
        c.stream, c.kind, c.n_groups, c.slot0, c.out0 = term_streams[k], _metrics_ops.MSE, 1, slot0s[k], k
    table = torch.zeros(ctypes.sizeof(m_terms), dtype=torch.uint8, device=device)
    rc = lib.nqa_metrics_fwd(m_streams, n_streams, m_terms, _lib.ptr(table), n_terms, n_terms + 1, n_terms, _lib.ptr(workspace),
                             workspace.numel() * 8, _lib.ptr(state), _lib.ptr(saved), _lib.ptr(values), _lib.stream_ptr(device))
    assert rc == -1 and lib.nqa_last_error().decode() == f"nqa_metrics_fwd: {message}"  # NQA_ERR_INVALID

    s_streams, s_terms = (_lib.StatsStream * n_streams)(), (_lib.StatsTerm * n_terms)()
    for c in s_streams:
        c.data, c.rows, c.cols, c.dtype, c.group_kind = x.data_ptr(), 4, 1, _lib.NQA_STATS_F64, _stats_ops.GROUP_NONE
    for k, c in enumerate(s_terms):
        c.stream, c.mod, c.n_groups, c.slot0 = term_streams[k], _stats_ops.IDENTITY, 1, slot0s[k]
    rc = lib.nqa_stats_update(s_streams, n_streams, s_terms, n_terms, _lib.ptr(workspace), workspace.numel() * 8,
                              _lib.ptr(state), _lib.stream_ptr(device))
    assert rc == -1 and lib.nqa_last_error().decode() == f"nqa_stats_update: {message}"

    torch.cuda.synchronize(device)
    for t, b in zip((workspace, state, saved, values), before):
        assert torch.equal(t, b)
