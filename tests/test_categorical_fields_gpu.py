"""Categorical graph-field embeddings on the GPU against the unmodified float64 oracle.

The oracle knows one type table only.  A model with fields is the oracle's model over CLASSES: class ``t + T c`` is atom
type ``t`` in a frame whose field values are the ``c``-th distinct combination, its embedding row is
``cat(type_row[t], field rows of c)`` and ``type_embed_num_features`` is ``F_total``; the per-type energy scales / shifts
are repeated per class.  Every evaluation here must stay on the HIP node kernels: the outer-product self-connection
(``FullyConnectedTensorProduct.forward``) is patched to raise."""

import pytest
import torch

from oracle import model as omodel

FIELDS = [{"field": "charge", "num_features": 5, "min": -1, "max": 2},
          {"field": "spin", "num_features": 4, "min": 0, "max": 2}]
TYPE_F = 8  # F_total = 8 + 5 + 4 = 17: not a multiple of 32
SCALES, SHIFTS = {"H": 1.3, "O": 0.7}, {"H": -1.0, "O": 2.0}


def _cfg(model_dtype="float32"):
    return dict(r_max=4.0, num_layers=3, l_max=2, parity=False, num_features=16, radial_mlp_depth=1, radial_mlp_width=32,
                num_bessels=8, polynomial_cutoff_p=6, avg_num_neighbors=25.0, model_dtype=model_dtype)


def _model(cfg, names, fields=FIELDS, seed=3):
    from nequip_amd.model import NequIPGNNModel

    return NequIPGNNModel(seed=seed, type_names=names, type_embed_num_features=TYPE_F, categorical_graph_field_embed=fields,
                          per_type_energy_scales=SCALES, per_type_energy_shifts=SHIFTS,
                          **{k: v for k, v in cfg.items()})


def _frames(n, seed=0):
    """``n`` small water boxes of different sizes / geometries with mixed (charge, spin) labels."""
    from nequip_amd.utils import synthetic as syn

    frames = []
    labels = [(0, 0), (1, 2), (-1, 1), (2, 0), (1, 2), (0, 1), (-1, 0), (2, 2)]
    for f in range(n):
        pos, types, cell, names = syn.water_box(n_side=2, seed=seed + f)
        d = syn.make_data(pos, types, 4.0, cell)
        q, s = labels[f % len(labels)]
        d["charge"], d["spin"] = torch.tensor([q]), torch.tensor([s])
        frames.append(d)
    return frames, names


def _no_outer_product(monkeypatch):
    from nequip_amd.o3.modules import FullyConnectedTensorProduct

    def boom(self, *a, **k):
        raise AssertionError("the outer-product (ATen) self-connection ran")

    monkeypatch.setattr(FullyConnectedTensorProduct, "forward", boom)


def _oracle_view(model, data, weights=None):
    """(oracle data, oracle cfg, oracle weights) of ``model`` on ``data``: classes in place of types."""
    sd = weights if weights is not None else {k.replace("model.func.", ""): v.detach().cpu()
                                               for k, v in model.state_dict().items()}
    emb = model.model.func.type_embed
    T = emb.num_types
    fields = list(emb.categorical_graph_field_embed_modules.keys())
    vals = torch.stack([data[f].view(-1).cpu() for f in fields], 1)  # [G, n_fields]
    combos = sorted(set(tuple(int(v) for v in row) for row in vals))
    cls_of_frame = torch.tensor([combos.index(tuple(int(v) for v in row)) for row in vals])
    batch = data.get("batch")
    frame = batch.cpu() if batch is not None else torch.zeros(data["atom_types"].numel(), dtype=torch.long)
    w = {k: v for k, v in sd.items() if "categorical_graph_field_embed_modules" not in k}
    type_w = sd["type_embed.embed_module.weight"]
    rows = []
    for c in combos:
        parts = [type_w]
        for f, k in zip(fields, c):
            tb = sd[f"type_embed.categorical_graph_field_embed_modules.{f}.weight"]
            parts.append(tb[k - emb.categorical_graph_field_embed_shifts[f]].view(1, -1).expand(T, -1))
        rows.append(torch.cat(parts, 1))
    w["type_embed.embed_module.weight"] = torch.cat(rows, 0)
    C = len(combos)
    for key in ("per_type_energy_scale_shift.scales", "per_type_energy_scale_shift.shifts"):
        if key in w and w[key].numel() > 1:
            w[key] = w[key].view(-1).repeat(C)
    od = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in data.items() if k not in fields}
    od["atom_types"] = data["atom_types"].view(-1).cpu() + T * cls_of_frame[frame]
    return od, w


def _ocfg(cfg, model):
    return dict(cfg, type_embed_num_features=model.model.func.type_embed.irreps_out["node_attrs"].dim)


def _check(ref, out, dtype, n):
    tol = 5e-5 if dtype == "float32" else 1e-9
    fscale = max(1.0, float(ref["forces"].abs().max()))
    torch.testing.assert_close(ref["total_energy"].view(-1), out["total_energy"].detach().cpu().view(-1).double(),
                               atol=tol * n, rtol=tol)
    torch.testing.assert_close(ref["forces"], out["forces"].detach().cpu().double(), atol=tol * fscale, rtol=tol)
    torch.testing.assert_close(ref["virial"].view(-1, 3, 3), out["virial"].detach().cpu().view(-1, 3, 3).double(),
                               atol=tol * n * fscale, rtol=10 * tol)


@pytest.mark.gpu
@pytest.mark.parametrize("model_dtype", ["float32", "float64"])
def test_single_frame_and_batch_against_oracle(device, model_dtype, monkeypatch):
    from nequip_amd.data import AtomicDataDict

    _no_outer_product(monkeypatch)
    cfg = _cfg(model_dtype)
    frames, names = _frames(7)
    model = _model(cfg, names).to(device).eval()
    for data in [frames[1], AtomicDataDict.batched_from_list(frames)]:
        out = model(AtomicDataDict.to_device(dict(data), device))
        od, w = _oracle_view(model, data)
        ref = omodel.energy_forces(od, _ocfg(cfg, model), w, with_virial=True)
        _check(ref, out, model_dtype, data["pos"].shape[0])
        assert "stress" in out and torch.isfinite(out["stress"]).all()


@pytest.mark.gpu
def test_same_geometry_different_charge(device, monkeypatch):
    from nequip_amd.data import AtomicDataDict

    _no_outer_product(monkeypatch)
    frames, names = _frames(1)
    a = dict(frames[0])
    b = dict(frames[0], charge=torch.tensor([2]))
    model = _model(_cfg(), names).to(device).eval()
    batch = model(AtomicDataDict.to_device(AtomicDataDict.batched_from_list([a, b]), device))["total_energy"].view(-1)
    ea = model(AtomicDataDict.to_device(dict(a), device))["total_energy"].view(-1)
    eb = model(AtomicDataDict.to_device(dict(b), device))["total_energy"].view(-1)
    assert abs(float(ea - eb)) > 1e-3
    torch.testing.assert_close(batch.cpu(), torch.cat([ea, eb]).cpu(), atol=5e-5 * 24, rtol=5e-5)


def _force_loss_grads(model, data, device, weights_cpu=None):
    from nequip_amd.data import AtomicDataDict

    gen = torch.Generator().manual_seed(0)
    n = data["pos"].shape[0]
    f_t = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    out = model(AtomicDataDict.to_device(dict(data), device))
    loss = (out["forces"] - f_t.to(device)).square().mean() + out["total_energy"].square().mean() / n
    model.zero_grad(set_to_none=True)
    loss.backward()
    return loss.detach(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}, f_t


@pytest.mark.gpu
@pytest.mark.parametrize("model_dtype", ["float64", "float32"])
@pytest.mark.parametrize("nframes", [1, 6])
def test_training_gradients_against_oracle(device, model_dtype, nframes, monkeypatch):
    """Force-matching loss (second order): gradients of the type table, the field tables and every sc weight."""
    from nequip_amd.data import AtomicDataDict

    _no_outer_product(monkeypatch)
    cfg = _cfg(model_dtype)
    frames, names = _frames(nframes, seed=4)
    data = frames[0] if nframes == 1 else AtomicDataDict.batched_from_list(frames)
    model = _model(cfg, names)
    sd = {k.replace("model.func.", ""): v.detach().clone() for k, v in model.state_dict().items()}
    pnames = {k.replace("model.func.", "") for k, _ in model.named_parameters()}
    leaves = {k: v.requires_grad_(k in pnames) for k, v in sd.items()}
    model = model.to(device).train()
    loss, grads, f_t = _force_loss_grads(model, data, device)

    od, w = _oracle_view(model, data, weights=leaves)
    ref = omodel.energy_forces(od, _ocfg(cfg, model), w, create_graph=True)
    n = data["pos"].shape[0]
    loss_ref = (ref["forces"] - f_t).square().mean() + ref["total_energy"].square().mean() / n
    names_w = [k for k, v in leaves.items() if v.requires_grad]
    gref = dict(zip(names_w, torch.autograd.grad(loss_ref, [leaves[k] for k in names_w], allow_unused=True)))
    tol = 1e-8 if model_dtype == "float64" else 2e-4
    torch.testing.assert_close(loss_ref.detach(), loss.cpu(), atol=tol, rtol=tol)
    checked = set()
    for k, g in grads.items():
        key = k.replace("model.func.", "")
        r = gref[key]
        assert r is not None, key
        torch.testing.assert_close(r, g.cpu(), atol=tol * max(1e-3, float(r.abs().max())), rtol=tol * 10, msg=key)
        checked.add(key)
    for want in ("type_embed.embed_module.weight", "type_embed.categorical_graph_field_embed_modules.charge.weight",
                 "type_embed.categorical_graph_field_embed_modules.spin.weight", "layer1_convnet.conv.sc.weight",
                 "layer2_convnet.conv.sc.weight"):
        assert want in checked, want


@pytest.mark.gpu
def test_batched_weight_gradients_are_deterministic(device, monkeypatch):
    from nequip_amd.data import AtomicDataDict

    _no_outer_product(monkeypatch)
    frames, names = _frames(8, seed=9)
    data = AtomicDataDict.batched_from_list(frames)
    model = _model(_cfg(), names).to(device).train()
    _, g1, _ = _force_loss_grads(model, data, device)
    _, g2, _ = _force_loss_grads(model, data, device)
    for k in g1:
        if "sc.weight" in k or "categorical" in k or "embed_module" in k:
            assert torch.equal(g1[k], g2[k]), k
    # first-order (no graph requested): the per-class nqa_wgrad launches
    model.zero_grad(set_to_none=True)
    outs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        out = model(AtomicDataDict.to_device(dict(data), device))
        out["total_energy"].sum().backward()
        outs.append({k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None})
    for k in outs[0]:
        assert torch.equal(outs[0][k], outs[1][k]), k


def _node_kernel_names(model, data, device):
    from torch.profiler import ProfilerActivity, profile

    from nequip_amd.data import AtomicDataDict

    d = AtomicDataDict.to_device(dict(data), device)
    model(dict(d))
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        model(dict(d))
        torch.cuda.synchronize()
    names = [e.key for e in prof.key_averages()]
    return names, {n: e.count for n, e in zip(names, prof.key_averages()) if "node" in n or "gate" in n}


@pytest.mark.gpu
def test_single_frame_runs_the_plain_models_node_kernels(device, monkeypatch):
    _no_outer_product(monkeypatch)
    frames, names = _frames(1)
    cfg = _cfg()
    plain = _model(cfg, names, fields=None).to(device).eval()
    withf = _model(cfg, names).to(device).eval()
    data = frames[0]
    try:
        all_p, node_p = _node_kernel_names(plain, {k: v for k, v in data.items() if k not in ("charge", "spin")}, device)
        all_f, node_f = _node_kernel_names(withf, data, device)
    except Exception as exc:  # pragma: no cover
        pytest.skip(f"no device activity records here: {exc}")
    if not any("nqa" in n or "node" in n for n in all_p):
        pytest.skip("the profiler returned no kernel names on this box")
    assert node_p and node_f == node_p, (node_p, node_f)
    assert any("fused" in n for n in node_f), node_f  # the fused node stage still runs with the folded table


@pytest.mark.gpu
def test_spatial_order_equals_unordered(device, monkeypatch):
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.utils import synthetic as syn

    _no_outer_product(monkeypatch)
    pos, types, cell, names = syn.water_box(n_side=4, seed=2)
    data = syn.make_data(pos, types, 4.0, cell)
    data["charge"], data["spin"] = torch.tensor([1]), torch.tensor([2])
    model = _model(_cfg(), names).to(device).eval()
    d = AtomicDataDict.to_device(data, device)
    plain = model(dict(d))
    monkeypatch.setenv("NQA_SPATIAL_ORDER_MIN", "1")
    model(dict(d))  # (first call with the cached topology builds the order)
    ordered = model(dict(d))
    torch.testing.assert_close(ordered["total_energy"], plain["total_energy"], atol=5e-5 * len(pos), rtol=1e-5)
    torch.testing.assert_close(ordered["forces"], plain["forces"], atol=1e-4, rtol=1e-4)


class _Atoms:
    def __init__(self, symbols, positions, cell):
        import numpy as np

        self._s, self._p, self._c = list(symbols), np.asarray(positions, dtype=np.float64), np.asarray(cell)

    def get_chemical_symbols(self):
        return self._s

    def get_positions(self):
        return self._p

    def get_cell(self):
        return self._c

    def get_pbc(self):
        import numpy as np

        return np.array([True] * 3)

    def __len__(self):
        return len(self._s)


@pytest.mark.gpu
def test_ase_calculator_with_charge_transform_and_refusals(device, monkeypatch):
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.integrations.ase import NequIPCalculator
    from nequip_amd.integrations.graphed_step import GraphedStep
    from nequip_amd.utils import synthetic as syn

    _no_outer_product(monkeypatch)
    pos, types, cell, names = syn.water_box(n_side=2, seed=5)
    model = _model(_cfg(), names).to(device).eval()

    def set_fields(data):
        data["charge"] = torch.tensor([1], device=data["pos"].device)
        data["spin"] = torch.tensor([0], device=data["pos"].device)
        return data

    calc = NequIPCalculator(model, device=device, r_max=4.0, chemical_symbols=names, transforms=[set_fields])
    atoms = _Atoms([names[t] for t in types], pos, cell)
    calc.calculate(atoms, properties=("energy", "forces"))
    data = syn.make_data(pos, types, 4.0, cell)
    data["charge"], data["spin"] = torch.tensor([1]), torch.tensor([0])
    out = model(AtomicDataDict.to_device(data, device))
    assert abs(calc.results["energy"] - float(out["total_energy"])) < 5e-5 * len(pos)
    torch.testing.assert_close(torch.as_tensor(calc.results["forces"]), out["forces"].detach().cpu().double(),
                               atol=1e-4, rtol=1e-4)
    with pytest.raises(NotImplementedError, match="categorical_graph_field_embed"):
        NequIPCalculator(model, device=device, r_max=4.0, chemical_symbols=names, graphed_md=True)
    with pytest.raises(NotImplementedError, match="categorical_graph_field_embed"):
        GraphedStep(model, torch.as_tensor(types).to(device), torch.as_tensor(cell).to(device), True, 4.0)
