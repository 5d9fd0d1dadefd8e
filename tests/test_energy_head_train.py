"""The training energy head (``nqa_energy_head_train_bwd / _bwd_bwd``, ``nn/_energy_head.py::energy_head_train``): Gate
(scalars) -> depth-0 readout -> PerTypeScaleShift with TRAINABLE tables, differentiable to second order in the features, with
the gradients of the readout weight and of the two tables from the same launches."""
import os
import subprocess
import sys

import pytest
import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
ACTS = {"silu": (1, torch.nn.functional.silu, 1.6791767923989418), "tanh": (2, torch.tanh, 1.5927812698663606)}


def _inputs(device, n, d, n_types, seed=3):
    g = torch.Generator().manual_seed(seed + 17 * n + d + n_types)
    h = (torch.randn(n, d, generator=g) * 2.0).to(device)
    w = ((torch.rand(d, generator=g) * 2 * 3 ** 0.5 - 3 ** 0.5) / d ** 0.5).to(device)
    # the last type has no atom (n_types == 1: the single type has them all)
    types = (torch.arange(n) % max(n_types - 1, 1))[torch.randperm(n, generator=g)].to(device)
    scales = (torch.rand(n_types, generator=g, dtype=torch.float64) + 0.5).to(device)
    shifts = torch.randn(n_types, generator=g, dtype=torch.float64).to(device)
    c = torch.randn(n, 1, generator=g, dtype=torch.float64).to(device)  # the energy gradient
    v = torch.randn(n, d, generator=g).to(device)  # the cotangent of the feature gradient
    return h, w, types, scales, shifts, c, v


def _both_orders(energy_fn, h, w, scales, shifts, c, v):
    """E, its gradients for the energy gradient ``c``, and the gradients of <g_h, v> (second order)."""
    h, w, scales, shifts, c = (t.detach().clone().requires_grad_(True) for t in (h, w, scales, shifts, c))
    e = energy_fn(h, w, scales, shifts)
    gh, gw, gsc, gsh = torch.autograd.grad((e * c).sum(), [h, w, scales, shifts], create_graph=True)
    gc, gh2, gw2, gsc2 = torch.autograd.grad((gh * v).sum(), [c, h, w, scales])
    first = dict(e=e, gh=gh, gw=gw, gscale=gsc, gshift=gsh)
    second = dict(gg=gc, gh2=gh2, gw2=gw2, gscale2=gsc2)
    return {k: t.detach() for k, t in {**first, **second}.items()}


def _chain(act_fn, cst, types):
    def energy(h, w, scales, shifts):  # as the modules compute it: float32 readout, float64 tables
        e32 = torch.mm(cst * act_fn(h), w.view(-1, 1))
        sc = torch.nn.functional.embedding(types, scales.view(-1, 1))
        sh = torch.nn.functional.embedding(types, shifts.view(-1, 1))
        return torch.addcmul(sh, sc, e32.to(torch.float64))

    return energy


def _head(act, cst, types):
    from nequip_amd.nn._energy_head import energy_head_train

    return lambda h, w, scales, shifts: energy_head_train(h, w, scales, shifts, types, act, cst)


# N = 4100: more atoms than one sweep of the 256 workgroups covers (a workgroup then walks several atoms per slot)
@pytest.mark.gpu
@pytest.mark.parametrize("n_types", [1, 3])
@pytest.mark.parametrize("act", ["silu", "tanh"])
@pytest.mark.parametrize("n,d", [(3, 32), (3, 64), (1001, 32), (1001, 64), (4100, 96)])
def test_training_head_matches_the_chain(device, n, d, act, n_types):
    act_id, act_fn, cst = ACTS[act]
    h, w, types, scales, shifts, c, v = _inputs(device, n, d, n_types)
    ref = _both_orders(_chain(act_fn, cst, types), h, w, scales, shifts, c, v)
    out = _both_orders(_head(act_id, cst, types), h, w, scales, shifts, c, v)
    for k in ("e", "gh", "gw", "gscale", "gshift", "gg", "gh2", "gw2", "gscale2"):
        assert out[k].shape == ref[k].shape and out[k].dtype == ref[k].dtype, k
        err, scale = float((out[k] - ref[k]).abs().max()), float(ref[k].abs().max())
        print(f"{k}: max|err| {err:.3e}  max|ref| {scale:.3e}  ratio {err / max(scale, 1e-300):.3e}")
        torch.testing.assert_close(out[k], ref[k], atol=2e-6 * scale, rtol=0, msg=lambda m, k=k: f"{k}: {m}")
    if n_types > 1:
        for k in ("gscale", "gshift", "gscale2"):  # the type without an atom
            assert float(out[k][-1]) == 0.0 and float(out[k][:-1].abs().min()) > 0.0, k


@pytest.mark.gpu
def test_training_head_without_atoms(device):
    h, w, types, scales, shifts, c, v = _inputs(device, 0, 32, 3)
    out = _both_orders(_head(1, ACTS["silu"][2], types), h, w, scales, shifts, c, v)
    torch.cuda.synchronize()
    assert out["e"].shape == (0, 1) and out["gh"].shape == (0, 32)
    for k in ("gw", "gscale", "gshift", "gw2", "gscale2"):
        assert float(out[k].abs().max()) == 0.0, k


@pytest.mark.gpu
def test_parameter_gradients_are_reproducible(device):
    h, w, types, scales, shifts, c, v = _inputs(device, 1001, 64, 3)
    fn = _head(1, ACTS["silu"][2], types)
    a = _both_orders(fn, h, w, scales, shifts, c, v)
    b = _both_orders(fn, h, w, scales, shifts, c, v)
    for k in ("gw", "gscale", "gshift", "gw2", "gscale2"):
        assert torch.equal(a[k], b[k]), k


# ---- model level -----------------------------------------------------------------------------------------------------------
def _water_model(device, trainable=True, **kw):
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=3, seed=4)
    data = AtomicDataDict.to_device(syn.make_data(pos, types, 4.5, cell), device)
    model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=2, l_max=1, parity=False,
                           num_features=32, radial_mlp_depth=1, radial_mlp_width=64, avg_num_neighbors=38.0,
                           per_type_energy_scales={"H": 1.3, "O": 0.7}, per_type_energy_shifts={"H": -1.0, "O": 2.0},
                           per_type_energy_scales_trainable=trainable, per_type_energy_shifts_trainable=trainable,
                           **kw).to(device)
    return model, data


def _spy(monkeypatch):
    from nequip_amd.nn import _energy_head

    fwd, train = [], []
    real, real_train = _energy_head._launch, _energy_head._launch_train
    monkeypatch.setattr(_energy_head, "_launch", lambda b, *a: (fwd.append(b), real(b, *a))[1])
    monkeypatch.setattr(_energy_head, "_launch_train", lambda o, *a: (train.append(o), real_train(o, *a))[1])
    return fwd, train


def _loss_gradients(model, data):
    model.zero_grad(set_to_none=True)
    out = model(dict(data))
    loss = out["total_energy"].square().sum() + out["forces"].square().sum()
    loss.backward()
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.gpu
def test_training_step_runs_the_training_head_and_matches_the_chain(device, monkeypatch):
    model, data = _water_model(device)
    model.train()
    fwd, train = _spy(monkeypatch)
    grads = _loss_gradients(model, data)
    # forward; the first backward inside ForceStressOutput and again for the energy term of the loss; the second backward
    assert fwd == [0] and sorted(set(train)) == [1, 2] and train[0] == 1, (fwd, train)
    assert set(grads) == {k for k, _ in model.named_parameters()}
    monkeypatch.setenv("NQA_NO_ENERGY_HEAD", "1")
    fwd.clear(), train.clear()
    ref = _loss_gradients(model, data)
    assert fwd == [] and train == []
    tol = 2e-4  # tests/test_training_step.py, float32 HIP kernels against ATen
    for k, r in ref.items():
        torch.testing.assert_close(grads[k], r, atol=tol * max(1e-3, float(r.abs().max())), rtol=tol * 10,
                                   msg=lambda m, k=k: f"{k}: {m}")
    for k in ("scales", "shifts"):
        assert float(grads[f"model.func.per_type_energy_scale_shift.{k}"].abs().min()) > 0.0


@pytest.mark.gpu
def test_constant_tables_keep_the_module_chain_in_training(device, monkeypatch):
    model, data = _water_model(device, trainable=False)
    model.train()
    fwd, train = _spy(monkeypatch)
    grads = _loss_gradients(model, data)
    assert fwd == [] and train == [] and len(grads) > 6


@pytest.mark.gpu
def test_eval_mode_table_gradients_on_request(device, monkeypatch):
    from nequip_amd.utils.wgrad import eval_parameter_gradients

    model, data = _water_model(device)
    m = model.model.func.eval()  # the energy model inside ForceStressOutput (whose own autograd.grad would consume the graph)
    ss = m.per_type_energy_scale_shift
    fwd, train = _spy(monkeypatch)
    try:
        eval_parameter_gradients(True)
        with torch.enable_grad():
            g = torch.autograd.grad(m(dict(data))["total_energy"].sum(), [ss.scales, ss.shifts])
            assert fwd == [0] and train == [1]
            monkeypatch.setenv("NQA_NO_ENERGY_HEAD", "1")
            ref = torch.autograd.grad(m(dict(data))["total_energy"].sum(), [ss.scales, ss.shifts])
            assert fwd == [0] and train == [1]
    finally:
        eval_parameter_gradients(False)
    for a, r in zip(g, ref):
        assert a is not None and a.shape == r.shape == (2, 1)
        torch.testing.assert_close(a, r, atol=2e-6 * float(r.abs().max()), rtol=0)
    # plain eval mode: the tables are constants of the inference head
    monkeypatch.delenv("NQA_NO_ENERGY_HEAD")
    fwd.clear(), train.clear()
    model.eval()(dict(data))
    assert fwd == [0, 1] and train == []


@pytest.mark.gpu
def test_modified_model_runs_the_head_of_the_new_module(device, monkeypatch):
    """``modify_PerTypeScaleShift`` on a built model: the readout's plan follows the swap (no stale-module error), in eval mode
    on the inference head and in training, with a first layer that has a self-connection (``learnable_shift``)."""
    from nequip_amd.model.modify_utils import modify

    model, data = _water_model(device, trainable=False, learnable_shift=True)
    fwd, train = _spy(monkeypatch)
    e0 = model.eval()(dict(data))["atomic_energy"].detach()
    model = modify(model, [dict(modifier="modify_PerTypeScaleShift", shifts={"O": 3.0}, shifts_trainable=True)]).to(device)
    out = model.eval()(dict(data))
    assert fwd == [0, 1, 0, 1]
    is_o = data["atom_types"].view(-1) == 1
    torch.testing.assert_close(out["atomic_energy"][is_o], e0[is_o] + 1.0, rtol=0, atol=1e-9)
    assert torch.equal(out["atomic_energy"][~is_o], e0[~is_o])
    model.train()
    grads = _loss_gradients(model, data)
    assert sorted(set(train)) == [1, 2]
    assert float(grads["model.func.per_type_energy_scale_shift.shifts"].abs().min()) > 0.0
    assert float(grads["model.func.layer0_convnet.conv.sc.weight"].abs().max()) > 0.0


_CAPTURE = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import torch
from test_energy_head_train import _water_model

device = torch.device("cuda:0")
model, data = _water_model(device)
model.train()

def step():
    model.zero_grad(set_to_none=True)
    out = model(dict(data))
    loss = out["total_energy"].square().sum() + out["forces"].square().sum()
    loss.backward()

side = torch.cuda.Stream(device=device)
side.wait_stream(torch.cuda.current_stream(device))
with torch.cuda.stream(side):
    for _ in range(2):
        step()
torch.cuda.current_stream(device).wait_stream(side)
torch.cuda.synchronize()
ref = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
graph = torch.cuda.CUDAGraph()
model.zero_grad(set_to_none=True)
with torch.cuda.graph(graph):
    step()
for p in model.parameters():
    p.grad.zero_()
graph.replay()
torch.cuda.synchronize()
for k, p in model.named_parameters():
    r = ref[k]
    torch.testing.assert_close(p.grad, r, atol=2e-6 * max(1e-3, float(r.abs().max())), rtol=2e-5, msg=lambda m: f"{k}: {m}")
for k in ("scales", "shifts"):
    g = dict(model.named_parameters())[f"model.func.per_type_energy_scale_shift.{k}"].grad
    assert float(g.abs().min()) > 0.0
print("CAPTURE_OK")
"""


@pytest.mark.gpu
def test_training_step_with_the_head_is_capturable():
    """One training step of the model above in a hipGraph, replayed once: the eager step's gradients (a fresh process, under
    one time limit)."""
    r = subprocess.run([sys.executable, "-c", _CAPTURE, ROOT, os.path.dirname(os.path.abspath(__file__))],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "CAPTURE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
