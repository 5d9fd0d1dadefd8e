"""``nequip_amd.train.ConFIGGradients`` on the multi-tensor HIP kernels (``nqa_config_collect`` / ``nqa_config_gram`` /
``nqa_config_apply``, csrc/config.hip) against the float64 restatement (``tests/config_restatement.py``).

Tolerances: the kernels differ from the ATen Gram form only in the order of the double sums, so the value of a gradient before
its rounding, and ``w``, are held to ten times what ``tests/test_config.py`` recorded for the case class (``GRAM_TOL``: regular
1e-13, dependent 2e-14, zero 5e-15, tiny 5e-11; relative to the largest element of the new gradient), and a written gradient
to one ulp of its dtype on top (rtol 2^-23 for float32).  ``w`` is compared by what it does: ``|dw_l| |g_l| / |new_grad|``."""
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, HERE)
import config_restatement as cr  # noqa: E402
from test_config import GRAM_TOL, P_GPU, assert_grads  # noqa: E402

pytestmark = pytest.mark.gpu
GUARD = 5.0


def _native_launches(monkeypatch):
    """Counts the calls into the library: the tests below are about the kernels, not about the ATen form."""
    from nequip_amd import _lib

    lib, calls = _lib.load(), {"nqa_config_collect": 0, "nqa_config_gram": 0, "nqa_config_apply": 0}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in calls:
                def counted(*a):
                    calls[name] += 1
                    return fn(*a)
                return counted
            return fn

    counting = Counting()
    monkeypatch.setattr(_lib, "load", lambda: counting)
    return calls


class _Synthetic:
    """Parameters of shapes (1,), (3, 5), (c-1,), (c,), (c+1,), (2c+3,), (0,) and a 7-element view that starts at an odd element
    of its storage; ``mixed``: the (c+1,) one is float64.  Their ``.grad``s are views into one flat buffer per dtype, with guard
    elements between them and starts at every residue mod 4 (aligned and misaligned chunks).  Term k is ``sum_i (p_i * g_ki)``:
    its gradient is ``g_k`` exactly."""

    def __init__(self, device, mixed):
        from nequip_amd import _lib

        c = self.chunk = int(_lib.load().nqa_ema_chunk_elems())
        shapes = [(1,), (3, 5), (c - 1,), (c,), (c + 1,), (2 * c + 3,), (0,)]
        dtypes = [torch.float64 if (mixed and s == (c + 1,)) else torch.float32 for s in shapes]
        params = [torch.nn.Parameter(torch.zeros(s, dtype=d, device=device)) for s, d in zip(shapes, dtypes)]
        storage = torch.zeros(16, device=device)
        params.append(torch.nn.Parameter(storage[3:10]))
        assert params[-1].data_ptr() % 16 == 12
        self.model = torch.nn.Module()
        self.model.p = torch.nn.ParameterList(params)
        self.params = params
        self.numel = sum(p.numel() for p in params)
        assert self.numel == P_GPU
        self.flat, self.inside = {}, {}
        cursor = {torch.float32: 0, torch.float64: 0}
        spans = []
        for i, p in enumerate(params):
            start = (cursor[p.dtype] + 3 + 3) // 4 * 4 + (i % 4 if p.dtype == torch.float32 else i % 2)
            spans.append((p.dtype, start, p.numel()))
            cursor[p.dtype] = start + p.numel()
        for dt, n in cursor.items():
            self.flat[dt] = torch.full((n + 8,), GUARD, dtype=dt, device=device)
            self.inside[dt] = torch.zeros(n + 8, dtype=torch.bool, device=device)
        for p, (dt, start, n) in zip(params, spans):
            p.grad = self.flat[dt][start:start + n].view(p.shape)
            p.grad.zero_()
            self.inside[dt][start:start + n] = True
        assert {p.grad.data_ptr() % 16 for p in params if p.dtype == torch.float32 and p.numel()} >= {0, 4, 8, 12}

    def loss_dict(self, rows, names):
        out, start = {n: 0.0 for n in names}, 0
        for p in self.params:
            for k, n in enumerate(names):
                g = rows[k, start:start + p.numel()].view(p.shape).to(device=p.device, dtype=p.dtype)
                out[n] = out[n] + (p * g).sum().double()
            start += p.numel()
        return out

    def guards_intact(self):
        return all(bool((self.flat[dt][~self.inside[dt]] == GUARD).all()) for dt in self.flat)


def _w_error(w, want, rows, new_grad):
    scale = float(new_grad.norm())
    err = float(((w - want).abs() * rows.norm(dim=1)).max())
    return err / scale if scale > 0 else err


def _run_cases(device, mixed, k, monkeypatch, **kw):
    from nequip_amd.train import ConFIGGradients
    from nequip_amd.train.config import gram_weights

    calls = _native_launches(monkeypatch)
    syn = _Synthetic(device, mixed)
    names = [f"t{i}" for i in range(k)]
    coeffs = cr.coefficients(k)
    loss = cr.make_loss(names, coeffs)
    cf = ConFIGGradients(syn.model, loss, **kw)
    pointers = [p.grad.data_ptr() for p in syn.params]
    results, n = [], 0
    for name, cls, rows in cr.cases(k, syn.numel):
        loss_dict = loss(syn.loss_dict(rows, names), {})
        cf.backward(loss_dict)
        n += 1
        assert cf._tables is not None, "the ATen form ran"
        assert [p.grad.data_ptr() for p in syn.params] == pointers and syn.guards_intact(), name
        got_rows = cf.component_gradients()
        assert got_rows.dtype == (torch.float64 if mixed else torch.float32) and got_rows.shape == (k, syn.numel)
        assert torch.equal(got_rows.double().cpu(), rows), f"{name}: the collected rows"
        results.append((name, cls, rows, [p.grad.clone() for p in syn.params], cf.weights.clone().cpu(),
                        cf.grad_norm.clone().cpu()))
    torch.cuda.synchronize()
    assert calls == {"nqa_config_collect": n * (k + 1), "nqa_config_gram": n, "nqa_config_apply": n}
    b = torch.tensor(coeffs, dtype=torch.float64)
    return syn, cf, [(name, cls, rows, grads, w, norm, cr.new_gradient(rows, b), gram_weights(rows @ rows.t(), b, cr.EPS)[0])
                     for name, cls, rows, grads, w, norm in results]


# ---- G1 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mixed", [False, True], ids=["float32", "one_float64"])
@pytest.mark.parametrize("k", cr.KS)
def test_kernels_give_the_restatement(device, mixed, k, monkeypatch):
    _, _, results = _run_cases(device, mixed, k, monkeypatch)
    for name, cls, rows, grads, w, norm, want, want_w in results:
        tol = 10.0 * GRAM_TOL[cls]
        assert not bool(torch.isnan(w).any())
        werr = _w_error(w, want_w, rows, want)
        print(f"K={k} {name}: w error {werr:.2e} (bound {tol:.1e})")
        assert werr <= tol, (name, werr)
        assert_grads(grads, want, tol, f"K={k} {name}")
        assert abs(float(norm) - float(want.norm())) <= tol * max(float(want.norm()), 1e-300), name
        if name == "all_zero":
            assert all(bool((g == 0).all()) for g in grads) and bool((w == 0).all())


# ---- G2 -------------------------------------------------------------------------------------------------------------------------
def test_two_evaluations_are_bit_identical(device, monkeypatch):
    _, _, first = _run_cases(device, True, 8, monkeypatch)
    _, _, second = _run_cases(device, True, 8, monkeypatch)
    for a, b in zip(first, second):
        assert torch.equal(a[4].view(torch.int64), b[4].view(torch.int64)), a[0]
        assert torch.equal(a[5].view(torch.int64), b[5].view(torch.int64)), a[0]
        for x, y in zip(a[3], b[3]):
            assert torch.equal(x, y), a[0]


# ---- G3 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("mixed", [False, True], ids=["float32", "one_float64"])
def test_clipping_is_folded_into_the_kernels(device, algorithm, mixed, monkeypatch):
    """Against ``clip_grad_norm_`` / ``clip_grad_value_`` applied in float64 to the restatement's result (the kernels clip the
    float64 value and round once)."""
    clip = {"norm": 0.25, "value": 0.004}[algorithm]
    _, _, results = _run_cases(device, mixed, 3, monkeypatch, gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    clipped_something = False
    for name, cls, rows, grads, w, norm, want, want_w in results:
        tol = 10.0 * GRAM_TOL[cls]
        assert abs(float(norm) - float(want.norm())) <= tol * max(float(want.norm()), 1e-300), name
        after = cr.clipped(want, algorithm, clip)
        clipped_something = clipped_something or not torch.equal(after, want)
        if algorithm == "value":  # relative to the largest element of the UNCLIPPED gradient: a clamp does not shrink an error
            tol_after = tol * float(want.abs().max()) / max(float(after.abs().max()), 1e-300)
        else:  # the factor scales gradient and error alike
            tol_after = tol
        assert_grads(grads, after, tol_after, f"{algorithm} {name}")
        if algorithm == "norm" and float(want.norm()) > 0:
            factor = min(1.0, clip / (float(want.norm()) + 1e-6))
            assert _w_error(w, want_w * factor, rows, want) <= tol, name
    assert clipped_something


# ---- G4 -------------------------------------------------------------------------------------------------------------------------
_CHILD_HEAD = r"""
import copy
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import torch
import config_restatement as cr
from nequip_amd.train import ConFIGGradients

device = torch.device("cuda:0")


def capture(step, warmup):
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        for _ in range(warmup):
            step()
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    return graph
"""

_MLP_CAPTURE = _CHILD_HEAD + r"""
model = cr.GoldenMLP("mixed").to(device)
loss = cr.make_loss(cr.GOLDEN_NAMES[:2], cr.GOLDEN_COEFFS[2])
gen = torch.Generator().manual_seed(5)
xs = [torch.randn(7, 5, generator=gen).to(device) for _ in range(4)]
ts = [torch.randn(7, 3, generator=gen).to(device) for _ in range(4)]
x, t = xs[0].clone(), ts[0].clone()

# a first call while the stream is capturing: refused, nothing launched
cold = ConFIGGradients(model, loss)
loss_dict = loss(cr.golden_terms(model(x), t, 2), {})
graph = torch.cuda.CUDAGraph()
try:
    with torch.cuda.graph(graph):
        cold.backward(loss_dict)
except RuntimeError as e:
    assert "once eagerly" in str(e), e
else:
    raise SystemExit("a first call under capture did not raise")
torch.cuda.synchronize()
assert all(p.grad is None for p in model.parameters())
del loss_dict, graph

cf = ConFIGGradients(model, loss)
opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)


def make_step(model, cf, opt, x, t):
    def step():
        cf.backward(loss(cr.golden_terms(model(x), t, 2), {}))
        opt.step()
    return step


step = make_step(model, cf, opt, x, t)
graph = capture(step, warmup=1)
pointers = [p.grad.data_ptr() for p in model.parameters()]
twin = copy.deepcopy(model)
twin_opt = torch.optim.Adam(twin.parameters(), lr=1e-2, capturable=True)
twin_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
twin_x, twin_t = x.clone(), t.clone()
twin_step = make_step(twin, ConFIGGradients(twin, loss), twin_opt, twin_x, twin_t)
for r in range(1, 4):
    x.copy_(xs[r]); t.copy_(ts[r]); twin_x.copy_(xs[r]); twin_t.copy_(ts[r])
    before = [p.detach().clone() for p in model.parameters()]
    graph.replay()
    twin_step()
    torch.cuda.synchronize()
    assert any(not torch.equal(a, p) for a, p in zip(before, model.parameters())), "the optimizer did not move the parameters"
    for p, q in zip(model.parameters(), twin.parameters()):
        # the same kernels on the same numbers; rocBLAS may pick its reduction order per call: a few float32 ulps
        torch.testing.assert_close(p.detach(), q.detach(), rtol=1e-5, atol=1e-7)
        torch.testing.assert_close(p.grad, q.grad, rtol=1e-4, atol=1e-6 * float(q.grad.abs().max()))
assert [p.grad.data_ptr() for p in model.parameters()] == pointers
print("CONFIG_CAPTURE_OK")
"""


def _child(script, marker):
    r = subprocess.run([sys.executable, "-c", script, ROOT, HERE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and marker in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_mlp_step_with_config_is_capturable(device):
    """Forward, two backward passes, ConFIG and capturable Adam as one hipGraph, after one eager call; three replays on changing
    inputs against three eager steps from the same start (a fresh process under one time limit, as ``test_ema_gpu.py`` does)."""
    _child(_MLP_CAPTURE, "CONFIG_CAPTURE_OK")


# ---- G5 -------------------------------------------------------------------------------------------------------------------------
def _water(device, seed=8):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=3, seed=seed)
    data = K.to_device(syn.make_data(pos, types, 4.5, cell), device)
    n = len(pos)
    gen = torch.Generator().manual_seed(0)
    target = {"forces": torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device),
              "total_energy": torch.randn(1, 1, generator=gen, dtype=torch.float64).to(device),
              "stress": (torch.randn(1, 3, 3, generator=gen, dtype=torch.float64) * 1e-2).to(device),
              "num_atoms": torch.tensor([n], device=device)}
    return data, target


@pytest.mark.parametrize("k", [2, 3])
def test_in_a_model_rows_are_the_terms_gradients(device, k):
    from nequip_amd.train import ConFIGGradients, EnergyForceLoss, EnergyForceStressLoss
    from test_zbl_gpu import _models

    data, target = _water(device)
    model = _models(device)[1].train()
    loss = EnergyForceLoss() if k == 2 else EnergyForceStressLoss()
    names = [n for n, e in loss.entries.items() if e.coeff is not None]
    assert len(names) == k
    params = [p for p in model.parameters() if p.requires_grad]
    out = dict(model(dict(data)))
    out["num_atoms"] = target["num_atoms"]
    loss_dict = loss(out, target, prefix="train/")
    want_rows = []
    for n in names:
        gs = torch.autograd.grad(loss_dict[f"train/{n}"], params, retain_graph=True, allow_unused=True)
        want_rows.append(torch.cat([(g if g is not None else torch.zeros_like(p)).double().flatten() for g, p in zip(gs, params)]))
    cf = ConFIGGradients(model, loss)
    cf.backward(loss_dict, prefix="train/")
    assert cf._tables is not None, "the ATen form ran"
    rows = cf.component_gradients().double()
    for i, n in enumerate(names):  # (the force kernels use atomics by default: the bars of test_zbl_gpu.py)
        torch.testing.assert_close(rows[i], want_rows[i], atol=1e-5 * float(want_rows[i].abs().max()), rtol=1e-4, msg=lambda s: f"{n}: {s}")
        assert float(want_rows[i].abs().max()) > 0
    coeffs = [loss.entries[n].coeff for n in names]
    want = cr.new_gradient(rows.cpu(), coeffs)
    assert_grads([p.grad.cpu() for p in params], want, 10.0 * GRAM_TOL["regular"], f"model K={k}")


# ---- G6 -------------------------------------------------------------------------------------------------------------------------
_MODEL_CAPTURE = _CHILD_HEAD + r"""
from nequip_amd.train import EnergyForceLoss
from test_config_gpu import _water
from test_zbl_gpu import _models

data, target = _water(device)
model = _models(device)[1].train()
loss = EnergyForceLoss()


def make_step(model, cf, opt):
    def step():
        out = dict(model(dict(data)))
        out["num_atoms"] = target["num_atoms"]
        cf.backward(loss(out, target))
        opt.step()
    return step


opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
graph = capture(make_step(model, ConFIGGradients(model, loss), opt), warmup=2)
twin = copy.deepcopy(model)
twin_opt = torch.optim.Adam(twin.parameters(), lr=1e-2, capturable=True)
twin_opt.load_state_dict(copy.deepcopy(opt.state_dict()))
twin_step = make_step(twin, ConFIGGradients(twin, loss), twin_opt)
start = [p.detach().clone() for p in model.parameters()]
for r in range(2):
    graph.replay()
    twin_step()
torch.cuda.synchronize()
moved = 0
for p, q, s in zip(model.parameters(), twin.parameters(), start):
    moved += int(not torch.equal(p.detach(), s))
    torch.testing.assert_close(p.detach(), q.detach(), atol=1e-5 * float(q.detach().abs().max()), rtol=1e-4)
assert moved > 0, "the optimizer did not move the parameters"
print("CONFIG_MODEL_CAPTURE_OK")
"""


def test_model_step_with_config_is_capturable(device):
    """The water-box model's whole step (forward, two backward passes, ConFIG, capturable Adam) as one hipGraph: two replays
    against two eager steps from the same start, at the first bar of the test above."""
    _child(_MODEL_CAPTURE, "CONFIG_MODEL_CAPTURE_OK")
