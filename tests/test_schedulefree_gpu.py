"""``nequip_amd.train.AdamWScheduleFree`` on the multi-tensor HIP kernels (``nqa_sfree_step`` / ``nqa_sfree_swap``,
csrc/schedulefree.hip): against the float64 restatement one step at a time (``tests/schedulefree_restatement.py`` derives the
bounds), at a misaligned view, next to tensors on the ATen form, under graph capture, and with the modules' weight caches."""
import copy
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, HERE)
import schedulefree_restatement as sr  # noqa: E402
import test_schedulefree as cpu_tests  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    from nequip_amd import _lib

    assert cpu_tests.CHUNK == _lib.load().nqa_ema_chunk_elems()
    return sr.Fixture(cpu_tests.CHUNK)


def _native_launches(monkeypatch):
    """Counts the calls into the library: the tests below are about the kernels, not about the ATen form."""
    from nequip_amd import _lib

    lib, calls = _lib.load(), {"nqa_sfree_step": 0, "nqa_sfree_swap": 0}

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


def _close(got, want):
    """Group state formed with the device's ``pow`` against Python's."""
    return got["k"] == want["k"] and all(
        abs(got[key] - want[key]) <= 2.0 * sr.POW_ULPS * sr.U64 * abs(want[key]) for key in ("weight_sum", "lr_max", "scheduled_lr"))


def _snapshot(opt, params):
    """``(y, g, z, v)`` clones of every parameter (``g`` is ``None`` without ``.grad``)."""
    return [(p.detach().clone(), None if p.grad is None else p.grad.clone(), opt.state[p]["z"].clone(),
             opt.state[p]["exp_avg_sq"].clone()) for p in params]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_kernel_step_is_the_restatement_one_step_at_a_time(device, fx, monkeypatch):
    from nequip_amd.train import AdamWScheduleFree

    calls = _native_launches(monkeypatch)
    params = cpu_tests._params(fx.before(0), device)  # 7 float32 and 7 float64 parameters, two groups, ONE launch per step
    opt = sr.make_optimizer(params, AdamWScheduleFree)
    worst = 0.0
    for k in sr.CHECKED:
        before = fx.before(k)
        sr.set_state(opt, params, before, k, z_fill=NAN if k == 0 else None)
        if k == 0:
            assert all(bool(torch.isnan(opt.state[p]["z"]).all()) for p in params)
        grads = [p.grad.clone() for p in params]
        versions = [p._version for p in params]
        opt.step()
        groups = opt.state_dict()["param_groups"]
        for gi in (0, 1):
            assert _close(groups[gi], sr.group_state(gi, k + 1)), (groups[gi], sr.group_state(gi, k + 1))
        for i, p in enumerate(params):
            gi = sr.group_of(i)
            worst = max(worst, sr.assert_step((p, opt.state[p]["z"], opt.state[p]["exp_avg_sq"]), before[i], sr.HYPERS[gi],
                                              sr.group_state(gi, k), f"step {k} parameter {i}"))
            assert torch.equal(sr.bits(p.grad), sr.bits(grads[i])), ".grad must be left untouched"
            assert p._version > versions[i]
    print(f"worst error / bound of the kernel: {worst:.3f}")
    assert calls == {"nqa_sfree_step": len(sr.CHECKED), "nqa_sfree_swap": 0}


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_mixed_eligibility(device, fx, monkeypatch):
    """One optimizer over a parameter that is a view at an odd element offset (element-wise path of the kernel, guard elements
    around it compared bit for bit), an aligned one, one without ``.grad`` (bit-identical, state untouched) and a
    non-contiguous one (ATen form): two steps, each within the bounds."""
    from nequip_amd.train import AdamWScheduleFree

    calls = _native_launches(monkeypatch)
    chunk = fx.chunk
    gen = torch.Generator().manual_seed(5)
    n = chunk + 5
    flat = torch.randn(n + 16, generator=gen).to(device)
    view = torch.nn.Parameter(flat[5:5 + n])
    aligned = torch.nn.Parameter(torch.randn(2 * chunk + 3, generator=gen).to(device))
    no_grad = torch.nn.Parameter(torch.randn(7, generator=gen).to(device))
    strided = torch.nn.Parameter(torch.randn(6, 5, generator=gen, dtype=torch.float64).to(device).t())
    assert view.data_ptr() % 16 == 4 and not strided.is_contiguous()
    params = [view, aligned, no_grad, strided]
    h = dict(sr.GROUP_A)
    opt = AdamWScheduleFree(params, **h)
    opt.train()
    inside = torch.zeros_like(flat, dtype=torch.bool)
    inside[5:5 + n] = True
    st = dict(k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
    frozen = _snapshot(opt, [no_grad])[0]
    for step in range(2):
        for p in (view, aligned, strided):
            g = torch.randn(p.shape, generator=gen, dtype=p.dtype) * 0.1
            g.view(-1)[0] = 0.0
            p.grad = torch.empty_like(p).copy_(g.to(device))  # (laid out like the parameter)
        assert not strided.grad.is_contiguous()
        before, flat0 = _snapshot(opt, params), flat.clone()
        opt.step()
        assert torch.equal(sr.bits(flat)[~inside], sr.bits(flat0)[~inside]), "written outside the view"
        for i, p in enumerate(params):
            if p is no_grad:
                continue
            sr.assert_step((p, opt.state[p]["z"], opt.state[p]["exp_avg_sq"]), before[i], h, st, f"step {step} parameter {i}")
        st = sr.advanced(h, st)
    for got, want in zip(_snapshot(opt, [no_grad])[0], frozen):
        assert (got is None and want is None) or torch.equal(sr.bits(got), sr.bits(want))
    assert _close(opt.state_dict()["param_groups"][0], st)
    assert calls["nqa_sfree_step"] == 2
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    assert opt.state_dict()["param_groups"][0]["k"] == 2


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_beta1_zero_is_adam_without_momentum(device, fx, wd, monkeypatch):
    calls = _native_launches(monkeypatch)
    cpu_tests._adam_oracle(fx, device, wd)
    assert calls["nqa_sfree_step"] == 3


def test_train_parameter_is_the_interpolation_of_z_and_the_running_average(device, fx, monkeypatch):
    calls = _native_launches(monkeypatch)
    cpu_tests._averaging_oracle(fx, device)
    assert calls == {"nqa_sfree_step": 4, "nqa_sfree_swap": 2}  # (train() of the initial state and eval())


def test_state_dict_round_trip_reproduces_the_next_step_bit_for_bit(device, fx, monkeypatch):
    calls = _native_launches(monkeypatch)
    cpu_tests._state_dict_round_trip(fx, device)
    assert calls["nqa_sfree_step"] == 5


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_mode_switching_on_the_swap_kernels(device, fx, monkeypatch):
    from nequip_amd.train import AdamWScheduleFree

    calls = _native_launches(monkeypatch)
    cpu_tests._mode_switching(fx, device, after_switch=torch.cuda.synchronize)
    assert calls == {"nqa_sfree_step": 1, "nqa_sfree_swap": 4}  # (eval, train, and the two of the context manager)

    p = torch.nn.Parameter(torch.randn(9).to(device))
    opt = AdamWScheduleFree([p])
    opt.train()
    p.grad = torch.randn(9).to(device)
    opt.step()
    for switch in (opt.eval, opt.train):
        if switch == opt.train:
            opt.eval()
        graph = torch.cuda.CUDAGraph()
        with pytest.raises(RuntimeError, match="cannot be captured"):
            with torch.cuda.graph(graph):
                switch()
        torch.cuda.synchronize()


def test_stepped_and_averaged_weights_reach_the_cached_weight_images(device, monkeypatch):
    """The modules keep derived weight images keyed on ``(data_ptr, _version)``; the kernels write through raw pointers.  A
    model with filled caches must evaluate with the stepped weights after ``step()`` and with the averaged ones after
    ``eval()``: this fails without the version bumps."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.train import AdamWScheduleFree
    from nequip_amd.utils import synthetic as syn
    from test_zbl_gpu import _models

    calls = _native_launches(monkeypatch)
    pos, types, cell, names = syn.water_box(n_side=3, seed=8)
    data = K.to_device(syn.make_data(pos, types, 4.5, cell), device)
    model = _models(device)[1].eval()
    twins = [copy.deepcopy(model), copy.deepcopy(model)]  # never evaluated before they get their weights: nothing cached

    def evaluate(m):
        out = m(dict(data))
        return out[K.TOTAL_ENERGY_KEY].detach().clone(), out[K.FORCE_KEY].detach().clone()

    def twin_of(m, twin):
        with torch.no_grad():
            for q, p in zip(twin.parameters(), m.parameters()):
                q.copy_(p)
        return evaluate(twin)

    opt = AdamWScheduleFree(model.parameters(), lr=2e-2)
    opt.train()
    e_raw, f_raw = evaluate(model)  # fills the caches with the images of the initial weights
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(device)
        opt.step()
    e_step, f_step = evaluate(model)
    e_twin, f_twin = twin_of(model, twins[0])
    assert not torch.equal(e_raw, e_twin), "the step must move the weights for this test to say anything"
    assert torch.equal(e_step, e_twin) and torch.equal(f_step, f_twin)
    opt.eval()
    e_avg, f_avg = evaluate(model)
    e_twin, f_twin = twin_of(model, twins[1])
    assert not torch.equal(e_avg, e_step), "the averaged weights must differ from the stepped ones"
    assert torch.equal(e_avg, e_twin) and torch.equal(f_avg, f_twin)
    assert calls == {"nqa_sfree_step": 2, "nqa_sfree_swap": 2}  # (train() of the initial state and eval())


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def _captured_run(device):
    """An MLP step (forward, backward, ``step()``) captured after one eager step and replayed on changing inputs; every replay
    is compared with the restatement of ONE step from the state before it.  Returns the final bits."""
    from nequip_amd.train import AdamWScheduleFree

    torch.manual_seed(7)
    model = torch.nn.Sequential(torch.nn.Linear(8, 33), torch.nn.Tanh(), torch.nn.Linear(33, 1)).to(device)
    params = list(model.parameters())
    h = dict(sr.DEFAULTS, lr=1e-2, weight_decay=0.1, warmup_steps=5)
    opt = AdamWScheduleFree(params, **h)
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(64, 8, generator=gen).to(device)
    target = torch.randn(64, 1, generator=gen).to(device)

    def step():
        opt.zero_grad(set_to_none=False)
        (model(x) - target).square().mean().backward()
        opt.step()

    opt.train()  # (state and tables exist now, without gradients)
    for p in params:
        p.grad = torch.zeros_like(p)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="once eagerly"):  # the tables do not know these gradients: a rebuild under capture
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    assert opt.state_dict()["param_groups"][0]["k"] == 0

    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        step()  # eagerly: k = 1, the gradient buffers exist from here on
    torch.cuda.current_stream(device).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    st = sr.advanced(h, dict(k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0))
    assert _close(opt.state_dict()["param_groups"][0], st), "capturing must not run the step"

    def replay_and_check(what):
        nonlocal st
        x.copy_(torch.randn(64, 8, generator=gen))
        before = _snapshot(opt, params)
        graph.replay()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            y, _, z, v = before[i]
            assert not torch.equal(p.detach(), y), "the replay did not move the parameters"
            sr.assert_step((p, opt.state[p]["z"], opt.state[p]["exp_avg_sq"]), (y, p.grad, z, v), h, st, f"{what} parameter {i}")
        st = sr.advanced(h, st)

    for r in range(3):  # k = 1, 2, 3: the warm-up factor 2/5, 3/5, 4/5 is formed on the device
        replay_and_check(f"replay {r}")
    assert opt.state_dict()["param_groups"][0]["k"] == 1 + 3
    assert _close(opt.state_dict()["param_groups"][0], st)

    # a changed learning rate: refused under capture, written in place by an eager step, and then read by the OLD graph
    opt.param_groups[0]["lr"] = h["lr"] = 5e-3
    other = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="once eagerly"):
        with torch.cuda.graph(other):
            opt.step()
    torch.cuda.synchronize()
    before = _snapshot(opt, params)
    opt.step()
    for i, p in enumerate(params):
        sr.assert_step((p, opt.state[p]["z"], opt.state[p]["exp_avg_sq"]), before[i], h, st, f"eager step parameter {i}")
    st = sr.advanced(h, st)
    replay_and_check("replay with the new lr")
    assert opt.state_dict()["param_groups"][0]["k"] == 6
    return [sr.bits(t).cpu() for p in params for t in (p, opt.state[p]["z"], opt.state[p]["exp_avg_sq"])]


def test_captured_step_advances_k_and_the_warm_up_on_every_replay(device):
    first = _captured_run(device)
    second = _captured_run(device)
    assert all(torch.equal(a, b) for a, b in zip(first, second)), "two identical runs must give identical bits"


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
_TRAIN_CAPTURE = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import torch
import schedulefree_restatement as sr
from nequip_amd.data import AtomicDataDict as K
from nequip_amd.train import AdamWScheduleFree, EnergyForceLoss
from nequip_amd.utils import synthetic as syn
from test_zbl_gpu import _models

device = torch.device("cuda:0")
pos, types, cell, names = syn.water_box(n_side=3, seed=8)
data = K.to_device(syn.make_data(pos, types, 4.5, cell), device)
n = len(pos)
model = _models(device)[1].train()
gen = torch.Generator().manual_seed(0)
target = {"forces": torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device),
          "total_energy": torch.randn(1, 1, generator=gen, dtype=torch.float64).to(device),
          "num_atoms": torch.tensor([n], device=device)}
loss_fn = EnergyForceLoss()
h = dict(sr.DEFAULTS, lr=1e-2, weight_decay=0.01, warmup_steps=10)
params = list(model.parameters())
opt = AdamWScheduleFree(params, **h)
opt.train()

def step():
    opt.zero_grad(set_to_none=False)
    out = dict(model(dict(data)))
    out["num_atoms"] = target["num_atoms"]
    loss_fn(out, target)["weighted_sum"].backward()
    opt.step()

side = torch.cuda.Stream(device=device)
side.wait_stream(torch.cuda.current_stream(device))
with torch.cuda.stream(side):
    for _ in range(2):
        step()
torch.cuda.current_stream(device).wait_stream(side)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
with torch.cuda.graph(graph):
    step()
torch.cuda.synchronize()
st = dict(k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
for _ in range(2):
    st = sr.advanced(h, st)
assert opt.state_dict()["param_groups"][0]["k"] == 2
stepped = [p for p in params if p.grad is not None]
assert stepped
for r in range(2):
    before = [(p.detach().clone(), opt.state[p]["z"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in stepped]
    graph.replay()
    torch.cuda.synchronize()
    worst = 0.0
    assert any(not torch.equal(p.detach(), b[0]) for p, b in zip(stepped, before)), "the optimizer did not move the parameters"
    for i, (p, (y, z, v)) in enumerate(zip(stepped, before)):
        worst = max(worst, sr.assert_step((p, opt.state[p]["z"], opt.state[p]["exp_avg_sq"]), (y, p.grad, z, v), h, st,
                                          f"replay {r} parameter {i}"))
    st = sr.advanced(h, st)
    print(f"replay {r}: worst error / bound {worst:.3f}")
assert opt.state_dict()["param_groups"][0]["k"] == 4
ys = [p.detach().clone() for p in params]
opt.eval()
out = model(dict(data))
assert bool(torch.isfinite(out[K.TOTAL_ENERGY_KEY]).all()) and bool(torch.isfinite(out[K.FORCE_KEY]).all())
xs = [p.detach().clone() for p in params]
assert any(not torch.equal(x, y) for x, y in zip(xs, ys))
opt.train()
b1 = h["betas"][0]
for p, x, y in zip(params, xs, ys):
    z = opt.state[p]["z"]
    allowed = sr.swap_bound(p.dtype, y, z, 1.0 - 1.0 / b1) + sr.swap_bound(p.dtype, x, z, 1.0 - b1)
    assert bool(((p.detach().cpu().double() - y.cpu().double()).abs() <= allowed).all())
print("SFREE_CAPTURE_OK")
"""


def test_training_step_with_schedulefree_is_capturable(device):
    """Forward, double backward, ``EnergyForceLoss`` and ``AdamWScheduleFree`` in one hipGraph, replayed twice and compared
    with the restatement each time; then ``eval()``, one evaluation and ``train()`` (a fresh process under one time limit, as
    ``test_ema_gpu.py`` does for its captured step)."""
    r = subprocess.run([sys.executable, "-c", _TRAIN_CAPTURE, ROOT, HERE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "SFREE_CAPTURE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
