"""``nequip_amd.train.Adam`` / ``AdamW`` / ``ReduceLROnPlateau`` on the multi-tensor HIP kernels (``nqa_adam_step`` /
``nqa_adam_grad_norm`` / ``nqa_adam_plateau``, csrc/adam.hip): against the float64 restatement one step at a time
(``tests/adam_restatement.py`` derives the bounds), at a misaligned view, next to tensors on the ATen form, with clipping by norm,
under graph capture together with the scheduler, and with the modules' weight caches."""
import copy
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adam_restatement as ar  # noqa: E402
import test_adam as cpu_tests  # noqa: E402

pytestmark = pytest.mark.gpu
NAMES = ("nqa_adam_step", "nqa_adam_grad_norm", "nqa_adam_plateau")


@pytest.fixture(scope="module")
def fx():
    from nequip_amd import _lib

    assert cpu_tests.CHUNK == _lib.load().nqa_ema_chunk_elems()
    return ar.Fixture(cpu_tests.CHUNK)


def _native_launches(monkeypatch):
    """Counts the calls into the library: the tests below are about the kernels, not about the ATen form."""
    from nequip_amd import _lib

    lib, calls = _lib.load(), {name: 0 for name in NAMES}

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


def _snapshot(opt, params):
    """``(p, g, exp_avg, exp_avg_sq, max_exp_avg_sq, step)`` clones of every parameter (``g`` is ``None`` without ``.grad``,
    ``max_exp_avg_sq`` zeros without amsgrad)."""
    def get(p, name):  # (before the first step there is no state: torch's initial one, zeros)
        return opt.state[p].get(name, torch.zeros((), device=p.device) if name == "step" else torch.zeros_like(p)).clone()

    return [(p.detach().clone(), None if p.grad is None else p.grad.clone(), get(p, "exp_avg"), get(p, "exp_avg_sq"),
             get(p, "max_exp_avg_sq"), get(p, "step")) for p in params]


def _all_bits(opt, params):
    return [ar.bits(t).cpu() for p in params for t in (p, *opt.state[p].values())]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_kernel_step_is_the_restatement_one_step_at_a_time(device, fx, monkeypatch):
    from nequip_amd.train import Adam

    calls = _native_launches(monkeypatch)
    # 7 float32 and 7 float64 parameters, two groups, ONE launch per step
    worst, opt, params = cpu_tests._steps_are_the_restatement(fx, device, lambda ps: ar.make_optimizer(ps, Adam))
    print(f"worst error / bound of the kernel: {worst:.3f}")
    assert calls == {"nqa_adam_step": len(ar.CHECKED), "nqa_adam_grad_norm": 0, "nqa_adam_plateau": 0}
    for p in params:
        step = opt.state[p]["step"]
        assert step.dtype == torch.float32 and step.dim() == 0 and step.device == p.device


def test_state_dicts_are_exchanged_with_torch_in_both_directions(device, fx, monkeypatch):
    calls = _native_launches(monkeypatch)
    cpu_tests._interchange(fx, device)
    assert calls["nqa_adam_step"] == 2


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_mixed_eligibility(device, fx, monkeypatch):
    """One optimizer over a parameter that is a view at an odd element offset (element-wise path of the kernel, guard elements
    around it compared bit for bit), an aligned one across two chunk boundaries, one without ``.grad`` (bit-identical, state and
    ``step`` untouched) and a non-contiguous float64 one (ATen form): two steps, each within the bounds."""
    from nequip_amd.train import Adam

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
    h = dict(ar.GROUP_A)
    opt = Adam(params, **h)
    inside = torch.zeros_like(flat, dtype=torch.bool)
    inside[5:5 + n] = True
    frozen = None
    for step in range(2):
        for p in (view, aligned, strided):
            g = torch.randn(p.shape, generator=gen, dtype=p.dtype) * 0.1
            g.view(-1)[0] = 0.0
            p.grad = torch.empty_like(p).copy_(g.to(device))  # (laid out like the parameter)
        assert not strided.grad.is_contiguous()
        if step == 0:
            opt.step()  # (builds the state)
            frozen = _snapshot(opt, [no_grad])[0]
        before, flat0 = _snapshot(opt, params), flat.clone()
        opt.step()
        assert torch.equal(ar.bits(flat)[~inside], ar.bits(flat0)[~inside]), "written outside the view"
        for i, p in enumerate(params):
            if p is no_grad:
                continue
            count = float(before[i][5])
            assert count == step + 1 and float(opt.state[p]["step"]) == count + 1
            ar.assert_step(ar.state_of(opt, p), before[i][:5], h, int(count), f"step {step} parameter {i}")
    for got, want in zip(_snapshot(opt, [no_grad])[0], frozen):
        assert (got is None and want is None) or torch.equal(ar.bits(got), ar.bits(want))
    assert float(opt.state[no_grad]["step"]) == 0
    assert calls["nqa_adam_step"] == 3
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            opt.step()
    torch.cuda.synchronize()
    assert float(opt.state[view]["step"]) == 3


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def test_clipping_by_norm_on_the_kernels(device, fx, monkeypatch):
    """``opt.grad_norm`` against a float64 sum on the CPU.  The kernels add ``N`` squares (one rounding each) in a fixed order:
    a lane at most 16 elements of its chunk in sequence, 6 levels of the wavefront's tree, then a lane of the second kernel its
    run of ``ceil(chunks / 64)`` partials and lane 0 the 64 lane sums: no term passes through more than
    ``DEPTH = 16 + 6 + ceil(chunks / 64) + 64`` additions, so the sum is within ``(DEPTH + 1) U64`` relative, the root halves
    that and adds a rounding of its own; the reference (``math.fsum`` of the rounded squares, one root) is within ``2 U64``."""
    calls = _native_launches(monkeypatch)
    norm, got, again = cpu_tests._clip_by_norm(fx, device)  # (clipped, then a norm below the clip value and no clipping)
    chunks = sum(-(-int(torch.Size(s).numel()) // fx.chunk) for s in ar.shapes(fx.chunk)) * 2
    depth = 16 + 6 + -(-chunks // 64) + 64
    assert abs(got - norm) <= ((depth + 1) / 2.0 + 1.0 + 2.0) * ar.U64 * norm, (got, norm)
    assert got == again, "the same gradients must give the same bits of the norm"
    assert calls == {"nqa_adam_step": 3, "nqa_adam_grad_norm": 2, "nqa_adam_plateau": 0}
    # two runs from the same state are bit-identical
    runs = []
    for _ in range(2):
        _, params, opt = cpu_tests._clipped_step(fx, device, 2, gradient_clip_val=0.5 * norm)
        runs.append(_all_bits(opt, params) + [ar.bits(opt.grad_norm.reshape(1)).cpu()])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_nan_gradient_under_clipping_on_the_kernels(device, monkeypatch):
    calls = _native_launches(monkeypatch)
    cpu_tests._nan_gradient(device)
    assert calls == {"nqa_adam_step": 2, "nqa_adam_grad_norm": 1, "nqa_adam_plateau": 0}


def test_clipping_by_value_on_the_kernels(device, fx, monkeypatch):
    calls = _native_launches(monkeypatch)
    k, clip = 1, 0.05
    grads = [row[1] for row in fx.before(k)]
    twins = cpu_tests._f64_twins(grads)
    torch.nn.utils.clip_grad_value_(twins, clip)
    before, params, opt = cpu_tests._clipped_step(fx, device, k, gradient_clip_val=clip, gradient_clip_algorithm="value")
    for i, p in enumerate(params):
        ar.assert_step(ar.state_of(opt, p), before[i], ar.HYPERS[ar.group_of(i)], k, f"clipped by value, {i}", g=twins[i].grad,
                       g_err=ar.value_clip_error(p.dtype, grads[i], clip))
    assert calls == {"nqa_adam_step": 1, "nqa_adam_grad_norm": 0, "nqa_adam_plateau": 0}


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_captured_step_equals_eager_steps_bit_for_bit(device, fx, monkeypatch):
    """One eager step, then ``step()`` captured: three replays with new gradient values written into the same ``.grad`` buffers
    equal three eager steps of a twin optimizer bit for bit, and the ``step`` tensors read 4 afterwards (with clipping by norm:
    the four launches of a step are in the graph)."""
    from nequip_amd.train import Adam

    calls = _native_launches(monkeypatch)
    rows = [fx.before(k) for k in (1, 2, 999, 0)]
    norm = math.sqrt(sum(float(r[1].double().square().sum()) for r in rows[1]))
    captured, twin = cpu_tests._params(rows[0], device), cpu_tests._params(rows[0], device)
    opts = [ar.make_optimizer(ps, Adam, gradient_clip_val=0.5 * norm) for ps in (captured, twin)]

    fresh = ar.make_optimizer(cpu_tests._params(rows[0], device), Adam)
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="once eagerly"):  # nothing was built: a build under capture
        with torch.cuda.graph(graph):
            fresh.step()
    torch.cuda.synchronize()

    def set_grads(params, k):
        for p, row in zip(params, rows[k]):
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(row[1])

    for params, opt in zip((captured, twin), opts):
        set_grads(params, 0)
        opt.step()
    torch.cuda.synchronize()
    launches = dict(calls)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        opts[0].step()
    torch.cuda.synchronize()
    assert {k: calls[k] - launches[k] for k in calls} == {"nqa_adam_step": 1, "nqa_adam_grad_norm": 1, "nqa_adam_plateau": 0}
    assert all(float(opts[0].state[p]["step"]) == 1 for p in captured), "capturing must not run the step"
    for r in range(3):
        set_grads(captured, r + 1)
        set_grads(twin, r + 1)
        graph.replay()
        opts[1].step()
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(_all_bits(opts[0], captured), _all_bits(opts[1], twin))), f"replay {r}"
        assert torch.equal(ar.bits(opts[0].grad_norm.reshape(1)), ar.bits(opts[1].grad_norm.reshape(1)))
    assert all(float(opts[0].state[p]["step"]) == 4 for p in captured)
    assert any(not torch.equal(p.detach().cpu(), row[0]) for p, row in zip(captured, rows[0]))


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def _build_tables(opt):
    """One eager step with zero gradients: the device tables exist afterwards (``lr`` plays no part)."""
    for group in opt.param_groups:
        for p in group["params"]:
            p.grad = torch.zeros_like(p)
    opt.step()
    assert opt._tables is not None


def test_reduce_lr_on_plateau_on_the_device_follows_torchs_rules(device, monkeypatch):
    calls = _native_launches(monkeypatch)
    cpu_tests._plateau_rules(device, cpu_tests.PLATEAU_CASES, prepare=_build_tables,
                             as_metric=lambda x: torch.tensor(x, dtype=torch.float64, device=device))
    assert calls["nqa_adam_plateau"] == len(cpu_tests.PLATEAU_CASES) * len(cpu_tests.METRICS)
    cpu_tests._plateau_rules(device, cpu_tests.PLATEAU_CASES[:4], prepare=_build_tables,
                             as_metric=lambda x: torch.tensor(x, dtype=torch.float32, device=device))
    # a float and a CPU tensor are copied into the scheduler's own buffer: the same kernel
    before = calls["nqa_adam_plateau"]
    cpu_tests._plateau_rules(device, cpu_tests.PLATEAU_CASES[:2], prepare=_build_tables)
    cpu_tests._plateau_rules(device, cpu_tests.PLATEAU_CASES[:2], prepare=_build_tables, as_metric=lambda x: torch.tensor(x))
    assert calls["nqa_adam_plateau"] - before == 4 * len(cpu_tests.METRICS)


def test_scheduler_captured_with_the_step_reduces_the_lr_the_next_replay_uses(device, monkeypatch):
    """``opt.step(); sched.step(metric)`` in one graph, the metric rewritten in place between replays: the replay after the
    patience runs out steps with the reduced ``lr`` (checked through the restatement with that ``lr``), a following eager
    ``step()`` does not restore the old one, and a host assignment reaches the device at the next eager step."""
    from nequip_amd.train import Adam, ReduceLROnPlateau

    calls = _native_launches(monkeypatch)
    gen = torch.Generator().manual_seed(17)
    params = [torch.nn.Parameter(torch.randn(1500, generator=gen).to(device)),
              torch.nn.Parameter(torch.randn(33, generator=gen, dtype=torch.float64).to(device))]
    h = dict(ar.DEFAULTS, lr=1e-2, weight_decay=0.01)
    opt = Adam(params, **h)
    sched = ReduceLROnPlateau(opt, factor=0.5, patience=1)  # (before the tables exist: its record follows them)
    metric = torch.ones((), dtype=torch.float64, device=device)

    def new_grads():
        for p in params:
            g = torch.randn(p.shape, generator=gen, dtype=p.dtype).to(device)
            if p.grad is None:
                p.grad = g
            else:
                p.grad.copy_(g)

    def checked(run, lr, count, what):
        new_grads()
        before = _snapshot(opt, params)
        run()
        torch.cuda.synchronize()
        for i, p in enumerate(params):
            assert float(before[i][5]) == count and float(opt.state[p]["step"]) == count + 1
            ar.assert_step(ar.state_of(opt, p), before[i][:5], dict(h, lr=lr), count, f"{what} parameter {i}")

    checked(opt.step, 1e-2, 0, "eager step")
    graph = torch.cuda.CUDAGraph()
    new_grads()
    with torch.cuda.graph(graph):
        opt.step()
        sched.step(metric)
    torch.cuda.synchronize()
    assert calls["nqa_adam_plateau"] == 1 and sched.state_dict()["last_epoch"] == 0, "capturing must not run the scheduler"
    # metric 1.0: best; 1.0: one bad epoch; 1.0: two bad epochs > patience: lr = 5e-3 AFTER the step of that replay
    for r, lr in enumerate((1e-2, 1e-2, 1e-2, 5e-3)):
        metric.fill_(1.0)
        checked(graph.replay, lr, 1 + r, f"replay {r}")
    assert opt.param_groups[0]["lr"] == 1e-2  # (the host has not looked yet)
    checked(opt.step, 5e-3, 5, "eager step after the reduction")  # ... and an eager step does not restore it
    assert sched.get_last_lr() == [5e-3] and opt.param_groups[0]["lr"] == 5e-3
    state = sched.state_dict()
    assert (state["last_epoch"], state["best"], state["num_bad_epochs"]) == (4, 1.0, 1)
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            sched.step(0.5)
    torch.cuda.synchronize()
    # a host assignment: refused under capture, written by the next eager step, and then read by the OLD graph
    opt.param_groups[0]["lr"] = 2e-3
    with pytest.raises(RuntimeError, match="once eagerly"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            opt.step()
    torch.cuda.synchronize()
    checked(opt.step, 2e-3, 6, "eager step with the assigned lr")
    metric.fill_(0.5)
    checked(graph.replay, 2e-3, 7, "replay with the assigned lr")
    assert sched.get_last_lr() == [2e-3] and sched.state_dict()["best"] == 0.5


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
def test_stepped_weights_reach_the_cached_weight_images(device, monkeypatch):
    """The modules keep derived weight images keyed on ``(data_ptr, _version)``; the kernels write through raw pointers.  A
    model with filled caches must evaluate with the stepped weights after ``step()``: this fails without the version bumps."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.train import Adam
    from nequip_amd.utils import synthetic as syn
    from test_zbl_gpu import _models

    calls = _native_launches(monkeypatch)
    pos, types, cell, names = syn.water_box(n_side=3, seed=8)
    data = K.to_device(syn.make_data(pos, types, 4.5, cell), device)
    model = _models(device)[1].eval()
    twin = copy.deepcopy(model)  # never evaluated before it gets its weights: nothing cached

    def evaluate(m):
        out = m(dict(data))
        return out[K.TOTAL_ENERGY_KEY].detach().clone(), out[K.FORCE_KEY].detach().clone()

    opt = Adam(model.parameters(), lr=2e-2)
    e_raw, f_raw = evaluate(model)  # fills the caches with the images of the initial weights
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=g).to(device)
        opt.step()
    e_step, f_step = evaluate(model)
    with torch.no_grad():
        for q, p in zip(twin.parameters(), model.parameters()):
            q.copy_(p)
    e_twin, f_twin = evaluate(twin)
    assert not torch.equal(e_raw, e_twin), "the step must move the weights for this test to say anything"
    assert torch.equal(e_step, e_twin) and torch.equal(f_step, f_twin)
    assert calls["nqa_adam_step"] == 2


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_training_stats_monitor_logs_the_moments_of_this_optimizer(device):
    from nequip_amd.train import Adam, TrainingStatsMonitor

    torch.manual_seed(2)
    model = torch.nn.Sequential(torch.nn.Linear(5, 9), torch.nn.Tanh(), torch.nn.Linear(9, 1)).to(device)
    opt = Adam(model.parameters(), lr=1e-2)
    monitor = TrainingStatsMonitor(log_freq=1, log_optimizer_states=True)
    x = torch.randn(16, 5, device=device)
    for _ in range(2):
        opt.zero_grad(set_to_none=False)
        model(x).square().mean().backward()
        monitor.on_after_backward(model)
        monitor.on_before_optimizer_step(model, opt)
        opt.step()
    keys = list(monitor.compute())
    for name, _ in model.named_parameters():
        assert any("optimizer.exp_avg." in k and k.endswith("/" + name) for k in keys), (name, keys[:8])
        assert any("optimizer.sqrt_exp_avg_sq." in k and k.endswith("/" + name) for k in keys), name
