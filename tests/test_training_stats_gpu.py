"""``nequip_amd.train.TrainingStatsMonitor`` on the HIP reduction (``nqa_tstats_reduce`` / ``nqa_tstats_advance``,
csrc/training_stats.hip), against the float64 restatement of the same bits (``tests/training_stats_restatement.py``).

Bounds (the worst case of a double accumulation over n elements, with a factor 4 for the merge tree): ``min``, ``max``,
``absmin``, ``absmax`` bit for bit; ``mean`` within ``4 n 2^-52 absmax``; ``std`` and ``rms`` within ``4 n 2^-52`` relative.  For
the rows of ``sqrt(exp_avg_sq)`` one ulp of the device's double-precision ``sqrt`` (specified to 1 ulp) is added: the extrema
within ``2^-52`` relative, the mean within ``(4 n + 1) 2^-52 absmax``."""
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import training_stats_restatement as tr  # noqa: E402

from nequip_amd.train import TrainingStatsMonitor  # noqa: E402

pytestmark = pytest.mark.gpu
NAN, INF = float("nan"), float("inf")
ULP = 2.0 ** -52
EXACT = ("min", "max", "absmin", "absmax")


def _chunk():
    from nequip_amd import _lib

    return int(_lib.load().nqa_tstats_chunk_elems())


def _native_calls(monkeypatch):
    """Counts the calls into the library (a reduce call is two launches, an advance call one)."""
    from nequip_amd import _lib

    lib, calls = _lib.load(), {"nqa_tstats_reduce": 0, "nqa_tstats_advance": 0}

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


def _numels(model):
    return {name: p.numel() for name, p in model.named_parameters()}


def _assert_close(got, want, numel, label=""):
    """Every key of ``want`` against ``got`` within the bounds of the module docstring; returns the worst error / bound."""
    assert list(got) == list(want), label
    worst = 0.0
    for key, w in want.items():
        h = got[key]
        head, name = key.split("/", 1)
        stat = head.rsplit(".", 1)[1]
        n = numel[name]
        root = ".sqrt_exp_avg_sq." in key
        if w != w:
            assert h != h, (label, key, h)
            continue
        if stat in EXACT or (root and stat in ("min", "max")):
            bound = ULP * abs(w) if root else 0.0
        elif stat == "mean":
            section = head.rsplit(".", 1)[0]
            absmax = want[f"{section}.absmax/{name}"] if f"{section}.absmax/{name}" in want else want[f"{section}.max/{name}"]
            bound = (4 * n + (1 if root else 0)) * ULP * absmax
        else:
            bound = 4 * n * ULP * abs(w)
        err = abs(h - w)
        assert err <= bound, (label, key, h, w, err, bound)
        if bound > 0.0:
            worst = max(worst, err / bound)
    return worst


def _module(tensors):
    m = torch.nn.Module()
    m.p = torch.nn.ParameterList([torch.nn.Parameter(t) for t in tensors])
    return m


def _randn(shape, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * 0.5 + 0.1).to(dtype)


# ---- sizes ------------------------------------------------------------------------------------------------------------------
CASES = ["1", "5", "c-1", "c", "c+1", "2c+3", "64x64", "negative", "float64", "view"]


@pytest.mark.parametrize("case", CASES)
def test_one_tensor_against_the_restatement(device, case, monkeypatch):
    c = _chunk()
    shapes = {"1": (1,), "5": (5,), "c-1": (c - 1,), "c": (c,), "c+1": (c + 1,), "2c+3": (2 * c + 3,), "64x64": (64, 64),
              "negative": (c + 5,), "float64": (c + 7,), "view": (c + 2,)}
    x = _randn(shapes[case], seed=CASES.index(case), dtype=torch.float64 if case == "float64" else torch.float32)
    if case == "negative":
        x = -x.abs() - 0.25
    if case == "view":
        buf = torch.zeros(x.numel() + 9, device=device)
        buf[1:1 + x.numel()] = x.to(device)
        x = buf[1:1 + x.numel()]
        assert x.data_ptr() % 16 == 4  # the element-wise path
    model = _module([x.to(device)])
    assert model.p[0].data_ptr() == x.data_ptr() or case != "view"
    model.p[0].grad = (model.p[0].detach() * 3.0).clone()
    calls = _native_calls(monkeypatch)
    mon = TrainingStatsMonitor(log_freq=1)
    mon.on_after_backward(model)
    mon.on_before_optimizer_step(model, [])
    assert calls == {"nqa_tstats_reduce": 2, "nqa_tstats_advance": 1}
    got, want = mon.compute(), tr.expected(model)
    worst = _assert_close(got, want, _numels(model), case)
    print(f"{case}: worst error / bound {worst:.3g}")
    if case == "1":
        assert math.isnan(got["training_stats.weights.std/p.0"])
    if case == "negative":
        assert got["training_stats.weights.max/p.0"] < 0.0 < got["training_stats.weights.absmin/p.0"]
    assert mon.step_count == 1 and mon.logged_step == 0


# ---- conditioning -----------------------------------------------------------------------------------------------------------
def test_std_of_large_values_with_a_small_spread(device):
    """1e6 + 1e-2 randn in float64 (the regime of per-type energy shifts): sequential Welford reaches 3e-9 on such data, the
    sum-of-squares formula 0.12; 1e-6 separates the two with margin on both sides."""
    g = torch.Generator().manual_seed(7)
    x = 1e6 + 1e-2 * torch.randn(5000, generator=g, dtype=torch.float64)
    model = _module([x.to(device)])
    mon = TrainingStatsMonitor(log_freq=1, log_gradients=False, log_optimizer_states=False)
    mon.on_before_optimizer_step(model, [])
    got, want = mon.compute(), tr.expected(model)
    rel = abs(got["training_stats.weights.std/p.0"] - want["training_stats.weights.std/p.0"]) / want["training_stats.weights.std/p.0"]
    print(f"std of 1e6 + 1e-2 randn: relative error {rel:.3g}")
    assert rel <= 1e-6
    assert got["training_stats.weights.min/p.0"] == want["training_stats.weights.min/p.0"]


# ---- non-finite -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["nan", "+inf", "+inf-inf"])
def test_non_finite_elements(device, case):
    c = _chunk()
    xs = [_randn((2 * c + 3,), 1), _randn((c + 1,), 2), _randn((17,), 3)]
    mid = c + c // 2  # in the middle chunk
    if case == "nan":
        xs[0][mid] = NAN
    else:
        xs[0][mid] = INF
        if case == "+inf-inf":
            xs[0][5] = -INF
    model = _module([x.to(device) for x in xs])
    for p in model.parameters():
        p.grad = p.detach().clone()
    mon = TrainingStatsMonitor(log_freq=1)
    mon.on_after_backward(model)
    mon.on_before_optimizer_step(model, [])
    got = mon.compute()
    want = tr.expected(model)
    first = {k: v for k, v in got.items() if k.endswith("/p.0")}
    assert len(first) == 8
    if case == "nan":
        assert all(math.isnan(v) for v in first.values()), first
    else:
        x = xs[0]
        assert first["training_stats.weights.max/p.0"] == INF == first["training_stats.weights.absmax/p.0"]
        assert first["training_stats.weights.min/p.0"] == (-INF if case == "+inf-inf" else float(x.min()))
        assert first["training_stats.weights.absmin/p.0"] == float(x.abs().min())
        assert first["training_stats.gradients.rms/p.0"] == INF == first["training_stats.gradients.absmax/p.0"]
        assert not math.isfinite(first["training_stats.weights.mean/p.0"])
        assert not math.isfinite(first["training_stats.weights.std/p.0"])
        aten = torch.sqrt(torch.mean(model.p[0].detach() ** 2)).item(), model.p[0].detach().abs().min().item()
        assert aten == (first["training_stats.gradients.rms/p.0"], first["training_stats.weights.absmin/p.0"])
    rest = {k: v for k, v in got.items() if not k.endswith("/p.0")}
    _assert_close(rest, {k: v for k, v in want.items() if not k.endswith("/p.0")}, _numels(model), case)


# ---- the sqrt transform -----------------------------------------------------------------------------------------------------
def test_sqrt_of_exp_avg_sq_with_zeros_and_denormals(device):
    c = _chunk()
    model = _module([_randn((c + 3,), 11).to(device), _randn((6,), 12).to(device)])
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    for p in model.parameters():
        p.grad = torch.zeros_like(p)
    opt.step()
    v0 = _randn((c + 3,), 13).square()
    v0[::7] = 0.0
    v0[1::7] = 1e-40  # a float32 denormal
    v0[2] = 1.401298464324817e-45  # the smallest one
    v1 = torch.tensor([0.0, 0.0, 1e-40, 4.0, 2.25, 1e-30])
    for p, v in zip(model.parameters(), (v0, v1)):
        opt.state[p]["exp_avg_sq"].copy_(v.to(device))
        assert torch.equal(opt.state[p]["exp_avg_sq"].cpu(), v)  # (the denormals arrive)
    mon = TrainingStatsMonitor(log_freq=1, log_weights=False, log_gradients=False)
    mon.on_before_optimizer_step(model, [opt])
    got, want = mon.compute(), tr.expected(model, [opt], log_weights=False, log_gradients=False)
    _assert_close(got, want, _numels(model))
    assert got["training_stats.optimizer.sqrt_exp_avg_sq.min/p.0"] == 0.0 == got["training_stats.optimizer.sqrt_exp_avg_sq.min/p.1"]
    assert got["training_stats.optimizer.sqrt_exp_avg_sq.max/p.1"] == 2.0


# ---- a whole module ---------------------------------------------------------------------------------------------------------
class Mixed(torch.nn.Module):
    """6 parameters of mixed float32 / float64; ``forward`` uses all of them."""

    def __init__(self, c):
        super().__init__()
        self.a = torch.nn.Parameter(_randn((c + 9,), 21))
        self.b = torch.nn.Parameter(_randn((33, 7), 22, torch.float64))
        self.c = torch.nn.Parameter(_randn((5,), 23))
        self.d = torch.nn.Parameter(_randn((2 * c + 1,), 24, torch.float64))
        self.e = torch.nn.Parameter(_randn((64, 64), 25))
        self.f = torch.nn.Parameter(_randn((3,), 26, torch.float64))

    def forward(self, s):
        return sum((p.double() * s).square().sum() + (p.double() * (s + 0.5)).sum() for p in self.parameters())


def _train(model, opt, mon, steps, first=0):
    for k in range(first, first + steps):
        opt.zero_grad(set_to_none=True)
        model(1.0 + 0.25 * k).backward()
        mon.on_after_backward(model)
        mon.on_before_optimizer_step(model, [opt])
        opt.step()


def test_whole_module_with_adam_and_launch_counts(device, monkeypatch):
    model = Mixed(_chunk()).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    mon = TrainingStatsMonitor(log_freq=1)
    _train(model, opt, mon, 2)
    calls = _native_calls(monkeypatch)
    opt.zero_grad(set_to_none=True)
    model(2.0).backward()
    mon.on_after_backward(model)
    assert calls == {"nqa_tstats_reduce": 1, "nqa_tstats_advance": 0}  # 2 launches
    mon.on_before_optimizer_step(model, [opt])
    assert calls == {"nqa_tstats_reduce": 2, "nqa_tstats_advance": 1}  # 2 + 1 launches: weights and both moments in one table
    got, want = mon.compute(), tr.expected(model, [opt])
    assert len(want) == 6 * (2 + 6 + 5)
    worst = _assert_close(got, want, _numels(model))
    print(f"whole module: worst error / bound {worst:.3g}")
    assert mon.step_count == 3 and mon.logged_step == 2
    # the CPU ATen form writes the same keys in the same order
    cpu = Mixed(_chunk())
    cpu_opt = torch.optim.Adam(cpu.parameters(), lr=1e-2)
    cpu_mon = TrainingStatsMonitor(log_freq=1)
    _train(cpu, cpu_opt, cpu_mon, 3)
    assert list(cpu_mon.compute()) == list(got)


# ---- gating -----------------------------------------------------------------------------------------------------------------
def test_log_freq_gates_on_the_device(device):
    model = Mixed(_chunk()).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    mon = TrainingStatsMonitor(log_freq=3)
    logged = None
    for step in range(7):
        opt.zero_grad(set_to_none=True)
        model(1.0 + step).backward()
        if step % 3:
            for p in model.parameters():
                p.grad.fill_(NAN)
        want = tr.expected(model, [opt]) if step % 3 == 0 else None
        mon.on_after_backward(model)
        mon.on_before_optimizer_step(model, [opt])
        got = mon.compute()
        if step % 3 == 0:
            _assert_close(got, want, _numels(model), f"step {step}")
            logged = got
            assert mon.logged_step == step
        else:
            # (the Adam state appears after step 0: its rows have no keys until step 3 logs them)
            assert got == logged and mon.logged_step == step - step % 3
            assert not any(v != v for v in got.values())
        assert mon.step_count == step + 1
        if step % 3 == 0:
            opt.step()
    assert any(".optimizer." in k for k in logged)


# ---- capture ----------------------------------------------------------------------------------------------------------------
def _captured_run(device):
    model = Mixed(_chunk()).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    mon = TrainingStatsMonitor(log_freq=2)
    _train(model, opt, mon, 2)
    opt.zero_grad(set_to_none=False)
    model(3.0).backward()
    torch.cuda.synchronize()

    def hooks():
        mon.on_after_backward(model)
        mon.on_before_optimizer_step(model, [opt])

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hooks()
    torch.cuda.synchronize()
    assert mon.step_count == 2, "capturing must not run the hooks"
    wants = []
    for r in range(5):
        with torch.no_grad():
            for i, p in enumerate(model.parameters()):
                p.mul_(1.0 + 0.125 * (r + 1)).add_(0.03125 * i)
                p.grad.copy_(p.detach() * (r - 2.5))
        wants.append(tr.expected(model, [opt]))
        graph.replay()
    torch.cuda.synchronize()
    return mon, model, opt, wants


def test_captured_hooks_log_every_log_freq_replays(device):
    mon, model, opt, wants = _captured_run(device)
    assert mon.step_count == 7 and mon.logged_step == 6  # replays at counts 2 .. 6: 2, 4 and 6 log
    got = mon.compute()
    worst = _assert_close(got, wants[4], _numels(model))
    print(f"captured: worst error / bound {worst:.3g}")
    again = _captured_run(device)[0].compute()
    assert list(again) == list(got) and all(again[k] == got[k] for k in got), "the same inputs give the same bits"
    # a table rebuild during capture raises
    for p in model.parameters():
        p.grad = p.grad.clone()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="once eagerly"):
        with torch.cuda.graph(graph):
            mon.on_after_backward(model)
    torch.cuda.synchronize()
    assert mon.step_count == 7


# ---- in-place rewrite -------------------------------------------------------------------------------------------------------
def test_tables_follow_reallocated_gradients(device):
    model = Mixed(_chunk()).to(device)
    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
    mon = TrainingStatsMonitor(log_freq=1)
    _train(model, opt, mon, 2)
    tables = (mon._gradients.tables, mon._step.tables)
    buffers = [t.tensors.data_ptr() for t in tables] + [t.out.data_ptr() for t in tables]
    keep = [p.grad for p in model.parameters()]  # the old gradients stay alive: the new ones lie elsewhere
    opt.zero_grad(set_to_none=True)
    model(-1.5).backward()
    assert all(p.grad.data_ptr() != k.data_ptr() for p, k in zip(model.parameters(), keep))
    want = tr.expected(model, [opt])
    mon.on_after_backward(model)
    mon.on_before_optimizer_step(model, [opt])
    _assert_close(mon.compute(), want, _numels(model))
    assert (mon._gradients.tables, mon._step.tables) == tables
    assert buffers == [t.tensors.data_ptr() for t in tables] + [t.out.data_ptr() for t in tables]
