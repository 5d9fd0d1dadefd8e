"""``nequip_amd.train.AdamWScheduleFree`` on the CPU (the ATen form of the step) and ``ScheduleFreeHooks``: against the float64
restatement one step at a time (``tests/schedulefree_restatement.py``, which derives the bounds), against ``torch.optim.Adam`` /
``AdamW`` where the method reduces to them, and against the averaging recursion that defines it."""
import copy
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import schedulefree_restatement as sr  # noqa: E402

CHUNK = 1024  # NQA_EMA_CHUNK (the GPU tests check it against the library)
CPU = torch.device("cpu")


@pytest.fixture(scope="module")
def fx():
    return sr.Fixture(CHUNK)


def _params(rows, device=CPU):
    return [torch.nn.Parameter(y.clone().to(device)) for y, _, _, _ in rows]


def _state(opt, p):
    return opt.state[p]["z"], opt.state[p]["exp_avg_sq"]


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_aten_step_is_the_restatement_one_step_at_a_time(fx):
    from nequip_amd.train import AdamWScheduleFree

    params = _params(fx.before(0))
    opt = sr.make_optimizer(params, AdamWScheduleFree)
    worst = 0.0
    for k in sr.CHECKED:
        before = fx.before(k)
        sr.set_state(opt, params, before, k, z_fill=float("nan") if k == 0 else None)
        grads = [p.grad.clone() for p in params]
        opt.step()
        groups = opt.state_dict()["param_groups"]
        for gi in (0, 1):
            want = sr.group_state(gi, k + 1)
            assert {key: groups[gi][key] for key in want} == want
        for i, p in enumerate(params):
            gi = sr.group_of(i)
            worst = max(worst, sr.assert_step((p, *_state(opt, p)), before[i], sr.HYPERS[gi], sr.group_state(gi, k),
                                              f"step {k} parameter {i}"))
            assert torch.equal(sr.bits(p.grad), sr.bits(grads[i])), ".grad must be left untouched"
    print(f"worst error / bound of the ATen form: {worst:.3f}")


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", sr.MUTATIONS)
def test_the_bound_is_not_loose(fx, mutation):
    """Each plausible mistake in the restatement leaves the bound by a factor of 10 at least on some element."""
    worst = 0.0
    for k in sr.CHECKED:
        for i, row in enumerate(fx.before(k)):
            h, st = sr.HYPERS[sr.group_of(i)], sr.group_state(sr.group_of(i), k)
            dtype = row[0].dtype
            for want, wrong, bound in zip(sr.restated(*row, h, st), sr.restated(*row, h, st, mutate=mutation),
                                          sr.bounds(dtype, *row, h, st)):
                ratio = (wrong - want).abs() / bound.clamp_min(1e-300)
                worst = max(worst, float(ratio[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
    print(f"{mutation}: worst error / bound {worst:.3g}")
    assert worst >= 10.0


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def _adam_oracle(fx, device, wd):
    """With ``b1 = 0`` the method is bias-corrected Adam without momentum (``AdamW`` with weight decay): three steps, float64,
    no warm-up, within the float64 bound of a step times the number of steps."""
    from nequip_amd.train import AdamWScheduleFree

    steps, lr, b2, eps = 3, 1e-2, 0.999, 1e-8
    rows = [fx.before(k)[7:] for k in (1, 2, 3)]  # (the float64 half; only y of the first and the gradients are used)
    ours, theirs = _params(rows[0], device), _params(rows[0], device)
    h = dict(sr.DEFAULTS, lr=lr, betas=(0.0, b2), eps=eps, weight_decay=wd)
    opt = AdamWScheduleFree(ours, **h)
    ref = (torch.optim.AdamW(theirs, lr=lr, betas=(0.0, b2), eps=eps, weight_decay=wd) if wd > 0
           else torch.optim.Adam(theirs, lr=lr, betas=(0.0, b2), eps=eps))
    opt.train()
    st = dict(k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
    tol = [torch.zeros_like(p, device=CPU) for p in ours]
    for k in range(steps):
        for i, (p, q) in enumerate(zip(ours, theirs)):
            p.grad = rows[k][i][1].clone().to(device)
            q.grad = rows[k][i][1].clone().to(device)
            z, v = (opt.state[p]["z"], opt.state[p]["exp_avg_sq"]) if opt.state[p] else (p, torch.zeros_like(p))
            tol[i] = torch.maximum(tol[i], sr.bounds(torch.float64, p, p.grad, z, v, h, st)[0])
        opt.step()
        ref.step()
        st = sr.advanced(h, st)
    for i, (p, q) in enumerate(zip(ours, theirs)):
        err = (p.detach() - q.detach()).abs().cpu()
        assert bool((err <= steps * tol[i]).all()), f"parameter {i}: {float((err / (steps * tol[i])).max()):.3f} of the tolerance"
        assert not torch.equal(p.detach().cpu(), rows[0][i][0]) or p.numel() == 0


@pytest.mark.parametrize("wd", [0.0, 0.1])
def test_beta1_zero_is_adam_without_momentum(fx, wd):
    _adam_oracle(fx, CPU, wd)


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def _averaging_oracle(fx, device):
    """Four steps in float64: with ``x_{k+1} = (1 - c_{k+1}) x_k + c_{k+1} z_{k+1}`` run on the recorded ``z``, the train-mode
    parameter is ``(1 - b1) z + b1 x`` and the parameter after ``eval()`` is ``x``.  The tolerance of ``y`` after step ``k`` is
    the sum of the bounds of the steps so far (an error of a step is carried on with a factor below one) and a lerp bound for
    forming the right-hand side; ``x`` is recovered from ``y`` and ``z`` with the factor ``1 / b1``."""
    from nequip_amd.train import AdamWScheduleFree

    steps = 4
    h = dict(sr.GROUP_A)
    b1 = h["betas"][0]
    rows = [fx.before(k)[7:] for k in (1, 2, 3, 1000)]
    params = _params(rows[0], device)
    opt = AdamWScheduleFree(params, **h)
    opt.train()
    st = dict(k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
    x = [p.detach().cpu().double().clone() for p in params]
    tol = [torch.zeros_like(t) for t in x]
    for k in range(steps):
        for i, p in enumerate(params):
            p.grad = rows[k][i][1].clone().to(device)
            tol[i] = tol[i] + sr.bounds(torch.float64, p, p.grad, *_state(opt, p), h, st)[0]
        opt.step()
        c = sr.scalars(h, st)["c"]
        st = sr.advanced(h, st)
        for i, p in enumerate(params):
            z = opt.state[p]["z"].detach().cpu()
            x[i] = (1.0 - c) * x[i] + c * z
            want = (1.0 - b1) * z + b1 * x[i]
            err = (p.detach().cpu() - want).abs()
            allowed = tol[i] + sr.swap_bound(torch.float64, z, x[i], b1)
            assert bool((err <= allowed).all()), f"step {k} parameter {i}: {float((err / allowed).max()):.3f} of the tolerance"
    ys = [p.detach().cpu().clone() for p in params]
    opt.eval()
    w = 1.0 - 1.0 / b1
    for i, p in enumerate(params):
        z = opt.state[p]["z"].detach().cpu()
        err = (p.detach().cpu() - x[i]).abs()
        allowed = (tol[i] + sr.swap_bound(torch.float64, z, x[i], b1)) / b1 + sr.swap_bound(torch.float64, ys[i], z, w)
        assert bool((err <= allowed).all()), f"eval parameter {i}: {float((err / allowed).max()):.3f} of the tolerance"
        assert bool((err < (x[i] - ys[i]).abs()).all() or p.numel() < 2), "x must differ from y for this to say anything"


def test_train_parameter_is_the_interpolation_of_z_and_the_running_average(fx):
    _averaging_oracle(fx, CPU)


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def _mode_switching(fx, device, after_switch=lambda: None):
    from nequip_amd.train import AdamWScheduleFree

    before = fx.before(2)
    params = _params(before, device)
    opt = sr.make_optimizer(params, AdamWScheduleFree)
    sr.set_state(opt, params, before, 2)
    ys = [p.detach().clone() for p in params]
    zs = [opt.state[p]["z"].clone() for p in params]
    versions = [p._version for p in params]
    opt.eval()
    after_switch()
    assert all(not g["train_mode"] for g in opt.param_groups)
    assert all(p._version > v for p, v in zip(params, versions))
    with pytest.raises(RuntimeError, match=r"\.train\(\)"):
        opt.step()
    xs = [p.detach().clone() for p in params]
    for i, (p, y, z) in enumerate(zip(params, ys, zs)):
        w = 1.0 - 1.0 / sr.HYPERS[sr.group_of(i)]["betas"][0]
        want = y.cpu().double() + (z.cpu().double() - y.cpu().double()) * w
        assert bool(((p.detach().cpu().double() - want).abs() <= sr.swap_bound(p.dtype, y, z, w)).all()), f"eval, parameter {i}"
        assert torch.equal(sr.bits(opt.state[p]["z"]), sr.bits(z)), "a mode switch must not write z"
    opt.eval()  # a no-op
    after_switch()
    assert all(torch.equal(sr.bits(p), sr.bits(x)) for p, x in zip(params, xs))
    with opt.averaged_parameters():  # already averaged: nothing on entry, nothing on exit
        assert all(torch.equal(sr.bits(p), sr.bits(x)) for p, x in zip(params, xs))
    assert all(not g["train_mode"] for g in opt.param_groups)
    opt.train()
    after_switch()
    assert all(g["train_mode"] for g in opt.param_groups)
    for i, (p, y, z, x) in enumerate(zip(params, ys, zs, xs)):
        b1 = sr.HYPERS[sr.group_of(i)]["betas"][0]
        allowed = sr.swap_bound(p.dtype, y, z, 1.0 - 1.0 / b1) + sr.swap_bound(p.dtype, x, z, 1.0 - b1)
        assert bool(((p.detach().cpu().double() - y.cpu().double()).abs() <= allowed).all()), f"train, parameter {i}"
    back = [p.detach().clone() for p in params]
    opt.train()  # a no-op
    assert all(torch.equal(sr.bits(p), sr.bits(b)) for p, b in zip(params, back))
    with opt.averaged_parameters():
        assert all(not g["train_mode"] for g in opt.param_groups)
        assert any(not torch.equal(p.detach(), b) for p, b in zip(params, back))
    assert all(g["train_mode"] for g in opt.param_groups)
    opt.step()


def test_mode_switching(fx):
    _mode_switching(fx, CPU)


def test_eval_without_beta1_is_refused_and_bad_hyperparameters_too():
    from nequip_amd.train import AdamWScheduleFree

    p = torch.nn.Parameter(torch.ones(3))
    opt = AdamWScheduleFree([p], betas=(0.0, 0.999))
    opt.train()
    with pytest.raises(ValueError, match="beta1 == 0"):
        opt.eval()
    with pytest.raises(ValueError, match="betas"):
        AdamWScheduleFree([p], betas=(1.0, 0.999))
    with pytest.raises(ValueError, match="lr"):
        AdamWScheduleFree([p], lr=-1.0)


def test_parameters_without_grad_are_skipped(fx):
    from nequip_amd.train import AdamWScheduleFree

    a, b = torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(5))
    opt = AdamWScheduleFree([a, b], lr=1e-2)
    opt.train()
    a.grad = torch.randn(5)
    b0 = b.detach().clone()
    opt.step()
    assert torch.equal(sr.bits(b), sr.bits(b0)) and torch.equal(sr.bits(opt.state[b]["z"]), sr.bits(b0))
    assert not bool(opt.state[b]["exp_avg_sq"].any()) and bool(opt.state[a]["exp_avg_sq"].any())
    assert opt.state_dict()["param_groups"][0]["k"] == 1


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
def _state_dict_round_trip(fx, device):
    from nequip_amd.train import AdamWScheduleFree

    rows = [fx.before(k) for k in (1, 2, 3, 1000)]
    params = _params(rows[0], device)
    opt = sr.make_optimizer(params, AdamWScheduleFree)
    opt.train()
    for k in range(3):
        for p, row in zip(params, rows[k]):
            p.grad = row[1].clone().to(device)
        opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == {"z", "exp_avg_sq"}
    assert {"k", "weight_sum", "lr_max", "scheduled_lr", "train_mode"} <= set(sd["param_groups"][0])
    assert [g["k"] for g in sd["param_groups"]] == [3, 3] and all(g["train_mode"] for g in sd["param_groups"])
    for gi in (0, 1):
        want = sr.group_state(gi, 3)
        assert {key: sd["param_groups"][gi][key] for key in want} == want
    twins = [torch.nn.Parameter(p.detach().clone()) for p in params]
    twin_opt = sr.make_optimizer(twins, AdamWScheduleFree)
    twin_opt.load_state_dict(sd)
    for p, q, row in zip(params, twins, rows[3]):
        p.grad = row[1].clone().to(device)
        q.grad = row[1].clone().to(device)
    opt.step()
    twin_opt.step()
    for p, q in zip(params, twins):
        assert torch.equal(sr.bits(p), sr.bits(q))
        for name in ("z", "exp_avg_sq"):
            assert torch.equal(sr.bits(opt.state[p][name]), sr.bits(twin_opt.state[q][name]))
    assert twin_opt.state_dict()["param_groups"] == opt.state_dict()["param_groups"]


def test_state_dict_round_trip_reproduces_the_next_step_bit_for_bit(fx):
    _state_dict_round_trip(fx, CPU)


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_hooks_switch_modes_and_carry_the_state_through_a_checkpoint():
    from nequip_amd.train import AdamWScheduleFree, ScheduleFreeHooks

    def make_optimizer(m):
        return AdamWScheduleFree(m.parameters(), lr=1e-2, warmup_steps=2)

    torch.manual_seed(0)
    model = torch.nn.Linear(4, 3).double()
    opt, hooks = make_optimizer(model), ScheduleFreeHooks()
    mode = lambda o: [g["train_mode"] for g in o.param_groups]  # noqa: E731
    hooks.on_train_epoch_start(opt)
    assert mode(opt) == [True]
    data = torch.randn(8, 4, dtype=torch.float64)
    for _ in range(3):
        opt.zero_grad()
        model(data).square().sum().backward()
        opt.step()
    y = [p.detach().clone() for p in model.parameters()]
    for hook in (hooks.on_validation_epoch_start, hooks.on_test_epoch_start, hooks.on_predict_epoch_start):
        hook(opt)
        assert mode(opt) == [False]
        x = [p.detach().clone() for p in model.parameters()]
        hooks.on_train_epoch_start(opt)
        assert mode(opt) == [True]
    assert all(not torch.equal(a, b) for a, b in zip(x, y))

    checkpoint = {"state_dict": copy.deepcopy(model.state_dict())}  # saved in train mode: the model holds y
    hooks.on_save_checkpoint(checkpoint, opt)
    assert set(checkpoint) == {"state_dict", "schedulefree_optimizer_state_dict"}
    assert checkpoint["schedulefree_optimizer_state_dict"]["param_groups"][0]["k"] == 3
    hooks.on_save_checkpoint(checkpoint, None)

    fresh, fresh_hooks = torch.nn.Linear(4, 3).double(), ScheduleFreeHooks()
    fresh.load_state_dict(checkpoint["state_dict"])
    fresh_hooks.on_load_checkpoint({})  # a checkpoint without the key stores nothing
    assert fresh_hooks._schedulefree_state_dict == {}
    fresh_hooks.on_load_checkpoint(checkpoint)
    assert fresh_hooks.evaluation_model(fresh, make_optimizer) is fresh
    for p, want in zip(fresh.parameters(), x):  # the averaged weights, formed by the same lerp from the same y and z
        assert torch.equal(sr.bits(p), sr.bits(want))
