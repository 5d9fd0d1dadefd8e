"""``nequip_amd.train.Adam`` / ``AdamW`` / ``ReduceLROnPlateau`` on the CPU (the ATen form of the step, the host rules of the
scheduler): against the float64 restatement one step at a time (``tests/adam_restatement.py``, which derives the bounds), against
``torch.optim.Adam`` / ``AdamW`` and ``torch.optim.lr_scheduler.ReduceLROnPlateau`` themselves, and state dicts exchanged with them
in both directions."""
import copy
import itertools
import math
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import adam_restatement as ar  # noqa: E402

CHUNK = 1024  # NQA_EMA_CHUNK (the GPU tests check it against the library)
CPU = torch.device("cpu")
NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    return ar.Fixture(CHUNK)


def _params(rows, device=CPU):
    return [torch.nn.Parameter(row[0].clone().to(device)) for row in rows]


def _torch_pair(params):
    """``torch.optim.Adam`` over group A and ``torch.optim.AdamW`` over group B, in their single-tensor form."""
    a = {k: v for k, v in ar.GROUP_A.items() if k != "decoupled_weight_decay"}
    b = {k: v for k, v in ar.GROUP_B.items() if k != "decoupled_weight_decay"}
    return (torch.optim.Adam([p for i, p in enumerate(params) if ar.group_of(i) == 0], foreach=False, **a),
            torch.optim.AdamW([p for i, p in enumerate(params) if ar.group_of(i) == 1], foreach=False, **b))


def _torch_groups(params):
    """One ``torch.optim.Adam`` with both groups (``decoupled_weight_decay`` per group), single-tensor form."""
    return ar.make_optimizer(params, torch.optim.Adam, foreach=False)


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def _steps_are_the_restatement(fx, device, opt_of, step_like=None):
    """Every checked step of every parameter within the bounds; returns the worst error / bound."""
    params = _params(fx.before(0), device)
    opt = opt_of(params)
    worst = 0.0
    for k in ar.CHECKED:
        before = fx.before(k)
        ar.set_state(opt, params, before, k, step_like)
        grads = [p.grad.clone() for p in params]
        versions = [p._version for p in params]
        opt.step()
        for i, p in enumerate(params):
            worst = max(worst, ar.assert_step(ar.state_of(opt, p), before[i], ar.HYPERS[ar.group_of(i)], k,
                                              f"step {k} parameter {i}"))
            assert torch.equal(ar.bits(p.grad), ar.bits(grads[i])), ".grad must be left untouched"
            assert p._version > versions[i]
            step = opt.state[p]["step"]
            assert float(step) == k + 1, (float(step), k)
    return worst, opt, params


def test_aten_step_is_the_restatement_one_step_at_a_time(fx):
    from nequip_amd.train import Adam

    worst, opt, params = _steps_are_the_restatement(fx, CPU, lambda ps: ar.make_optimizer(ps, Adam))
    print(f"worst error / bound of the ATen form: {worst:.3f}")
    for p in params:
        step = opt.state[p]["step"]
        assert step.dtype == torch.float32 and step.dim() == 0 and step.device == p.device


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def test_torch_adam_and_adamw_lie_within_the_same_bounds(fx):
    """The bounds against the reference alone: ``torch.optim.Adam`` / ``AdamW`` (``foreach=False``), one step from the same state."""
    worst = 0.0
    for k in ar.CHECKED:
        before = fx.before(k)
        params = _params(before)
        for gi, opt in enumerate(_torch_pair(params)):
            ids = [i for i in range(14) if ar.group_of(i) == gi]
            sd = opt.state_dict()
            for slot, i in enumerate(ids):
                y, g, m, v, x = before[i]
                params[i].grad = g.clone()
                sd["state"][slot] = {"step": torch.tensor(float(k)), "exp_avg": m.clone(), "exp_avg_sq": v.clone()}
                if ar.HYPERS[gi]["amsgrad"]:
                    sd["state"][slot]["max_exp_avg_sq"] = x.clone()
            opt.load_state_dict(sd)
            opt.step()
            for i in ids:
                worst = max(worst, ar.assert_step(ar.state_of(opt, params[i]), before[i], ar.HYPERS[gi], k,
                                                  f"torch, step {k} parameter {i}"))
                assert float(opt.state[params[i]]["step"]) == k + 1
    print(f"worst error / bound of torch.optim.Adam / AdamW: {worst:.3f}")


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ar.MUTATIONS)
def test_the_bound_is_not_loose(fx, mutation):
    """Each plausible mistake in the restatement leaves the bound by a factor of 10 at least on some element."""
    worst = 0.0
    for k in ar.CHECKED:
        for i, row in enumerate(fx.before(k)):
            h, dtype = ar.HYPERS[ar.group_of(i)], row[0].dtype
            for want, wrong, bound in zip(ar.restated(*row, h, k), ar.restated(*row, h, k, mutate=mutation),
                                          ar.bounds(dtype, *row, h, k)):
                ratio = (wrong - want).abs() / bound.clamp_min(1e-300)
                worst = max(worst, float(ratio[bound > 0].max()) if bool((bound > 0).any()) else 0.0)
    print(f"{mutation}: worst error / bound {worst:.3g}")
    assert worst >= 10.0


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def _interchange(fx, device):
    """A state dict of ours loads into ``torch.optim.Adam`` and one of torch's (host-side ``step`` values) loads here: the
    ``step`` values, the moments and the amsgrad maxima arrive bit for bit, and the next step of the receiver is within the
    bounds."""
    from nequip_amd.train import Adam

    k = 2
    before, after = fx.before(k), fx.before(999)
    ours = _params(before, device)
    opt = ar.make_optimizer(ours, Adam)
    ar.set_state(opt, ours, before, k)
    opt.step()
    sd = copy.deepcopy(opt.state_dict())
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq", "max_exp_avg_sq"}  # (group A: amsgrad)
    assert set(sd["state"][7]) == {"step", "exp_avg", "exp_avg_sq"}
    assert all(float(s["step"]) == k + 1 for s in sd["state"].values())

    # ours -> torch
    theirs = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    ref = _torch_groups(theirs)
    ref.load_state_dict(copy.deepcopy(sd))
    assert [g["lr"] for g in ref.param_groups] == [h["lr"] for h in ar.HYPERS]
    assert [g["decoupled_weight_decay"] for g in ref.param_groups] == [False, True]
    for p, q in zip(ours, theirs):
        for name, t in opt.state[p].items():
            got = ref.state[q][name]
            assert float(got) == k + 1 if name == "step" else torch.equal(ar.bits(got), ar.bits(t)), name
    snapshot = [(q.detach().clone(), None, *(ref.state[q][n].clone() for n in ("exp_avg", "exp_avg_sq")),
                 ref.state[q].get("max_exp_avg_sq", torch.zeros_like(q)).clone()) for q in theirs]
    for i, q in enumerate(theirs):
        q.grad = after[i][1].clone().to(device)
    ref.step()
    for i, q in enumerate(theirs):
        y, _, m, v, x = snapshot[i]
        ar.assert_step(ar.state_of(ref, q), (y, q.grad, m, v, x), ar.HYPERS[ar.group_of(i)], k + 1, f"torch after ours, {i}")
        assert float(ref.state[q]["step"]) == k + 2

    # torch -> ours: torch's default form keeps `step` as float32 tensors on the CPU; numbers are taken too
    sd_ref = copy.deepcopy(ref.state_dict())
    sd_ref["state"][3]["step"] = float(sd_ref["state"][3]["step"])
    back = [torch.nn.Parameter(q.detach().clone()) for q in theirs]
    opt2 = ar.make_optimizer(back, Adam)
    opt2.load_state_dict(sd_ref)
    assert "foreach" not in opt2.param_groups[0]
    for q, p in zip(theirs, back):
        step = opt2.state[p]["step"]
        assert step.dtype == torch.float32 and step.dim() == 0 and step.device == p.device and float(step) == k + 2
        for name in ("exp_avg", "exp_avg_sq", "max_exp_avg_sq"):
            assert (name in opt2.state[p]) == (name in ref.state[q])
            if name in ref.state[q]:
                assert torch.equal(ar.bits(opt2.state[p][name]), ar.bits(ref.state[q][name]))
    snapshot = [(p.detach().clone(), None, *(t.clone() for t in ar.state_of(opt2, p)[1:3]),
                 opt2.state[p].get("max_exp_avg_sq", torch.zeros_like(p)).clone()) for p in back]
    for i, p in enumerate(back):
        p.grad = before[i][1].clone().to(device)
    opt2.step()
    for i, p in enumerate(back):
        y, _, m, v, x = snapshot[i]
        ar.assert_step(ar.state_of(opt2, p), (y, p.grad, m, v, x), ar.HYPERS[ar.group_of(i)], k + 2, f"ours after torch, {i}")
        assert float(opt2.state[p]["step"]) == k + 3


def test_state_dicts_are_exchanged_with_torch_in_both_directions(fx):
    _interchange(fx, CPU)


def test_load_state_dict_keeps_the_state_tensors(fx):
    from nequip_amd.train import Adam

    before = fx.before(2)
    params = _params(before)
    opt = ar.make_optimizer(params, Adam)
    ar.set_state(opt, params, before, 2)
    opt.step()
    ptrs = [[t.data_ptr() for t in opt.state[p].values()] for p in params]
    ar.set_state(opt, params, fx.before(999), 999)
    assert ptrs == [[t.data_ptr() for t in opt.state[p].values()] for p in params]
    assert all(float(opt.state[p]["step"]) == 999 for p in params)


def test_parameters_without_grad_are_skipped_and_do_not_count():
    from nequip_amd.train import Adam

    a, b = torch.nn.Parameter(torch.randn(5)), torch.nn.Parameter(torch.randn(5))
    opt = Adam([a, b], lr=1e-2, amsgrad=True)
    a.grad = torch.randn(5)
    b0 = b.detach().clone()
    opt.step()
    assert torch.equal(ar.bits(b), ar.bits(b0)) and not bool(opt.state[b]["exp_avg_sq"].any())
    assert float(opt.state[a]["step"]) == 1 and float(opt.state[b]["step"]) == 0
    assert bool(opt.state[a]["exp_avg_sq"].any())


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def _f64_twins(grads):
    twins = [torch.nn.Parameter(torch.zeros(g.shape, dtype=torch.float64)) for g in grads]
    for t, g in zip(twins, grads):
        t.grad = g.detach().cpu().double().clone()
    return twins


def _clipped_step(fx, device, k, **clip):
    from nequip_amd.train import Adam

    before = fx.before(k)
    params = _params(before, device)
    opt = ar.make_optimizer(params, Adam, **clip)
    ar.set_state(opt, params, before, k)
    grads = [p.grad.clone() for p in params]
    opt.step()
    for p, g in zip(params, grads):
        assert torch.equal(ar.bits(p.grad), ar.bits(g)), ".grad must be left untouched"
    return before, params, opt


def _clip_by_norm(fx, device):
    k = 2
    grads = [row[1] for row in fx.before(k)]
    norm = math.sqrt(math.fsum(float(x) ** 2 for g in grads for x in g.double().reshape(-1).tolist()))
    # clipping: against clip_grad_norm_ applied in float64 before the restatement
    clip = 0.5 * norm
    twins = _f64_twins(grads)
    total = torch.nn.utils.clip_grad_norm_(twins, clip)
    factor = min(1.0, clip / (float(total) + 1e-6))
    assert factor < 0.6
    before, params, opt = _clipped_step(fx, device, k, gradient_clip_val=clip)
    assert opt.gradient_clip_algorithm == "norm"
    got = opt.grad_norm
    assert got.dtype == torch.float64 and got.dim() == 0 and got.device.type == device.type
    for i, p in enumerate(params):
        g_err = ar.norm_clip_error(p.dtype, twins[i].grad, factor, fx.n_total())
        ar.assert_step(ar.state_of(opt, p), before[i], ar.HYPERS[ar.group_of(i)], k, f"clipped by norm, {i}", g=twins[i].grad,
                       g_err=g_err)
    # a norm below the clip value: the bits of no clipping
    _, loose, loose_opt = _clipped_step(fx, device, k, gradient_clip_val=2.0 * norm)
    _, plain, plain_opt = _clipped_step(fx, device, k)
    assert plain_opt.grad_norm is None
    for p, q in zip(loose, plain):
        for a, b in zip(ar.state_of(loose_opt, p), ar.state_of(plain_opt, q)):
            assert (a is None and b is None) or torch.equal(ar.bits(a), ar.bits(b))
    return norm, float(got), float(loose_opt.grad_norm)


def test_clipping_by_norm_is_clip_grad_norm_before_the_step(fx):
    norm, got, again = _clip_by_norm(fx, CPU)
    assert abs(got - norm) <= (fx.n_total() + 2) * ar.U64 * norm and got == again


def test_clipping_by_value_is_clip_grad_value_before_the_step(fx):
    k, clip = 1, 0.05
    grads = [row[1] for row in fx.before(k)]
    twins = _f64_twins(grads)
    torch.nn.utils.clip_grad_value_(twins, clip)
    assert any(not torch.equal(t.grad, g.double()) for t, g in zip(twins, grads))
    before, params, opt = _clipped_step(fx, CPU, k, gradient_clip_val=clip, gradient_clip_algorithm="value")
    for i, p in enumerate(params):
        ar.assert_step(ar.state_of(opt, p), before[i], ar.HYPERS[ar.group_of(i)], k, f"clipped by value, {i}", g=twins[i].grad,
                       g_err=ar.value_clip_error(p.dtype, grads[i], clip))


def _nan_gradient(device):
    """A NaN in one gradient: by norm every stepped parameter becomes NaN, as after ``clip_grad_norm_(error_if_nonfinite=False)``
    (whose factor is NaN); by value the NaN passes the clamp and reaches its own element only."""
    from nequip_amd.train import Adam

    out = {}
    for algorithm in ("norm", "value"):
        torch.manual_seed(3)
        params = [torch.nn.Parameter(torch.randn(9).to(device)), torch.nn.Parameter(torch.randn(4, dtype=torch.float64).to(device)),
                  torch.nn.Parameter(torch.randn(3).to(device))]
        opt = Adam(params, lr=1e-2, gradient_clip_val=0.1, gradient_clip_algorithm=algorithm)
        for p in params[:2]:
            p.grad = torch.randn(p.shape, dtype=p.dtype).to(device)
        with torch.no_grad():
            params[0].grad[4] = NAN
        grads = [p.grad.clone() for p in params[:2]]
        kept = params[2].detach().clone()
        opt.step()
        for p, g in zip(params, grads):
            assert torch.equal(ar.bits(p.grad), ar.bits(g))
        assert torch.equal(ar.bits(params[2]), ar.bits(kept))
        out[algorithm] = [p.detach().cpu() for p in params[:2]], opt
    by_norm, opt = out["norm"]
    twins = _f64_twins(grads)
    total = torch.nn.utils.clip_grad_norm_(twins, 0.1, error_if_nonfinite=False)
    assert math.isnan(float(total)) and all(bool(t.grad.isnan().all()) for t in twins)
    assert math.isnan(float(opt.grad_norm)) and all(bool(p.isnan().all()) for p in by_norm)
    by_value, _ = out["value"]
    assert bool(by_value[0].isnan()[4]) and int(by_value[0].isnan().sum()) == 1 and not bool(by_value[1].isnan().any())


def test_nan_gradient_under_clipping():
    _nan_gradient(CPU)


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
METRICS = [1.0, 0.9, 0.9, 0.95, NAN, 0.9, 0.8999, 0.5, 0.6, 0.6, 0.6, 0.497, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.6, 0.4,
           0.6, 0.6, 0.6]
PLATEAU_CASES = [dict(mode=mode, threshold_mode=tm, patience=patience, cooldown=cooldown, **rest)
                 for mode, tm, patience, cooldown, rest in itertools.product(
                     ("min", "max"), ("rel", "abs"), (0, 2), (0, 2),
                     (dict(min_lr=0.0, eps=5e-4),  # the second reduction of group B (2.7e-4) is smaller than eps
                      dict(min_lr=[2e-3, 1e-6], eps=1e-8)))]


def _metric(case, value):
    return value if case["mode"] == "min" else 1.0 - value  # (a maximised quantity that plateaus where the other does)


def _plateau_rules(device, cases, prepare=lambda opt: None, as_metric=lambda x: x):
    """After every call the ``lr`` of every group equals torch's ``ReduceLROnPlateau`` on a ``torch.optim.Adam``, compared with
    ``==``; so do the keys and values of ``state_dict()``."""
    from nequip_amd.train import Adam, ReduceLROnPlateau

    for case in cases:
        mine = [torch.nn.Parameter(torch.ones(3).to(device)), torch.nn.Parameter(torch.ones(2).to(device))]
        ref = [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2))]
        opt = Adam([dict(params=mine[:1], lr=1e-2), dict(params=mine[1:], lr=3e-3)])
        ref_opt = torch.optim.Adam([dict(params=ref[:1], lr=1e-2), dict(params=ref[1:], lr=3e-3)])
        prepare(opt)
        kw = dict(case, factor=0.1, threshold=0.01)
        sched, ref_sched = ReduceLROnPlateau(opt, **kw), torch.optim.lr_scheduler.ReduceLROnPlateau(ref_opt, **kw)
        for n, value in enumerate(METRICS):
            metric = as_metric(_metric(case, value))
            sched.step(metric)
            ref_sched.step(float(metric))
            want = [g["lr"] for g in ref_opt.param_groups]
            assert sched.get_last_lr() == want == [g["lr"] for g in opt.param_groups], (case, n)
        assert ref_opt.param_groups[0]["lr"] < 1e-2, case  # the sequence does reduce
        got, want = sched.state_dict(), ref_sched.state_dict()
        assert set(got) == set(want), case
        assert got == want, (case, got, want)
        if case["eps"] == 5e-4:  # group A was reduced twice, group B once: its second reduction is smaller than eps
            assert [g["lr"] for g in opt.param_groups] == [1e-2 * 0.1 * 0.1, 3e-3 * 0.1], case


def test_reduce_lr_on_plateau_host_rules_are_torchs():
    _plateau_rules(CPU, PLATEAU_CASES)
    _plateau_rules(CPU, PLATEAU_CASES[:2], as_metric=lambda x: torch.tensor(x))


def test_reduce_lr_on_plateau_state_dict_round_trip():
    from nequip_amd.train import Adam, ReduceLROnPlateau

    p = torch.nn.Parameter(torch.ones(3))
    opt, ref_opt = Adam([p], lr=1e-2), torch.optim.Adam([torch.nn.Parameter(torch.ones(3))], lr=1e-2)
    ref = torch.optim.lr_scheduler.ReduceLROnPlateau(ref_opt, patience=1, cooldown=1, factor=0.5)
    for value in METRICS[:6]:
        ref.step(value)
    sched = ReduceLROnPlateau(opt, patience=7)
    sched.load_state_dict(ref.state_dict())
    opt.param_groups[0]["lr"] = ref_opt.param_groups[0]["lr"]
    for value in METRICS[6:]:
        sched.step(value)
        ref.step(value)
        assert opt.param_groups[0]["lr"] == ref_opt.param_groups[0]["lr"]
    assert sched.state_dict() == ref.state_dict()


# ---- 7 ----------------------------------------------------------------------------------------------------------------------
def test_argument_validation():
    from nequip_amd.train import Adam, AdamW, ReduceLROnPlateau

    p = torch.nn.Parameter(torch.ones(3))
    for bad in (dict(lr=-1.0), dict(betas=(1.0, 0.999)), dict(betas=(0.9, -0.1)), dict(eps=-1.0), dict(weight_decay=-1.0),
                dict(gradient_clip_val=-1.0), dict(gradient_clip_val=1.0, gradient_clip_algorithm="both")):
        with pytest.raises(ValueError):
            Adam([p], **bad)
    for unknown in ("fused", "foreach", "capturable", "differentiable"):
        with pytest.raises(TypeError):
            Adam([p], **{unknown: True})
        with pytest.raises(ValueError, match="unknown"):
            Adam([{"params": [p], unknown: True}])
    with pytest.raises(TypeError):
        AdamW([p], decoupled_weight_decay=False)
    with pytest.raises(ValueError, match="complex"):
        Adam([torch.nn.Parameter(torch.ones(3, dtype=torch.complex64))])
    assert AdamW([p]).param_groups[0]["weight_decay"] == 1e-2 and AdamW([p]).param_groups[0]["decoupled_weight_decay"] is True
    assert Adam([p], gradient_clip_algorithm="value").gradient_clip_algorithm is None  # (no value: no clipping)
    sparse = torch.nn.Parameter(torch.ones(4, 2))
    sparse.grad = torch.sparse_coo_tensor(torch.tensor([[0], [1]]), torch.tensor([1.0]), (4, 2))
    with pytest.raises(RuntimeError, match="sparse"):
        Adam([sparse]).step()
    opt = Adam([p])
    with pytest.raises(ValueError, match="Factor"):
        ReduceLROnPlateau(opt, factor=1.0)
    with pytest.raises(TypeError):
        ReduceLROnPlateau(p)
    with pytest.raises(ValueError, match="mode"):
        ReduceLROnPlateau(opt, mode="best")
    with pytest.raises(ValueError, match="threshold mode"):
        ReduceLROnPlateau(opt, threshold_mode="both")
    with pytest.raises(ValueError, match="min_lrs"):
        ReduceLROnPlateau(opt, min_lr=[0.0, 0.0])


# ---- 8 ----------------------------------------------------------------------------------------------------------------------
def test_adam_symbols_are_exported_and_declared():
    """The entry points are declared in the header, bound in ``_lib`` and exported by the built library."""
    from nequip_amd import _lib

    names = ("nqa_adam_step", "nqa_adam_grad_norm", "nqa_adam_plateau")
    header = open(os.path.join(HERE, "..", "include", "nequip_amd.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES, name
        assert f" {name}(" in header, name
    for record in ("nqa_adam_tensor", "nqa_adam_group", "nqa_adam_clip", "nqa_adam_plateau_state"):
        assert f"}} {record};" in header, record
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
    assert "adam.hip" in open(os.path.join(HERE, "..", "nequip_amd", "csrc", "build.py")).read()
