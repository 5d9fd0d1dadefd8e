"""What the Adam / AdamW tests share: the seeded fixture, the float64 restatement of one step of torch's ``_single_tensor_adam``
with Python doubles for the scalars, and the error bounds.

The fixture is that of ``schedulefree_restatement.py`` (shapes ``()``, ``(1,)``, ``(7,)``, ``(3, 5)``, ``(C,)``, ``(C + 1,)``,
``(2 C + 3,)`` with ``C`` the chunk length of the kernels, once float32 (parameters 0..6) and once float64 (7..13); parameters
N(0, 1), gradients N(0, 1) times a factor per shape between 1 and 1e-3, with exact zeros): its ``(y, g, z, v)`` before step ``k``
give the parameter ``y``, the gradient ``g``, ``exp_avg = z - y`` (0.1 N(0, 1)), ``exp_avg_sq = v`` and ``max_exp_avg_sq = v``
times a seeded factor in [0.5, 1.5) (so that the maximum falls on either side); before step 0 all state is zero, as torch starts.
Parameters with an even index are group A (coupled weight decay 0.1, amsgrad), the odd ones group B (decoupled weight decay 0.05,
``eps=1e-3``, ``betas=(0.95, 0.99)``, ``maximize``): both groups hold both dtypes, a long tensor and short ones.  ``CHECKED`` are
the step counts BEFORE the step.  Always one step at a time from a state that is set: nothing accumulates.

The bounds.  ``u`` is ``2^-24`` / ``2^-53``; scalars are formed in double and rounded once to the tensor's type (1 u each).
``U64 = 2^-53`` whatever the dtype: the device forms ``b**(step+1)`` with its own ``pow``, allowed ``POW_ULPS = 4`` ulp against
Python's.  With ``g`` the gradient after clipping and the sign of ``maximize`` (exact), ``s = step + 1``:

* coupled decay ``g' = g + wd p``: the scalar, the product, the sum: ``d_g = 3 u (|g| + wd |p|) + g_err`` (``g_err``: what a
  clipped gradient carries in, below); otherwise ``d_g = g_err``.  Decoupled decay ``p' = p (1 - lr wd)``: the scalar (two
  operations in double and its rounding), the product: ``d_p0 = (2 u + 2 U64) |p|``; otherwise 0.
* ``m' = lerp(m, g', 1 - b1)``: the difference, the scalar (one operation in double, its rounding), the product, the sum, and
  ``d_g`` carried in with the weight: ``d_m = (4 u + U64) (|m| + |g'|) + (1 - b1) d_g``.
* ``v' = b2 v + (1 - b2) g' g'``: two roundings and a scalar on the first term, three and a scalar on the second, one sum, all
  terms positive: ``6 u v'``; and ``d_g`` carried in: ``d_v = 6 u v' + (1 - b2) (2 |g'| d_g + d_g^2)``.  The maximum of amsgrad
  is exact on its operands: ``max_exp_avg_sq'`` has the same ``d_v``, and so has the value ``x`` under the root.
* ``r = sqrt(x)``: ``|sqrt(x^) - sqrt(x)| = |x^ - x| / (sqrt(x^) + sqrt(x)) <= d_v / sqrt(x)`` (0 where ``d_v`` is 0), the root
  itself 2 u (a few ulp of a device ``sqrt``): ``d_r = d_v / sqrt(x) + 2 u r``.
* ``q = r / sqrt(bc2)``: ``bc2 = 1 - b2**s`` cancels: a relative error ``e`` of the power is ``e b2**s / bc2`` of ``bc2`` and
  half of that in its root; the subtraction, the root and the rounding add ``2 U64 + u``:
  ``e_2 = 0.5 POW_ULPS U64 b2**s / bc2 + 2 U64 + u``; the division 2 u (a device may multiply by the reciprocal):
  ``d_q = d_r / sqrt(bc2) + (e_2 + 2 u) q``.  ``denom = q + eps``: the scalar and the sum: ``d_d = d_q + u eps + u denom``.
* ``t = m' / denom``: ``d_t = (d_m + |t| d_d) / (denom - d_d) + 2 u |t|`` (rigorous in ``d_d``, not first order).
* ``step_size = lr / bc1``, ``bc1 = 1 - b1**s``: ``e_1 = POW_ULPS U64 b1**s / bc1 + 2 U64 + u`` (the power, the subtraction, the
  division, the rounding).  ``p'' = p' - step_size t``: the product and the sum (in either association: ATen's ``addcdiv`` forms
  ``(step_size m') / denom``, the same count): ``d_p = d_p0 + step_size (d_t + (e_1 + u) |t|) + u |p''|``.

A gradient clipped by norm is ``g factor`` with ``factor = min(1, clip / (norm + 1e-6))``: the norm is a sum of ``N`` squares in
double on both sides, each within ``(N + 2) U64 / 2`` after the root, the quotient and the sum 2 U64 more, then the rounding of
the factor and the product: ``g_err = (2 u + (N + 4) U64) |g|`` (0 where the factor is exactly 1: nothing is multiplied).
Clipped by value: the bound is rounded once: ``g_err = u clip`` on the clamped elements.

Float64 results are compared with a restatement that rounds in float64 itself: their bounds are doubled (as the EMA bound is).
``tests/test_adam.py`` checks that six plausible mistakes in the restatement leave these bounds by a factor 10 at least, and that
``torch.optim.Adam`` / ``AdamW`` themselves lie within them.
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import schedulefree_restatement as sr  # noqa: E402

U, U64, POW_ULPS, SLACK = sr.U, sr.U64, sr.POW_ULPS, sr.SLACK
CHECKED = (0, 1, 2, 999)
DEFAULTS = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False, maximize=False,
                decoupled_weight_decay=False)
GROUP_A = dict(DEFAULTS, lr=1e-2, weight_decay=0.1, amsgrad=True)
GROUP_B = dict(DEFAULTS, lr=3e-3, weight_decay=0.05, decoupled_weight_decay=True, eps=1e-3, betas=(0.95, 0.99), maximize=True)
HYPERS = (GROUP_A, GROUP_B)
MUTATIONS = ("bc1_omitted", "eps_inside_sqrt", "decay_after_update", "amsgrad_max_before_update", "step_not_advanced",
             "maximize_ignored")
NAMES = ("p", "exp_avg", "exp_avg_sq", "max_exp_avg_sq")

group_of, order, bits, shapes = sr.group_of, sr.order, sr.bits, sr.shapes


def _f64(t):
    return t.detach().cpu().double()


# ---- the step -------------------------------------------------------------------------------------------------------------------
def restated(p, g, m, v, x, h, step, mutate=None):
    """One step in float64 from the count ``step``: ``(p', m', v', x')`` (``x`` is ``max_exp_avg_sq``; without amsgrad it is
    returned as it came).  ``g`` is the gradient after clipping."""
    p, g, m, v, x = (_f64(t) for t in (p, g, m, v, x))
    lr, (b1, b2), eps, wd = h["lr"], h["betas"], h["eps"], h["weight_decay"]
    if h["maximize"] and mutate != "maximize_ignored":
        g = -g
    s = step if mutate == "step_not_advanced" else step + 1
    late_decay = wd != 0 and h["decoupled_weight_decay"] and mutate == "decay_after_update"
    if wd != 0 and not late_decay:
        if h["decoupled_weight_decay"]:
            p = p * (1.0 - lr * wd)
        else:
            g = g + wd * p
    m1 = m + (g - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * g * g
    if h["amsgrad"]:
        x1 = torch.maximum(x, v if mutate == "amsgrad_max_before_update" else v1)
        root = x1
    else:
        x1, root = x, v1
    bc1 = 1.0 if mutate == "bc1_omitted" or s == 0 else 1.0 - b1 ** s
    bc2 = 1.0 if s == 0 else 1.0 - b2 ** s
    if mutate == "eps_inside_sqrt":
        denom = torch.sqrt(root / bc2 + eps)
    else:
        denom = torch.sqrt(root) / bc2 ** 0.5 + eps
    p1 = p - (lr / bc1) * (m1 / denom)
    if late_decay:
        p1 = p1 * (1.0 - lr * wd)
    return p1, m1, v1, x1


def bounds(dtype, p, g, m, v, x, h, step, g_err=None):
    """``(d_p, d_m, d_v, d_x)``: see the module docstring."""
    p, g, m, v, x = (_f64(t) for t in (p, g, m, v, x))
    u = U[dtype]
    lr, (b1, b2), eps, wd = h["lr"], h["betas"], h["eps"], h["weight_decay"]
    s = step + 1
    if h["maximize"]:
        g = -g
    d_g = torch.zeros_like(g) if g_err is None else _f64(g_err)
    d_p0 = torch.zeros_like(p)
    if wd != 0 and h["decoupled_weight_decay"]:
        d_p0 = (2.0 * u + 2.0 * U64) * p.abs()
        p = p * (1.0 - lr * wd)
    elif wd != 0:
        d_g = 3.0 * u * (g.abs() + wd * p.abs()) + d_g
        g = g + wd * p
    m1 = m + (g - m) * (1.0 - b1)
    v1 = b2 * v + (1.0 - b2) * g * g
    d_m = (4.0 * u + U64) * (m.abs() + g.abs()) + (1.0 - b1) * d_g
    d_v = 6.0 * u * v1 + (1.0 - b2) * (2.0 * g.abs() * d_g + d_g * d_g)
    root = torch.maximum(x, v1) if h["amsgrad"] else v1
    r = torch.sqrt(root)
    d_r = torch.where(d_v > 0, d_v / r.clamp_min(1e-300), torch.zeros_like(r)) + 2.0 * u * r
    bc1, bc2 = 1.0 - b1 ** s, 1.0 - b2 ** s
    e_2 = 0.5 * POW_ULPS * U64 * b2 ** s / bc2 + 2.0 * U64 + u
    e_1 = POW_ULPS * U64 * b1 ** s / bc1 + 2.0 * U64 + u
    q = r / bc2 ** 0.5
    d_q = d_r / bc2 ** 0.5 + (e_2 + 2.0 * u) * q
    denom = q + eps
    d_d = d_q + u * eps + u * denom
    t = (m1 / denom).abs()
    d_t = (d_m + t * d_d) / (denom - d_d) + 2.0 * u * t
    step_size = lr / bc1
    p1 = p - step_size * (m1 / denom)
    d_p = d_p0 + step_size * (d_t + (e_1 + u) * t) + u * p1.abs()
    d_x = d_v if h["amsgrad"] else torch.zeros_like(d_v)
    return tuple(SLACK[dtype] * b for b in (d_p, d_m, d_v, d_x))


def assert_step(after, before, h, step, what="", g=None, g_err=None):
    """``after = (p', m', v', x')`` is one step of ``before = (p, g, m, v, x)`` within the bounds (``g``: the clipped gradient
    to restate with instead, ``g_err`` its error); returns the worst error / bound."""
    dtype = after[0].dtype
    assert all(t is None or t.dtype == dtype for t in after) and after[0].shape == before[0].shape, what
    p, g0, m, v, x = before
    g = g0 if g is None else g
    worst = 0.0
    wants, allowed = restated(p, g, m, v, x, h, step), bounds(dtype, p, g, m, v, x, h, step, g_err)
    for name, got, want, bound in zip(NAMES, after, wants, allowed):
        if got is None:
            assert name == "max_exp_avg_sq" and not h["amsgrad"], what
            continue
        err = (_f64(got) - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert bool((err <= bound).all()), f"{what} {name}: step={step} worst error / bound {ratio:.3f}"
        worst = max(worst, ratio)
    return worst


def norm_clip_error(dtype, g_clipped, factor, n_total):
    """``g_err`` of a gradient clipped by norm (``factor``: the float64 factor; exactly 1 multiplies nothing)."""
    if factor == 1.0:
        return torch.zeros_like(_f64(g_clipped))
    return (2.0 * U[dtype] + (n_total + 4.0) * U64) * _f64(g_clipped).abs()


def value_clip_error(dtype, g, clip):
    """``g_err`` of a gradient clipped by value: the rounded bound, on the clamped elements."""
    return torch.where(_f64(g).abs() >= clip, torch.full_like(_f64(g), U[dtype] * clip), torch.zeros_like(_f64(g)))


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
class Fixture:
    """``before(k)``: the 14 ``(p, g, exp_avg, exp_avg_sq, max_exp_avg_sq)`` before the step from count ``k``, generated once
    per ``k`` and handed out as clones."""

    def __init__(self, chunk, seed=20):
        self.chunk = int(chunk)
        self._inner = sr.Fixture(chunk, seed)
        self._seed = seed
        self._cache = {}

    def before(self, k):
        if k not in self._cache:
            gen = torch.Generator().manual_seed(self._seed * 7919 + k)
            out = []
            for y, g, z, v in self._inner.before(k):
                if k == 0:
                    m, v, x = torch.zeros_like(y), torch.zeros_like(y), torch.zeros_like(y)
                else:
                    m = z - y
                    x = v * (0.5 + torch.rand(y.shape, generator=gen, dtype=y.dtype))
                out.append((y, g, m, v, x))
            self._cache[k] = out
        return [tuple(t.clone() for t in row) for row in self._cache[k]]

    def n_total(self):
        return 2 * sum(int(torch.Size(s).numel()) for s in shapes(self.chunk))


def make_optimizer(params, cls, hypers=HYPERS, **overrides):
    """The two groups over ``params`` (14 tensors in fixture order)."""
    groups = [dict(hypers[gi], params=[p for i, p in enumerate(params) if group_of(i) == gi]) for gi in (0, 1)]
    return cls(groups, **overrides)


def set_state(opt, params, before, k, step_like=None):
    """Puts the optimizer over ``params`` into the state before the step from count ``k`` through ``load_state_dict``; the
    parameters and their ``.grad`` are written in place.  ``step_like(k, p)``: the form the ``step`` values take in the loaded
    dict (default: a 0-d float32 tensor on the parameter's device)."""
    sd = opt.state_dict()
    sd["state"] = {}
    with torch.no_grad():
        for slot, i in enumerate(order()):
            y, g, m, v, x = before[i]
            p = params[i]
            p.copy_(y)
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(g)
            state = {"step": torch.tensor(float(k), device=p.device) if step_like is None else step_like(k, p),
                     "exp_avg": m.clone().to(p.device), "exp_avg_sq": v.clone().to(p.device)}
            if HYPERS[group_of(i)]["amsgrad"]:
                state["max_exp_avg_sq"] = x.clone().to(p.device)
            sd["state"][slot] = state
    opt.load_state_dict(sd)


def state_of(opt, p):
    """``(p, exp_avg, exp_avg_sq, max_exp_avg_sq or None)``"""
    s = opt.state[p]
    return p, s["exp_avg"], s["exp_avg_sq"], s.get("max_exp_avg_sq")
