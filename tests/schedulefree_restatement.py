"""What the schedule-free AdamW tests share: the seeded fixture, the float64 restatement of one step with Python doubles for the
scalars, and the error bounds.

The parameter list is that of the EMA tests: shapes ``()``, ``(1,)``, ``(7,)``, ``(3, 5)``, ``(C,)``, ``(C + 1,)``, ``(2 C + 3,)``
with ``C`` the chunk length of the kernels, once in float32 (parameters 0..6) and once in float64 (7..13).  Parameters with an
even index are group A (``lr=1e-2, wd=0.1, warmup_steps=3``), the odd ones group B (``lr=3e-3, wd=0, eps=1e-3, r=0.5,
weight_lr_power=1, betas=(0.95, 0.99)``): both groups hold both dtypes, a long tensor and short ones.  Parameters are N(0, 1);
gradients N(0, 1) times a factor per shape between 1 and 1e-3, with exact zeros; before step ``k > 0`` ``z`` is the parameter
plus 0.1 N(0, 1) and ``exp_avg_sq`` a squared gradient-like value, before step 0 ``exp_avg_sq`` is zero and ``z`` is whatever
the test puts there (the step reads the parameter instead).  The group state before step ``k`` is the scalar recursion run
from 0.  Always one step at a time from a state that is set: nothing accumulates.

The bounds.  ``u`` is ``2^-24`` / ``2^-53``; scalars are formed in double and rounded once to the tensor's type (1 u each).
``U64 = 2^-53`` whatever the dtype: the device forms ``b2**(k+1)``, ``(k+1)**r`` and ``lr_max**weight_lr_power`` with its own
``pow``, allowed ``POW_ULPS = 4`` ulp against Python's.

* ``v' = b2 v + (1-b2) g g``: two roundings and a scalar on the first term, three and a scalar on the second, one sum, all
  terms positive: ``6 u v'``.
* ``root = sqrt(v'/bc2)``: 6 u from ``v'``, the scalar, the division (2 u: a device may multiply by the reciprocal), halved by
  the root to 4.5 u, the root itself 2 u (a few ulp of device ``sqrt``): 6.5 u.  ``bc2 = 1 - b2**(k+1)`` cancels: a relative
  error ``e`` of the power is ``e b2**(k+1)/bc2`` of ``bc2`` and half of that in the root: ``e_bc2 = 0.5 POW_ULPS U64
  b2**(k+1)/bc2``.  ``denom = root + eps``: the scalar and the sum, 2 u more; ``g/denom`` 2 u more; the sum with ``wd y`` (a
  scalar, a product: 2 u of its own) 1 u more:  ``d_gn = (12 u + e_bc2) |g|/denom + 3 u wd |y|``.
* ``c = weight/weight_sum`` carries two powers, a product, a sum and a quotient: relative ``e_c = (2 POW_ULPS + 2) U64``.
  ``lerp(y, z, c)``: the difference, the scalar, the product, the sum: ``4 u (|y| + |z|)``, and ``e_c c (|y| + |z|)``.
  ``a = lr_k (b1 (1-c) - 1)``: absolute error ``lr_k b1 c e_c + 3 U64 |a|`` in double; then its rounding, the product with
  ``gn`` and the final sum: ``by = 4 u S + e_c c S + |a| d_gn + (3 (u + U64) |a| + lr_k b1 c e_c) G``, ``S = |y| + |z|``,
  ``G = |g|/denom + wd |y|``.
* ``z' = z - lr_k gn``: ``bz = u |z| + 3 u lr_k G + lr_k d_gn`` (``lr_k`` itself is the same IEEE operations on both sides).

Float64 results are compared with a restatement that rounds in float64 itself: their bounds are doubled (as the EMA bound is).
``tests/test_schedulefree.py`` checks that six plausible mistakes in the restatement leave these bounds by a factor 10 at least.
"""
import torch

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
U64 = 2.0 ** -53
POW_ULPS = 4.0
SLACK = {torch.float32: 1.0, torch.float64: 2.0}
CHECKED = (0, 1, 2, 3, 1000)
SCALES = (1.0, 0.3, 0.1, 0.03, 0.01, 0.003, 0.001)
DEFAULTS = dict(lr=0.0025, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, warmup_steps=0, r=0.0, weight_lr_power=2.0)
GROUP_A = dict(DEFAULTS, lr=1e-2, weight_decay=0.1, warmup_steps=3)
GROUP_B = dict(DEFAULTS, lr=3e-3, weight_decay=0.0, eps=1e-3, r=0.5, weight_lr_power=1.0, betas=(0.95, 0.99))
HYPERS = (GROUP_A, GROUP_B)
MUTATIONS = ("c_from_old_weight_sum", "no_bias_correction", "k_in_warmup", "wd_times_z", "eps_inside_sqrt", "lr_in_z_update")


def shapes(chunk):
    return [(), (1,), (7,), (3, 5), (chunk,), (chunk + 1,), (2 * chunk + 3,)]


def group_of(i):
    return i % 2


def order():
    """Parameter indices in state-dict order: group A's, then group B's."""
    return [i for i in range(14) if group_of(i) == 0] + [i for i in range(14) if group_of(i) == 1]


# ---- scalars ------------------------------------------------------------------------------------------------------------------
def scalars(h, st, mutate=None):
    """The scalars of the step that follows the group state ``st``, in Python doubles."""
    k, warmup = st["k"], h["warmup_steps"]
    b1, b2 = h["betas"]
    if mutate == "k_in_warmup":
        sched = k / warmup if k < warmup else 1.0
    else:
        sched = (k + 1) / warmup if k < warmup else 1.0
    bc2 = 1.0 if mutate == "no_bias_correction" else 1.0 - b2 ** (k + 1)
    lr_k = h["lr"] * sched
    lr_max = max(lr_k, st["lr_max"])
    weight = ((k + 1) ** h["r"]) * (lr_max ** h["weight_lr_power"])
    weight_sum = st["weight_sum"] + weight
    if mutate == "c_from_old_weight_sum":
        c = weight / st["weight_sum"] if st["weight_sum"] != 0.0 else 0.0
    else:
        c = weight / weight_sum if weight_sum != 0.0 else 0.0
    return dict(bc2=bc2, lr_k=lr_k, lr_max=lr_max, weight_sum=weight_sum, c=c, a=lr_k * (b1 * (1.0 - c) - 1.0))


def advanced(h, st):
    s = scalars(h, st)
    return dict(k=st["k"] + 1, weight_sum=s["weight_sum"], lr_max=s["lr_max"], scheduled_lr=s["lr_k"])


_STATES = {}


def group_state(gi, k):
    """The state of group ``gi`` after ``k`` steps from the initial one."""
    if (gi, k) not in _STATES:
        st = dict(k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0)
        for _ in range(k):
            st = advanced(HYPERS[gi], st)
        _STATES[gi, k] = st
    return dict(_STATES[gi, k])


# ---- the step -------------------------------------------------------------------------------------------------------------------
def _f64(t):
    return t.detach().cpu().double()


def restated(y, g, z, v, h, st, mutate=None):
    """One step in float64: ``(y', z', v')``."""
    y, g, z, v = _f64(y), _f64(g), _f64(z), _f64(v)
    s = scalars(h, st, mutate)
    b1, b2 = h["betas"]
    if st["k"] == 0:
        z = y.clone()
    v1 = b2 * v + (1.0 - b2) * g * g
    if mutate == "eps_inside_sqrt":
        denom = torch.sqrt(v1 / s["bc2"] + h["eps"])
    else:
        denom = torch.sqrt(v1 / s["bc2"]) + h["eps"]
    gn = g / denom + h["weight_decay"] * (z if mutate == "wd_times_z" else y)
    y1 = y + (z - y) * s["c"] + s["a"] * gn
    z1 = z - (h["lr"] if mutate == "lr_in_z_update" else s["lr_k"]) * gn
    return y1, z1, v1


def bounds(dtype, y, g, z, v, h, st):
    """``(by, bz, bv)``: see the module docstring."""
    y, g, z, v = _f64(y), _f64(g), _f64(z), _f64(v)
    u, s = U[dtype], scalars(h, st)
    b1, b2 = h["betas"]
    if st["k"] == 0:
        z = y
    v1 = b2 * v + (1.0 - b2) * g * g
    denom = torch.sqrt(v1 / s["bc2"]) + h["eps"]
    t1, t2 = g.abs() / denom, h["weight_decay"] * y.abs()
    e_bc2 = 0.5 * POW_ULPS * U64 * b2 ** (st["k"] + 1) / s["bc2"]
    e_c = (2.0 * POW_ULPS + 2.0) * U64
    d_gn = (12.0 * u + e_bc2) * t1 + 3.0 * u * t2
    big_s, big_g, a = y.abs() + z.abs(), t1 + t2, abs(s["a"])
    by = 4.0 * u * big_s + e_c * s["c"] * big_s + a * d_gn + (3.0 * (u + U64) * a + s["lr_k"] * b1 * s["c"] * e_c) * big_g
    bz = u * z.abs() + 3.0 * u * s["lr_k"] * big_g + s["lr_k"] * d_gn
    bv = 6.0 * u * v1
    return tuple(SLACK[dtype] * b for b in (by, bz, bv))


def assert_step(after, before, h, st, what=""):
    """``after = (y', z', v')`` is one step of ``before = (y, g, z, v)`` within the bounds; returns the worst error / bound."""
    dtype = after[0].dtype
    assert all(t.dtype == dtype for t in after) and after[0].shape == before[0].shape, what
    worst = 0.0
    for name, got, want, bound in zip(("y", "z", "v"), after, restated(*before, h, st), bounds(dtype, *before, h, st)):
        err = (_f64(got) - want).abs()
        ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
        assert bool((err <= bound).all()), f"{what} {name}: k={st['k']} worst error / bound {ratio:.3f}"
        worst = max(worst, ratio)
    return worst


def swap_bound(dtype, a, b, w):
    """``lerp(a, b, w)``: the difference, the scalar, the product, the sum, times ``max(1, |w|)``; doubled in float64."""
    return 4.0 * SLACK[dtype] * U[dtype] * max(1.0, abs(w)) * (_f64(a).abs() + _f64(b).abs())


# ---- the fixture ----------------------------------------------------------------------------------------------------------------
class Fixture:
    """``before(k)``: the 14 ``(y, g, z, v)`` before step ``k``, generated once per ``k`` and handed out as clones."""

    def __init__(self, chunk, seed=20):
        self.chunk = int(chunk)
        self.seed = seed
        self._cache = {}

    def before(self, k):
        if k not in self._cache:
            gen = torch.Generator().manual_seed(self.seed * 100003 + k)
            out = []
            for dtype in (torch.float32, torch.float64):
                for shape, scale in zip(shapes(self.chunk), SCALES):
                    y = torch.randn(shape, generator=gen, dtype=dtype)
                    g = torch.randn(shape, generator=gen, dtype=dtype) * scale
                    g = torch.where(torch.rand(shape, generator=gen) < 0.1, torch.zeros_like(g), g)
                    if g.numel() >= 7:
                        g.view(-1)[2] = 0.0
                    if k == 0:
                        z, v = y.clone(), torch.zeros_like(y)
                    else:
                        z = y + 0.1 * torch.randn(shape, generator=gen, dtype=dtype)
                        v = (torch.randn(shape, generator=gen, dtype=dtype) * scale).square() * 0.5
                    out.append((y, g, z, v))
            self._cache[k] = out
        return [tuple(t.clone() for t in row) for row in self._cache[k]]


def make_optimizer(params, cls, **overrides):
    """The two groups over ``params`` (14 tensors in fixture order)."""
    groups = [dict(HYPERS[gi], params=[p for i, p in enumerate(params) if group_of(i) == gi]) for gi in (0, 1)]
    for g in groups:
        g.update(overrides)
    return cls(groups)


def set_state(opt, params, before, k, z_fill=None):
    """Puts the optimizer over ``params`` into the state before step ``k`` through ``load_state_dict``; the parameters and
    their ``.grad`` are written in place.  ``z_fill``: what ``z`` holds instead (before step 0, where it must not be read)."""
    sd = opt.state_dict()
    ids = order()
    sd["state"] = {}
    with torch.no_grad():
        for slot, i in enumerate(ids):
            y, g, z, v = before[i]
            p = params[i]
            p.copy_(y)
            if p.grad is None:
                p.grad = torch.empty_like(p)
            p.grad.copy_(g)
            if z_fill is not None:
                z = torch.full_like(z, z_fill)
            sd["state"][slot] = {"z": z.clone().to(p.device), "exp_avg_sq": v.clone().to(p.device)}
    for gi, group in enumerate(sd["param_groups"]):
        group.update(group_state(gi, k))
        group["train_mode"] = True
    opt.load_state_dict(sd)


def bits(t):
    """The tensor as integers of its element size, flat: for bit-for-bit comparisons."""
    t = t.detach().contiguous().reshape(-1)
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])

