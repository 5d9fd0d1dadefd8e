"""What the EMA tests share: the layout of ``tests/golden/ref_ema.npz`` (written by ``tests/golden/make_ema_golden.py`` from the
reference's own ``EMAWeights``), the float64 restatement of one update and the error bound.

The parameter list: shapes ``()``, ``(1,)``, ``(7,)``, ``(3, 5)``, ``(C,)``, ``(C + 1,)``, ``(2 C + 3,)`` with ``C`` the chunk
length of the kernels, once in float32 and once in float64 (14 parameters in one model).  The six short tensors are stored
whole.  The long one is a tiling of ``PERIOD`` values at every step (an update is element-wise, so its EMA is the same tiling:
the maker checks that on the reference's output) and one period is stored: nothing of the reference's result is lost.
The float64 parameters are formed from the stored float32 ones (``params64``), with a full double mantissa.

One update is three roundings of quantities no larger than ``|a| + |b|``: the bound per element is ``4 2^-24 (|a| + |b|)`` in
float32 and ``8 2^-53 (|a| + |b|)`` in float64 (which leaves room for the restatement's own rounding), against
``a + (b - a) w`` in float64 with ``w`` formed in Python doubles.  Always one step at a time: nothing accumulates.
"""
import os

import numpy as np
import torch

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_ema.npz")
PERIOD = 41
N_STEPS = 12
RECORDED = {0.5: (1, 2, 3, 8, 9, 10, 11, 12), 0.999: (1, 2)}  # EMA states kept (8 and 11: the states before 9 and 12)
CHECKED = {0.5: (1, 2, 3, 9, 10, 12), 0.999: (1, 2)}  # updates compared one step at a time
EPS = {torch.float32: 4.0 * 2.0 ** -24, torch.float64: 8.0 * 2.0 ** -53}


def shapes(chunk):
    return [(), (1,), (7,), (3, 5), (chunk,), (chunk + 1,), (2 * chunk + 3,)]


def tag(decay):
    return {0.5: "d05", 0.999: "d999"}[decay]


def expand(flat, chunk):
    """The stored 1-D array of one state and dtype -> the list of full tensors."""
    flat = np.asarray(flat)
    out, at = [], 0
    for shape in shapes(chunk):
        n = int(np.prod(shape, dtype=np.int64))
        if n == 2 * chunk + 3:
            out.append(torch.from_numpy(np.resize(flat[at:at + PERIOD], n).copy()))
            at += PERIOD
        else:
            out.append(torch.from_numpy(flat[at:at + n].copy()).reshape(shape))
            at += n
    assert at == len(flat)
    return out


def condense(tensors, chunk):
    """Inverse of ``expand`` (the long tensor must be the tiling of its first period)."""
    parts = []
    for t, shape in zip(tensors, shapes(chunk)):
        t = t.detach().reshape(-1)
        if t.numel() == 2 * chunk + 3:
            assert torch.equal(t, torch.from_numpy(np.resize(t[:PERIOD].numpy(), t.numel()))), "not a tiling"
            t = t[:PERIOD]
        parts.append(t.numpy())
    return np.concatenate(parts)


def params64(p32, p32_other):
    """Float64 parameters with a full mantissa from two stored float32 sets."""
    return [a.double() + b.double() * 2.0 ** -26 for a, b in zip(p32, p32_other)]


class Fixture:
    def __init__(self):
        self.z = np.load(FIXTURE)
        self.chunk = int(self.z["chunk"])
        self.state_keys = [str(k) for k in self.z["state_keys"]]
        self.extra_state = {"decay": float(self.z["extra_decay"]), "num_updates": int(self.z["extra_num_updates"]),
                            "is_holding_ema_weights": bool(self.z["extra_is_holding_ema_weights"])}
        self._params = {}

    def params(self, k):
        """The 14 parameters before update ``k`` (1-based): 7 float32, then 7 float64."""
        if k not in self._params:
            p32 = expand(self.z[f"p32_{k}"], self.chunk)
            other = expand(self.z[f"p32_{k % N_STEPS + 1}"], self.chunk)
            self._params[k] = p32 + params64(p32, other)
        return [t.clone() for t in self._params[k]]

    def ema(self, decay, k):
        """The reference's 14 EMA buffers after update ``k``."""
        return expand(self.z[f"ema32_{tag(decay)}_{k}"], self.chunk) + expand(self.z[f"ema64_{tag(decay)}_{k}"], self.chunk)


def bits(t):
    """The tensor as integers of its element size, flat: for bit-for-bit comparisons (NaN payloads and signed zeros included)."""
    t = t.detach().reshape(-1)
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()])


def weight(decay, n):
    return 1.0 - min(decay, (1 + n) / (10 + n))


def restated(ema, param, n, decay):
    """Float64 restatement of the update with ``n`` updates done before it."""
    a, b = ema.detach().cpu().double(), param.detach().cpu().double()
    return b.clone() if n == 0 else a + (b - a) * weight(decay, n)


def assert_update(after, before, param, n, decay, what=""):
    """``after`` is one update of ``before`` towards ``param``, within the bound (exactly ``param`` for ``n == 0``)."""
    assert after.dtype == before.dtype == param.dtype and after.shape == param.shape, what
    got = after.detach().cpu().double()
    if n == 0:
        assert torch.equal(got, param.detach().cpu().double()), f"{what}: the first update must copy"
        return 0.0
    want = restated(before, param, n, decay)
    bound = EPS[after.dtype] * (before.detach().cpu().double().abs() + param.detach().cpu().double().abs())
    err = (got - want).abs()
    assert bool((err <= bound).all()), f"{what}: n={n} worst error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}"
    return float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.0
