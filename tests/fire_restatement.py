"""What the FIRE tests share: a numpy float64 restatement of the definition that ``nequip_amd/integrations/relax.py`` and
``csrc/relax.hip`` implement, per system; the textbook loop; the analytic test force; the comparison.

One step of a system, with ``F`` the force at the current positions (rows of ``fixed`` atoms count as zero)::

    reduce   P = sum F.v,  FF = sum F.F,  VV = sum v.v,  M = max over atoms of (Fx^2 + Fy^2 + Fz^2)
    decide   fmax = sqrt(M);  converged = M < fmax_target^2;  if converged nothing changes, else
               nsteps == 0:  cv = 0, cf = 0
               P > 0:        cv = 1 - a, cf = a sqrt(VV) / sqrt(FF); if npos > nmin: dt = min(dt finc, dtmax), a = a fa; npos += 1
               otherwise:    cv = 0, cf = 0, a = astart, dt = dt fdec, npos = 0
             c = cf + dt;  VVn = cv cv VV + 2 cv c P + c c FF;  normdr = dt sqrt(VVn)
             scale = normdr > maxstep ? maxstep / normdr : 1;  nsteps += 1
    move     v = cv v + cf F;  v = v + dt F;  x = x + scale (dt v)

``textbook`` is ASE's loop written out literally, with the direct norm ``dr = dt v; normdr = sqrt(vdot(dr, dr))``.

The decisions.  Three comparisons of floating-point numbers steer a run: ``P > 0``, ``normdr > maxstep`` and ``M < fmax_target^2``.
The restatement records the relative margin of every one it takes (``|P| / sqrt(FF VV)``, ``|normdr - maxstep| / maxstep``,
``|M - target^2| / target^2``) and asserts that each is at least ``MARGIN = 1e-6``, seven orders of magnitude above anything a
summation order can change, so driver and restatement take the same branches.

The bounds.  Given the same branches, both sides carry out the same float64 operations per element; they differ in the order in
which the three sums over the ``3 n`` components of a system are added.  A sum of ``m`` terms of one sign is off by at most about
``m eps`` relative (``eps = 2^-53``); ``P`` is not of one sign, but it enters only through ``VVn``, whose three terms are all
non-negative and of which ``|2 cv c P| <= cv^2 VV + c^2 FF`` (Cauchy-Schwarz, then the inequality of the means), so ``VVn``, and
with it ``scale``, is off by about ``3 n eps`` relative at most, and so is ``cf``.  Per step that moves every velocity by at most
``3 n eps |cf F_i| <= 3 n eps ||v||`` (``||cf F|| = a ||v||``, ``a <= 1``) and every position by at most ``3 n eps`` times the length of the
step, which ``maxstep`` caps.  Once the two sides differ at all, their per-element roundings are no longer the same either: each
step adds up to about ``eps |x|`` to a position and ``eps |v|`` to a velocity.  These errors feed back through the force.  The
linearised map of a step is a damped velocity-Verlet map, which does not amplify errors exponentially as long as
``dt^2 k_eff < 4``; here ``dt <= dtmax = 1`` and ``k_eff = k + 3 q d^2 <= 2.8``.  ``AMP = 8`` is allowed for its transient
growth.  Over ``steps`` steps, element by element and with no relative term::

    |x - x_ref| <= AMP steps eps (3 n maxstep + max |x_ref|)
    |v - v_ref| <= AMP steps eps (3 n + 1) max over the run of ||v_ref||

For the largest case (n = 16 385, 25 steps, maxstep 0.2) that is 2.2e-10 Angstrom; for n = 1 it is 1e-13.  Observed errors are at
the level of a few eps, since rounding errors do not all point the same way.  The state ``dt``, ``a``, ``npos``, ``nsteps`` follows
from the branches alone and is compared exactly.  ``fmax`` is the square root of a maximum, which no order changes, over forces
at positions that are off by the above: with ``|dF| <= k_eff sqrt(3) |dx|`` it may differ by ``5 x_atol``, plus 8 eps relative
for the square root and the three squares.  A float32 force is evaluated by the same torch function on the same device on both
sides, so it is the same float32 number wherever the positions are the same float64 numbers.
"""
import math

import numpy as np
import torch

EPS = 2.0 ** -53
AMP = 8.0
MARGIN = 1e-6
DEFAULTS = dict(dt=0.1, maxstep=0.2, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)

# ---- the analytic force: every atom in an anharmonic well of its own, F = -k_i (x - x0_i) - q |x - x0_i|^2 (x - x0_i) ------------
Q_WELL = 0.5


def wells(n, seed=0, spread=0.4):
    """``n`` wells (stiffness ``k`` in [0.5, 2], centres ``x0`` away from the origin) and start positions ``x`` about them."""
    rng = np.random.default_rng(seed)
    k = rng.uniform(0.5, 2.0, size=n)
    x0 = np.array([3.0, -2.0, 2.5]) + rng.uniform(-0.5, 0.5, size=(n, 3))
    x = x0 + spread * rng.normal(size=(n, 3))
    return k, x0, x


def force_numpy(x, k, x0):
    d = x - x0
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return -k[:, None] * d - (Q_WELL * r2)[:, None] * d


def force_torch(x, k, x0):
    """The same operations in the same order on the tensors' device (float64)."""
    d = x - x0
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return -k[:, None] * d - (Q_WELL * r2)[:, None] * d


def energy_torch(x, k, x0):
    d = x - x0
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    return (0.5 * k * r2 + 0.25 * Q_WELL * r2 * r2).sum()


def torch_force_step(k, x0, device, force_dtype=torch.float64):
    """A ``force_step`` for the driver: forces rounded to ``force_dtype``.  The wells live on the device before the first call,
    so that the call copies nothing from the host (it can be captured into a graph)."""
    kt, x0t = torch.from_numpy(np.ascontiguousarray(k)).to(device), torch.from_numpy(np.ascontiguousarray(x0)).to(device)

    def step(pos):
        return {"forces": force_torch(pos, kt, x0t).to(force_dtype), "total_energy": energy_torch(pos, kt, x0t).reshape(1, 1)}

    return step


def restated_force(k, x0, device, force_dtype=torch.float64):
    """The force callback of the restatement that rounds like ``torch_force_step``: the same function on the same device."""
    step = torch_force_step(k, x0, device, force_dtype)

    def force(x):
        return step(torch.from_numpy(np.ascontiguousarray(x)).to(device))["forces"].double().cpu().numpy()

    return force


# ---- the restatement -------------------------------------------------------------------------------------------------------------
class Restated:
    """Float64 numpy FIRE of ONE system.  ``force(x [n, 3]) -> F [n, 3]``; ``fixed``: ``[n]`` bool or None."""

    def __init__(self, force, x, fixed=None, fmax_target=0.05, **params):
        p = dict(DEFAULTS, **params)
        self.force, self.p, self.target = force, p, float(fmax_target)
        self.x = np.array(x, dtype=np.float64)
        self.v = np.zeros_like(self.x)
        self.fixed = np.zeros(len(self.x), dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
        self.dt, self.a, self.npos, self.nsteps = float(p["dt"]), float(p["astart"]), 0, 0
        self.fmax, self.converged = 0.0, False
        self.margins = {"P": math.inf, "cap": math.inf, "fmax": math.inf}
        self.capped, self.vnorm_max = 0, 0.0
        self.f = np.asarray(self.force(self.x), dtype=np.float64)

    def _decision(self, name, margin):
        assert margin >= MARGIN, f"the {name} decision of step {self.nsteps} has a relative margin of {margin:.3e} only"
        self.margins[name] = min(self.margins[name], margin)

    def step(self, new_forces=None):
        """``new_forces``: the force at the new positions, where the caller has it (lockstep runs); else ``force`` is asked."""
        p = self.p
        f = np.where(self.fixed[:, None], 0.0, self.f)
        v = self.v
        # reduce
        P, FF, VV = float(np.sum(f * v)), float(np.sum(f * f)), float(np.sum(v * v))
        M = float(np.max(f[:, 0] * f[:, 0] + f[:, 1] * f[:, 1] + f[:, 2] * f[:, 2]))
        # decide
        t2 = self.target * self.target
        self._decision("fmax", abs(M - t2) / t2)
        self.fmax, self.converged = math.sqrt(M), M < t2
        if self.converged:
            return
        dt, a = self.dt, self.a
        cv = cf = 0.0
        if self.nsteps == 0:
            assert VV == 0.0
        else:
            self._decision("P", abs(P) / math.sqrt(FF * VV))
            if P > 0.0:
                cv = 1.0 - a
                cf = a * math.sqrt(VV) / math.sqrt(FF)
                if self.npos > p["nmin"]:
                    dt = min(dt * p["finc"], p["dtmax"])
                    a = a * p["fa"]
                self.npos += 1
            else:
                a, dt, self.npos = p["astart"], dt * p["fdec"], 0
        c = cf + dt
        vvn = cv * cv * VV + 2.0 * cv * c * P + c * c * FF
        normdr = dt * math.sqrt(vvn)
        self._decision("cap", abs(normdr - p["maxstep"]) / p["maxstep"])
        capped = normdr > p["maxstep"]
        scale = p["maxstep"] / normdr if capped else 1.0
        self.capped += int(capped)
        self.dt, self.a = dt, a
        self.nsteps += 1
        # move
        free = ~self.fixed[:, None]
        v_new = cv * v + cf * f
        v_new = v_new + dt * f
        self.v = np.where(free, v_new, v)
        self.x = np.where(free, self.x + scale * (dt * v_new), self.x)
        self.vnorm_max = max(self.vnorm_max, float(np.sqrt(np.sum(self.v * self.v))))
        self.f = np.asarray(self.force(self.x) if new_forces is None else new_forces, dtype=np.float64)

    def run(self, n):
        for _ in range(n):
            self.step()

    def relax(self, fmax, max_steps=10000):
        """Steps until the verdict is ``converged``; returns the number of steps that moved the system."""
        self.target = float(fmax)
        for _ in range(max_steps):
            self.step()
            if self.converged:
                return self.nsteps
        raise AssertionError(f"the restatement did not reach fmax < {fmax} in {max_steps} steps")


def textbook(force, x, steps, **params):
    """ASE's FIRE loop, literally (no convergence test): ``(x, v)`` after ``steps`` steps."""
    p = dict(DEFAULTS, **params)
    r = np.array(x, dtype=np.float64)
    v, dt, a, npos = None, p["dt"], p["astart"], 0
    for _ in range(steps):
        f = np.asarray(force(r), dtype=np.float64)
        if v is None:
            v = np.zeros_like(r)
        else:
            vf = np.vdot(f, v)
            if vf > 0.0:
                v = (1.0 - a) * v + a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(v, v))
                if npos > p["nmin"]:
                    dt = min(dt * p["finc"], p["dtmax"])
                    a *= p["fa"]
                npos += 1
            else:
                v[:] *= 0.0
                a = p["astart"]
                dt *= p["fdec"]
                npos = 0
        v += dt * f
        dr = dt * v
        normdr = np.sqrt(np.vdot(dr, dr))
        if normdr > p["maxstep"]:
            dr = p["maxstep"] * dr / normdr
        r = r + dr
    return r, v


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def bounds(ref, steps):
    """``(x_atol, v_atol)`` of the docstring for the system of ``ref`` after ``steps`` steps."""
    n = len(ref.x)
    x_atol = AMP * steps * EPS * (3 * n * ref.p["maxstep"] + float(np.max(np.abs(ref.x))))
    v_atol = AMP * steps * EPS * (3 * n + 1) * ref.vnorm_max
    return x_atol, v_atol


def assert_close(driver, refs, what="", steps=None):
    """The driver (one system per entry of ``refs``, concatenated) against the restatements: positions and velocities at the
    bounds of the docstring, the rest of the state exactly."""
    refs = list(refs)
    x, v = driver.positions.detach().cpu().numpy(), driver.velocities.detach().cpu().numpy()
    dt, a = driver.dt.detach().cpu().numpy(), driver.a.detach().cpu().numpy()
    nsteps, conv = driver.nsteps.detach().cpu().numpy(), driver.converged.detach().cpu().numpy()
    fmax = driver.fmax.detach().cpu().numpy()
    assert len(refs) == driver.num_systems
    off, worst_x, worst_v = 0, 0.0, 0.0
    for s, ref in enumerate(refs):
        n = len(ref.x)
        x_atol, v_atol = bounds(ref, ref.nsteps if steps is None else steps)
        ex, ev = float(np.max(np.abs(x[off:off + n] - ref.x))), float(np.max(np.abs(v[off:off + n] - ref.v)))
        if ref.nsteps > 0:  # (a system that never moved has bounds of zero)
            worst_x, worst_v = max(worst_x, ex / x_atol), max(worst_v, ev / v_atol)
        assert ex <= x_atol, f"{what}: positions of system {s} off by {ex:.3e}, bound {x_atol:.3e}"
        assert ev <= v_atol, f"{what}: velocities of system {s} off by {ev:.3e}, bound {v_atol:.3e}"
        assert dt[s] == ref.dt and a[s] == ref.a and nsteps[s] == ref.nsteps, \
            f"{what}: system {s} has dt {dt[s]!r} a {a[s]!r} nsteps {nsteps[s]}, restatement {ref.dt!r} {ref.a!r} {ref.nsteps}"
        assert bool(conv[s]) == ref.converged, f"{what}: verdict of system {s}"
        np.testing.assert_allclose(fmax[s], ref.fmax, rtol=8 * EPS, atol=5 * x_atol, err_msg=f"{what}: fmax of system {s}")
        off += n
    assert off == x.shape[0]
    print(f"{what}: worst error of x {worst_x:.3e}, of v {worst_v:.3e} of their bounds")
