"""What the variable-cell FIRE tests share: the analytic test potential (energy, forces, stress), a numpy float64 restatement of
the definition that ``nequip_amd.integrations.CellFIRE`` and ``csrc/relax_cell.hip`` implement, per system; the literal filter and
FIRE loop; the comparison.

The definition.  Per system: ``n`` atoms, reference cell ``C0`` (rows are the lattice vectors), current cell ``C = C0 D^T``,
``cell_factor`` (default ``n``).  Generalised coordinates ``q_i = x_i D^-T`` (carried, never re-solved) and ``Q = cell_factor D``.
With ``F`` the force and ``sigma`` the stress at ``(x, C)``, ``V = |det C|``::

    atoms    g_i = F_i D                                  (rows of fixed atoms count as zero)
    cell     W = -V (sigma + p I);  G = W D^-T;  hydrostatic: G = (tr G / 3) I;  mask: G = G * mask;
             constant_volume: tr G / 3 off the diagonal;  G = G / cell_factor
    reduce   P = sum g.v,  FF = sum g.g,  VV = sum v.v,  M = max |g_i|^2          (over the atoms, with the D of F)
    decide   the 9 components of G join P, FF, VV (against vD), its three row norms join M
             fmax = sqrt(M);  converged = M < target^2;  if converged nothing changes, else the FIRE branch of
             fire_restatement.py (cv, cf, dt, a, npos, scale, nsteps += 1) and the cell move:
             vD = cv vD + cf G;  vD = vD + dt G;  Q = cell_factor D + scale (dt vD);  D_new = Q / cell_factor;  C = C0 D_new^T
    move     g = F D_old;  v = cv v + cf g;  v = v + dt g;  q = q + scale (dt v);  x = q D_new^T

``textbook`` is the literal loop: ASE's ``UnitCellFilter`` (``get_positions`` / ``get_forces`` / ``set_positions``, with ``q``
re-solved from ``x`` at every step) around ASE's FIRE with the direct norm of the step.

The test potential.  Every atom is tethered to a fractional site that follows the cell, ``d_i = x_i - s0_i C``::

    E     = sum (k_i / 2 |d_i|^2 + q / 4 |d_i|^4) + B / 2 (V - V0)^2 / V0 + K / 4 ||C^T C - G0||_F^2
    F_i   = -(k_i + q |d_i|^2) d_i
    sigma = (1 / V) [ sum (k_i + q |d_i|^2) d_i (x) d_i + B (V - V0) / V0 V I + sym(K A (A - G0)) ],   A = C^T C

with ``q = 0.5``, ``B = 2``, ``K = 0.3``, a triclinic ``C0``, and ``G0``, ``V0`` from a target cell 5 % away.  It is written once
for numpy arrays and torch tensors: elementwise operations and sums over the atoms by a fixed pairwise tree, so that a system gives
the same bits alone and inside a batch, on either library.

The decisions.  As in fire_restatement.py: ``P > 0``, ``normdr > maxstep`` and ``M < target^2`` steer a run; the restatement records
the relative margin of every one it takes and asserts that each is at least ``MARGIN = 1e-6``.

The bounds.  Given the same branches, both sides carry out the same float64 operations per element, up to the order of the sums
over the ``m = 3 (n + 3)`` generalised components and of the three-term sums of the 3 x 3 products.  The derivation of
fire_restatement.py carries over with ``m`` for ``3 n``: ``VVn``, ``scale`` and ``cf`` are off by ``m eps`` relative at most, which
moves a generalised coordinate by at most ``m eps`` times the length of the step, capped by ``maxstep``, and a velocity by
``m eps ||v||``; ``AMP = 8`` covers the transient growth through the force.  New are the 3 x 3 products.  With the cell strain
inside 20 %, ``||D||`` and ``||D^-1||`` stay below ``R = 1.5``:

* ``g = F D``: three terms, off by ``3 eps |F| ||D|| <= 3 R eps`` relative to ``|F|``, i.e. ``3 R^2 eps`` relative to ``|g|``;
  it enters ``v`` like the force does.
* ``x = q D^T``: off by ``3 eps |q| ||D|| <= 3 R^2 eps |x|`` per evaluation, and by ``3 |q| |dD| <= 3 R max |x| |dD|`` where
  ``D`` itself is off by ``dD``.
* ``G = W D^-T / cell_factor``: the determinant of ``C`` (five roundings), the cofactors and determinant of ``D`` (relative to
  ``||D||^2``), the quotient and the three-term product: allowed ``CELL_OPS = 30`` eps relative in all, which moves ``vD`` like a
  force error and ``D`` by that fraction of the step; ``Q = cell_factor D``, the sum and ``Q / cell_factor`` round ``D`` three
  more times per step.  A step of the cell is a step of ``Q``: ``D`` moves by at most ``maxstep / cell_factor``.

Over ``steps`` steps, element by element and with no relative term (``xmax = max |x_ref|``)::

    |D - D_ref|   <= AMP steps eps ((m + CELL_OPS) maxstep / cell_factor + 3 max |D_ref|)                      =: D_atol
    |x - x_ref|   <= AMP steps eps (m maxstep + (1 + 3 R^2) xmax) + 3 R xmax D_atol                            =: x_atol
    |v - v_ref|   <= AMP steps eps (m + 1 + 3 R^2) max over the run of ||(v, vD)_ref||                         =: v_atol
    |vD - vD_ref| <= AMP steps eps (m + 1 + CELL_OPS) max over the run of ||(v, vD)_ref||

``dt``, ``a``, ``npos``, ``nsteps`` and the verdict follow from the branches alone and are compared exactly.  ``fmax`` is the square
root of a maximum over forces at coordinates that are off by the above: an atom's ``d_i`` is off by ``x_atol + 3 cmax D_atol``
(``cmax = max |C0|``, ``|s0| <= 1``) and ``|dF| <= k_eff sqrt(3) |dd|`` with ``k_eff <= 2.8``, hence ``5 (x_atol + 3 cmax D_atol)``;
a row of ``G`` is off by the stiffness of the cell terms, ``(2 B V R^2 + 12 K ||C||_F^4) / cell_factor`` per unit of ``D``, times
``3 D_atol``; plus ``16 eps`` relative for the square root, the squares and ``g = F D``.
"""
import math

import numpy as np
import torch

from fire_restatement import AMP, DEFAULTS, EPS, MARGIN

R_NORM = 1.5
CELL_OPS = 30.0
Q_WELL, B_BULK, K_SHAPE = 0.5, 2.0, 0.3


# ---- the potential, once for numpy and torch -------------------------------------------------------------------------------------
def _tree_sum(t):
    """The sum over axis 0 by a fixed pairwise tree (zeros up to the next power of two): the same bits whatever the library, the
    device and the place of the rows in a larger array."""
    n, length = t.shape[0], 1
    while length < n:
        length *= 2
    if length != n:
        shape = (length - n,) + tuple(t.shape[1:])
        if isinstance(t, torch.Tensor):
            t = torch.cat([t, torch.zeros(shape, dtype=t.dtype, device=t.device)])
        else:
            t = np.concatenate([t, np.zeros(shape, dtype=t.dtype)])
    while length > 1:
        length //= 2
        t = t[:length] + t[length:2 * length]
    return t[0]


def _stack(parts):
    return torch.stack(parts) if isinstance(parts[0], torch.Tensor) else np.stack(parts)


def _matmul3(a, b):
    """``a b`` for ``[..., 3, 3]``, the three products added left to right."""
    return (a[..., :, 0, None] * b[..., 0, None, :] + a[..., :, 1, None] * b[..., 1, None, :]
            + a[..., :, 2, None] * b[..., 2, None, :])


def _transpose(a):
    return a.transpose(-1, -2) if isinstance(a, torch.Tensor) else np.swapaxes(a, -1, -2)


def _det3(c):
    """``[S]`` determinants of ``[S, 3, 3]``."""
    return (c[:, 0, 0] * (c[:, 1, 1] * c[:, 2, 2] - c[:, 1, 2] * c[:, 2, 1])
            - c[:, 0, 1] * (c[:, 1, 0] * c[:, 2, 2] - c[:, 1, 2] * c[:, 2, 0])
            + c[:, 0, 2] * (c[:, 1, 0] * c[:, 2, 1] - c[:, 1, 1] * c[:, 2, 0]))


def potential(x, cell, k, s0, g0, v0, sidx, offsets):
    """``(E [S], F [N, 3], sigma [S, 3, 3])`` at positions ``x [N, 3]`` and cells ``cell [S, 3, 3]``.  ``k [N]``, ``s0 [N, 3]``,
    ``g0 [S, 3, 3]``, ``v0 [S]``, ``sidx [N]`` (the system of every atom) are arrays or tensors like ``x``; ``offsets`` is the
    Python list of the ``S + 1`` atom offsets."""
    cn = cell[sidx]
    d = x - (s0[:, 0:1] * cn[:, 0, :] + s0[:, 1:2] * cn[:, 1, :] + s0[:, 2:3] * cn[:, 2, :])
    r2 = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    w = k + Q_WELL * r2
    forces = -w[:, None] * d
    e_atom = 0.5 * k * r2 + 0.25 * Q_WELL * r2 * r2
    dyad = w[:, None, None] * (d[:, :, None] * d[:, None, :])
    e_sites = _stack([_tree_sum(e_atom[offsets[s]:offsets[s + 1]]) for s in range(len(offsets) - 1)])
    site = _stack([_tree_sum(dyad[offsets[s]:offsets[s + 1]]) for s in range(len(offsets) - 1)])
    vol = abs(_det3(cell))
    a = _matmul3(_transpose(cell), cell)
    resid = a - g0
    shape = K_SHAPE * _matmul3(a, resid)
    shape = 0.5 * (shape + _transpose(shape))
    eye = torch.eye(3, dtype=cell.dtype, device=cell.device) if isinstance(cell, torch.Tensor) else np.eye(3)
    bulk = (B_BULK * (vol - v0) / v0 * vol)[:, None, None] * eye
    sigma = (site + bulk + shape) / vol[:, None, None]
    energy = e_sites + 0.5 * B_BULK * (vol - v0) * (vol - v0) / v0 + 0.25 * K_SHAPE * (resid * resid).reshape(-1, 9).sum(-1)
    return energy, forces, sigma


BASE_CELL = np.array([[4.0, 0.3, 0.2], [0.1, 4.4, 0.4], [0.3, 0.2, 3.8]])


def site_system(n, seed=0, spread=0.3, at_minimum=False):
    """One system: ``dict(k, s0, c0, g0, v0, x)``.  A triclinic ``C0``; ``G0`` and ``V0`` from a target cell 5 % away; the atoms
    start ``spread`` away from their sites.  ``at_minimum``: target cell = ``C0`` and atoms on their sites (E = 0, F = 0,
    sigma = 0)."""
    rng = np.random.default_rng(seed)
    c0 = BASE_CELL + rng.uniform(-0.1, 0.1, size=(3, 3))
    target = c0 if at_minimum else c0 @ (np.eye(3) + 0.05 * rng.uniform(-1.0, 1.0, size=(3, 3)))
    k = rng.uniform(0.5, 2.0, size=n)
    s0 = rng.uniform(0.0, 1.0, size=(n, 3))
    sites = s0[:, 0:1] * c0[0] + s0[:, 1:2] * c0[1] + s0[:, 2:3] * c0[2]
    x = sites if at_minimum else sites + spread * rng.normal(size=(n, 3))
    g0 = _matmul3(target.T[None], target[None])[0]
    return dict(k=k, s0=s0, c0=c0, g0=g0, v0=abs(float(_det3(target[None])[0])), x=x)


def concatenated(parts):
    """The systems of ``parts`` along the atom axis: ``dict(k, s0, c0 [S, 3, 3], g0, v0 [S], x, sidx, offsets)``."""
    counts = [len(p["k"]) for p in parts]
    return dict(k=np.concatenate([p["k"] for p in parts]), s0=np.concatenate([p["s0"] for p in parts]),
                c0=np.stack([p["c0"] for p in parts]), g0=np.stack([p["g0"] for p in parts]),
                v0=np.array([p["v0"] for p in parts]), x=np.concatenate([p["x"] for p in parts]),
                sidx=np.repeat(np.arange(len(parts)), counts), offsets=[0] + list(np.cumsum(counts).tolist()))


def numpy_force(part):
    """``force(x, C) -> (F, sigma [3, 3])`` of one system in numpy."""
    n = len(part["k"])
    sidx = np.zeros(n, dtype=np.int64)

    def force(x, cell):
        _, f, sig = potential(x, cell[None], part["k"], part["s0"], part["g0"][None], np.array([part["v0"]]), sidx, [0, n])
        return f, sig[0]

    return force


def numpy_energy(part, x, cell):
    n = len(part["k"])
    return float(potential(x, cell[None], part["k"], part["s0"], part["g0"][None], np.array([part["v0"]]),
                           np.zeros(n, dtype=np.int64), [0, n])[0][0])


def torch_force_step(parts, device, dtype=torch.float64):
    """A ``force_step(positions, cell)`` for the driver over the systems of ``parts``: forces and stress rounded to ``dtype``.
    Everything it reads lives on the device before the first call, so that a call copies nothing from the host."""
    c = concatenated(parts)
    t = {name: torch.from_numpy(np.ascontiguousarray(c[name])).to(device) for name in ("k", "s0", "g0", "v0", "sidx")}
    offsets = c["offsets"]

    def step(pos, cell):
        e, f, sig = potential(pos, cell, t["k"], t["s0"], t["g0"], t["v0"], t["sidx"], offsets)
        return {"forces": f.to(dtype), "total_energy": e, "stress": sig.to(dtype)}

    return step


def restated_force(part, device, dtype=torch.float64):
    """The force callback of the restatement that rounds like ``torch_force_step``: the same function on the same device."""
    step = torch_force_step([part], device, dtype)

    def force(x, cell):
        out = step(torch.from_numpy(np.ascontiguousarray(x)).to(device), torch.from_numpy(np.ascontiguousarray(cell[None])).to(device))
        return out["forces"].double().cpu().numpy(), out["stress"].double().cpu().numpy()[0]

    return force


# ---- 3 x 3 helpers of the restatement --------------------------------------------------------------------------------------------
def inverse_transpose(d):
    """``D^-T`` by cofactors."""
    cof = np.empty((3, 3))
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            cof[i, j] = d[i1, j1] * d[i2, j2] - d[i1, j2] * d[i2, j1]
    det = d[0, 0] * cof[0, 0] + d[0, 1] * cof[0, 1] + d[0, 2] * cof[0, 2]
    return cof / det


def cell_force(sigma, d, c0, cell_factor, pressure=0.0, hydrostatic=False, constant_volume=False, mask=None):
    cell = c0 @ d.T
    vol = abs(float(_det3(cell[None])[0]))
    w = -vol * (sigma + pressure * np.eye(3))
    g = w @ inverse_transpose(d)
    if hydrostatic:
        g = (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0 * np.eye(3)
    if mask is not None:
        g = g * mask
    if constant_volume:
        g = g - (g[0, 0] + g[1, 1] + g[2, 2]) / 3.0 * np.eye(3)
    return g / cell_factor


# ---- the restatement -------------------------------------------------------------------------------------------------------------
class Restated:
    """Float64 numpy variable-cell FIRE of ONE system.  ``force(x [n, 3], C [3, 3]) -> (F [n, 3], sigma [3, 3])``."""

    def __init__(self, force, x, c0, fixed=None, cell_factor=None, scalar_pressure=0.0, hydrostatic_strain=False,
                 constant_volume=False, mask=None, fmax_target=0.05, **params):
        p = dict(DEFAULTS, **params)
        self.force, self.p, self.target = force, p, float(fmax_target)
        self.x = np.array(x, dtype=np.float64)
        self.q = self.x.copy()
        n = len(self.x)
        self.c0 = np.array(c0, dtype=np.float64)
        self.cell = self.c0.copy()
        self.D, self.vD = np.eye(3), np.zeros((3, 3))
        self.v = np.zeros_like(self.x)
        self.fixed = np.zeros(n, dtype=bool) if fixed is None else np.asarray(fixed, dtype=bool)
        self.cell_factor = float(n if cell_factor is None else cell_factor)
        self.filter = dict(pressure=float(scalar_pressure), hydrostatic=bool(hydrostatic_strain),
                           constant_volume=bool(constant_volume), mask=None if mask is None else np.asarray(mask, dtype=np.float64))
        self.dt, self.a, self.npos, self.nsteps = float(p["dt"]), float(p["astart"]), 0, 0
        self.fmax, self.converged = 0.0, False
        self.margins = {"P": math.inf, "cap": math.inf, "fmax": math.inf}
        self.capped, self.vnorm_max = 0, 0.0
        self.f, self.sigma = self.force(self.x, self.cell)

    def _decision(self, name, margin):
        assert margin >= MARGIN, f"the {name} decision of step {self.nsteps} has a relative margin of {margin:.3e} only"
        self.margins[name] = min(self.margins[name], margin)

    def generalised(self):
        """``(g [n, 3], G [3, 3])`` at the current state."""
        f = np.where(self.fixed[:, None], 0.0, np.asarray(self.f, dtype=np.float64))
        return f @ self.D, cell_force(np.asarray(self.sigma, dtype=np.float64), self.D, self.c0, self.cell_factor, **self.filter)

    def step(self):
        p = self.p
        g, G = self.generalised()
        v, vD = self.v, self.vD
        # reduce, and the cell's rows
        P = float(np.sum(g * v)) + float(np.sum(G * vD))
        FF = float(np.sum(g * g)) + float(np.sum(G * G))
        VV = float(np.sum(v * v)) + float(np.sum(vD * vD))
        M = max(float(np.max(np.sum(g * g, axis=1))), float(np.max(np.sum(G * G, axis=1))))
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
        # the cell move
        vD_new = cv * vD + cf * G
        vD_new = vD_new + dt * G
        Q = self.cell_factor * self.D
        Q = Q + scale * (dt * vD_new)
        self.vD, self.D = vD_new, Q / self.cell_factor
        self.cell = self.c0 @ self.D.T
        # move
        free = ~self.fixed[:, None]
        v_new = cv * v + cf * g
        v_new = v_new + dt * g
        self.v = np.where(free, v_new, v)
        self.q = np.where(free, self.q + scale * (dt * v_new), self.q)
        self.x = self.q @ self.D.T
        self.vnorm_max = max(self.vnorm_max, math.sqrt(float(np.sum(self.v * self.v)) + float(np.sum(self.vD * self.vD))))
        self.f, self.sigma = self.force(self.x, self.cell)

    def run(self, n):
        for _ in range(n):
            self.step()

    def relax(self, fmax, max_steps=10000):
        self.target = float(fmax)
        for _ in range(max_steps):
            self.step()
            if self.converged:
                return self.nsteps
        raise AssertionError(f"the restatement did not reach fmax < {fmax} in {max_steps} steps")


def textbook(force, x, c0, steps, cell_factor=None, scalar_pressure=0.0, hydrostatic_strain=False, constant_volume=False,
             mask=None, **params):
    """ASE's ``UnitCellFilter`` around ASE's FIRE, literally (no convergence test): ``(x, C, v)`` after ``steps`` steps, with
    ``v`` the ``[n + 3, 3]`` generalised velocities."""
    p = dict(DEFAULTS, **params)
    x, c0 = np.array(x, dtype=np.float64), np.array(c0, dtype=np.float64)
    n = len(x)
    cell = c0.copy()
    factor = float(n if cell_factor is None else cell_factor)
    v, dt, a, npos = None, p["dt"], p["astart"], 0
    for _ in range(steps):
        # get_positions / get_forces of the filter
        D = np.linalg.solve(c0, cell).T
        r = np.concatenate([np.linalg.solve(D, x.T).T, factor * D])
        F, sigma = force(x, cell)
        vol = abs(np.linalg.det(cell))
        virial = -vol * (sigma + scalar_pressure * np.eye(3))
        virial = np.linalg.solve(D, virial.T).T
        if hydrostatic_strain:
            virial = np.diag([virial.trace() / 3.0] * 3)
        if mask is not None:
            virial = virial * mask
        if constant_volume:
            virial = virial - np.eye(3) * (virial.trace() / 3.0)
        f = np.concatenate([F @ D, virial / factor])
        # FIRE
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
        # set_positions of the filter
        D_new = r[n:] / factor
        cell = c0 @ D_new.T
        x = r[:n] @ D_new.T
    return x, cell, v


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def bounds(ref, steps):
    """``(x_atol, v_atol, D_atol, vD_atol, fmax_atol)`` of the docstring for the system of ``ref`` after ``steps`` steps."""
    n = len(ref.x)
    m = 3 * (n + 3)
    maxstep, factor = ref.p["maxstep"], ref.cell_factor
    xmax = float(np.max(np.abs(ref.x)))
    scale = AMP * steps * EPS
    d_atol = scale * ((m + CELL_OPS) * maxstep / factor + 3.0 * float(np.max(np.abs(ref.D))))
    x_atol = scale * (m * maxstep + (1.0 + 3.0 * R_NORM ** 2) * xmax) + 3.0 * R_NORM * xmax * d_atol
    v_atol = scale * (m + 1.0 + 3.0 * R_NORM ** 2) * ref.vnorm_max
    vd_atol = scale * (m + 1.0 + CELL_OPS) * ref.vnorm_max
    cmax, cnorm = float(np.max(np.abs(ref.c0))), float(np.sqrt(np.sum(ref.cell * ref.cell)))
    vol = abs(float(np.linalg.det(ref.cell)))
    stiffness = (2.0 * B_BULK * vol * R_NORM ** 2 + 12.0 * K_SHAPE * cnorm ** 4) / factor
    fmax_atol = 5.0 * (x_atol + 3.0 * cmax * d_atol) + stiffness * 3.0 * d_atol
    return x_atol, v_atol, d_atol, vd_atol, fmax_atol


def assert_close(driver, refs, what="", steps=None):
    """The driver (one system per entry of ``refs``, concatenated) against the restatements: ``x``, ``v``, ``D``, ``vD`` and
    ``fmax`` at the bounds of the docstring, the rest of the state exactly."""
    refs = list(refs)
    x, v = driver.positions.detach().cpu().numpy(), driver.velocities.detach().cpu().numpy()
    D, vD = driver.deform_grad.detach().cpu().numpy(), driver.cell_velocities.detach().cpu().numpy()
    cell = driver.cell.detach().cpu().numpy()
    dt, a = driver.dt.detach().cpu().numpy(), driver.a.detach().cpu().numpy()
    nsteps, conv = driver.nsteps.detach().cpu().numpy(), driver.converged.detach().cpu().numpy()
    fmax = driver.fmax.detach().cpu().numpy()
    assert len(refs) == driver.num_systems
    off, worst = 0, {"x": 0.0, "v": 0.0, "D": 0.0, "vD": 0.0}
    for s, ref in enumerate(refs):
        n = len(ref.x)
        assert float(np.linalg.norm(ref.D, 2)) <= R_NORM and float(np.linalg.norm(np.linalg.inv(ref.D), 2)) <= R_NORM, \
            f"{what}: the strain of system {s} left the range the bounds are derived for"
        x_atol, v_atol, d_atol, vd_atol, fmax_atol = bounds(ref, ref.nsteps if steps is None else steps)
        err = {"x": (float(np.max(np.abs(x[off:off + n] - ref.x))), x_atol),
               "v": (float(np.max(np.abs(v[off:off + n] - ref.v))), v_atol),
               "D": (float(np.max(np.abs(D[s] - ref.D))), d_atol), "vD": (float(np.max(np.abs(vD[s] - ref.vD))), vd_atol)}
        for name, (e, atol) in err.items():
            if ref.nsteps > 0:  # (a system that never moved has bounds of zero)
                worst[name] = max(worst[name], e / atol)
            assert e <= atol, f"{what}: {name} of system {s} off by {e:.3e}, bound {atol:.3e}"
        cell_atol = 3.0 * float(np.max(np.abs(ref.c0))) * (d_atol + 2.0 * EPS * R_NORM)
        assert float(np.max(np.abs(cell[s] - ref.cell))) <= cell_atol, f"{what}: cell of system {s}"
        assert dt[s] == ref.dt and a[s] == ref.a and nsteps[s] == ref.nsteps, \
            f"{what}: system {s} has dt {dt[s]!r} a {a[s]!r} nsteps {nsteps[s]}, restatement {ref.dt!r} {ref.a!r} {ref.nsteps}"
        assert bool(conv[s]) == ref.converged, f"{what}: verdict of system {s}"
        np.testing.assert_allclose(fmax[s], ref.fmax, rtol=16 * EPS, atol=fmax_atol, err_msg=f"{what}: fmax of system {s}")
        off += n
    assert off == x.shape[0]
    print(f"{what}: worst errors as fractions of their bounds: " + ", ".join(f"{k} {w:.3e}" for k, w in worst.items()))
