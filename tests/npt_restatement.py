"""What the LangevinNPT tests share: a numpy float64 restatement of the scheme of ``nequip_amd.integrations.LangevinNPT`` and
``csrc/md.hip`` (``nqa_md_langevin_step`` + ``nqa_md_npt_bath`` + ``nqa_md_npt_scale``), written from the equations, the test
system and the comparison.  The Philox functions are those of ``langevin_restatement``, the analytic potential (tethered sites +
bulk + shape energy, with its exact forces and stress; the bulk term restores the volume, so one atom is stable) is the one of
``cell_fire_restatement``, masses and velocities come from ``nosehoover_restatement.system``.

One step.  ``F`` and ``sigma`` are the force and the stress ((1/V) dE/d(strain)) at ``(x, C)``, ``C`` the cell (rows are the
lattice vectors), ``s`` the count of completed steps, ``a = compressibility dt / taup``, ``hdt = dt / 2``::

    B  v1 = v + hdt F/m;   A  x' = x + hdt v1;   O  v2 = c1 v1 + (c2 sqrt(kB T / m)) z;   A  x' = x' + hdt v2
    K  = 1/2 sum m v^2  (the completed velocities of the START of the step);   V = |det C|  (cofactors along the first row)
    P  = (2 K) / (3 V) - (sigma_00 + sigma_11 + sigma_22) / 3
    xi = noise(seed, s, 3N + 1)[3N]                              (z are the components 0 .. 3N - 1 of the same call)
    d_eps = -a (p0 - P) + sqrt((2 kB T a) / V) xi;   mu = exp(d_eps / 3)
    C = mu C;   x = mu x';   v2 = v2 / mu;   then F', sigma' at (x, C) and   B  v' = v2 + hdt F'/m

The bounds.  Everything ``langevin_restatement`` derives for the atoms' part carries over: per component the same float64
operations on both sides, the normals off by ``NORMAL_ATOL``, hence ``RTOL = 1e-10`` plus ``X_ATOL = 1e-12`` Angstrom for
positions and ``1e-11 sqrt(kB T / 1 amu)`` for velocities.  New here is that a sum over the atoms feeds back into the trajectory,
through ``mu``:

* ``K`` is a sum of N positive terms in another order: off by ``N eps`` relative (eps = 2^-53).
* ``P``: its kinetic part ``Pkin = 2K / 3V`` is off by ``Pkin N eps`` (plus three roundings); the determinant is five roundings.
* ``mu``: ``d_eps`` is off by ``a`` times the error of ``P``, the noise term by a few ulp of itself (``sqrt``, the quotient, and
  ``xi`` off by ``NORMAL_ATOL``, times ``sqrt(2 kT a / V)`` which is below 0.01 here), and ``exp`` of the device library and
  numpy's differ by an ulp or two of ``mu``:  ``|d mu| / mu <= (a / 3) N eps Pkin + MU_OPS eps`` per step with ``MU_OPS = 8``.
* That error multiplies the cell, every position and (inverted) every velocity, once per step, and accumulates.  It returns
  through the stress and the forces at the displaced state, but the loop gain is small: ``a / 3`` times the stiffness
  ``dP / d(strain)`` (some tens of eV/A^3 at the most crowded case) is about 0.1 per step, and the time step times the largest
  spring constant over the smallest mass is 0.14; ``AMP = 8``, the factor ``fire_restatement`` allows for the same reason, covers
  the transient growth over the 25 (CPU: up to 200, with ``a (dP / d strain) = 0``) steps compared here.

With ``Pkin`` the largest kinetic pressure of the reference run, relative for the cell and added to the Langevin bounds for the
atoms (``xmax``, ``vmax``: the largest components of the reference)::

    cell_rtol = AMP steps eps ((a / 3) N Pkin + MU_OPS)
    x_atol    = X_ATOL + cell_rtol xmax
    v_atol    = 1e-11 sqrt(kB T) + cell_rtol vmax + steps dt K_EFF x_atol       (K_EFF = 2.8 / 1 amu: the stiffest spring, the
                                                                                  lightest mass, as in cell_fire_restatement)
    K         rtol = RTOL  (N eps and twice the relative error of v are both far below it)
    P         atol = Pkin (N eps + 5 cell_rtol + RTOL) + stress_atol
    stress_atol = (3 K_EFF dmax N / V) (x_atol + 3 cmax cell_rtol) + (2 B V / V0 + 12 K_shape ||C||_F^4 / V) 3 cell_rtol

(the stress at a state that is off by the above: the site dyads ``sum w d (x) d / V`` with ``|d| <= dmax`` and ``w <= K_EFF``,
and the stiffness of the bulk and shape terms as ``cell_fire_restatement`` bounds it).  ``nsteps`` is compared exactly.

Float32 forces and stress are rounded by the same torch function on the same device on both sides, from inputs that agree to
about 1e-13 relative; that such a difference flips a float32 rounding has a probability of about 1e-6 per value and is, as in
``langevin_restatement``, not part of the bounds (the seeds are fixed, so a case either meets one or never does).
"""
import copy
import math

import numpy as np
import torch

import cell_fire_restatement as C
import langevin_restatement as L
from langevin_restatement import FS, KB, RTOL, SEED, X_ATOL, FakeAtoms  # noqa: F401  (re-exported)

EPS = 2.0 ** -53
AMP = 8.0
MU_OPS = 8.0
K_EFF = 2.8

# CODATA 2014, written out independently of the module under test
GPA = 1e-21 / 1.6021766208e-19
BAR = 1e-25 / 1.6021766208e-19


def det3(c):
    """``_det3`` of cell_fire_restatement for one ``[3, 3]`` matrix."""
    return float(C._det3(np.asarray(c, dtype=np.float64)[None])[0])


def noise_table(seed, first_step, steps, count):
    """``[steps, count]``: ``noise(seed, s, count)`` for ``s = first_step .. first_step + steps - 1`` in one vectorised call (the
    same functions on the same counters: the same bits)."""
    i = np.tile(np.arange(count, dtype=np.uint64), steps)
    s = np.repeat(np.arange(first_step, first_step + steps, dtype=np.uint64), count)
    w = L.philox4x32_10((i & L.MASK, i >> L.S32, s & L.MASK, s >> L.S32), (seed & 0xFFFFFFFF, seed >> 32))
    return L.normals_of(np.stack(w, axis=1)).reshape(steps, count)


class Restated:
    """Float64 numpy NPT with the closing B undeferred.  ``force(x [N, 3], C [3, 3]) -> (F [N, 3], sigma [3, 3])``."""

    def __init__(self, force, masses, dt, temperature, friction, pressure, compressibility, taup, x, cell, v, seed=0, nsteps=0,
                 table=None):
        self.force, self.m = force, np.asarray(masses, dtype=np.float64).copy()
        self.dt, self.temperature, self.friction, self.seed = float(dt), float(temperature), float(friction), int(seed)
        self.p0, self.compressibility, self.taup = float(pressure), float(compressibility), float(taup)
        self.x, self.v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
        self.cell = np.array(cell, dtype=np.float64).reshape(3, 3)
        self.nsteps, self.table = nsteps, table
        self.mu, self.pressure, self.ekin, self.pkin_max = 1.0, 0.0, 0.0, 0.0
        self.f, self.sigma = (np.asarray(a, dtype=np.float64) for a in self.force(self.x, self.cell))

    def step(self, new_forces=None):
        """``new_forces``: ``(F, sigma)`` at the new state, where the caller has them (lockstep runs); else ``force`` is asked."""
        m, hdt, n3 = self.m[:, None], 0.5 * self.dt, 3 * len(self.m)
        kt = KB * self.temperature
        c1 = math.exp(-self.friction * self.dt)
        c2 = math.sqrt(1.0 - c1 * c1)
        a = self.compressibility * self.dt / self.taup
        zs = L.noise(self.seed, self.nsteps, n3 + 1) if self.table is None else self.table[self.nsteps]
        z, xi = zs[:n3].reshape(-1, 3), float(zs[n3])
        # the thermostat's part
        ekin = 0.5 * float(np.sum(m * self.v * self.v))
        v1 = self.v + hdt * (self.f / m)
        x = self.x + hdt * v1
        v2 = c1 * v1 + (c2 * np.sqrt(kt / m)) * z
        x = x + hdt * v2
        # the barostat
        vol = abs(det3(self.cell))
        s = self.sigma
        p = (2.0 * ekin) / (3.0 * vol) - (s[0, 0] + s[1, 1] + s[2, 2]) / 3.0
        d_eps = -a * (self.p0 - p) + math.sqrt((2.0 * kt * a) / vol) * xi
        mu = math.exp(d_eps / 3.0)
        assert math.isfinite(mu) and vol > 0.0
        self.cell = mu * self.cell
        self.x = mu * x
        v2 = v2 / mu
        self.mu, self.pressure, self.ekin = mu, p, ekin
        self.pkin_max = max(self.pkin_max, (2.0 * ekin) / (3.0 * vol))
        f, sigma = self.force(self.x, self.cell) if new_forces is None else new_forces
        self.f, self.sigma = np.asarray(f, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
        self.v = v2 + hdt * (self.f / m)
        self.nsteps += 1

    def run(self, n):
        for _ in range(n):
            self.step()

    def snapshot(self):
        return copy.copy(self)

    @property
    def volume(self):
        return abs(det3(self.cell))

    @property
    def kinetic_energy(self):
        return 0.5 * float(np.sum(self.m[:, None] * self.v * self.v))


# ---- the test system -------------------------------------------------------------------------------------------------------------
def site_case(n):
    """``(part, masses, x, cell, v)``: the tethered-site system of ``n`` atoms (seed ``n``) with the masses and the 600 K
    velocities of ``nosehoover_restatement.system``."""
    part = C.site_system(n, seed=n)
    masses, _, v = L.system(n, seed=n)
    return part, masses, part["x"], part["c0"], v


def zero_force_numpy(x, cell):
    return np.zeros_like(x), np.zeros((3, 3))


def zero_force_step(pos, cell):
    return {"forces": torch.zeros_like(pos), "total_energy": torch.zeros(1, 1, dtype=pos.dtype, device=pos.device),
            "stress": torch.zeros(1, 3, 3, dtype=pos.dtype, device=pos.device)}


# ---- the comparison --------------------------------------------------------------------------------------------------------------
def bounds(ref, steps, temperature, part=None):
    """``dict(cell_rtol, x_atol, v_atol, p_atol)`` of the docstring for the run of ``ref`` over ``steps`` steps; ``part``: the
    site system behind the stress (None: no stress, as for the ideal gas)."""
    n = len(ref.m)
    a = ref.compressibility * ref.dt / ref.taup
    cell_rtol = AMP * steps * EPS * ((a / 3.0) * n * ref.pkin_max + MU_OPS)
    x_atol = X_ATOL + cell_rtol * float(np.max(np.abs(ref.x)))
    v_atol = L.v_atol(temperature) + cell_rtol * float(np.max(np.abs(ref.v))) + steps * ref.dt * K_EFF * x_atol
    stress_atol = 0.0
    if part is not None:
        vol, cmax = ref.volume, float(np.max(np.abs(ref.cell)))
        d = ref.x - part["s0"] @ ref.cell
        dmax = float(np.max(np.sqrt(np.sum(d * d, axis=1))))
        cnorm = float(np.sqrt(np.sum(ref.cell * ref.cell)))
        stress_atol = ((3.0 * K_EFF * dmax * n / vol) * (x_atol + 3.0 * cmax * cell_rtol)
                       + (2.0 * C.B_BULK * vol / part["v0"] + 12.0 * C.K_SHAPE * cnorm ** 4 / vol) * 3.0 * cell_rtol)
    p_atol = ref.pkin_max * (n * EPS + 5.0 * cell_rtol + RTOL) + stress_atol
    return dict(cell_rtol=cell_rtol, x_atol=x_atol, v_atol=v_atol, p_atol=p_atol)


def assert_close(driver, ref, what="", temperature=300.0, part=None, steps=None):
    """``x``, completed ``v``, ``C``, ``K``, ``P`` and ``nsteps`` of the driver against the restatement; prints the worst
    error next to each bound."""
    b = bounds(ref, ref.nsteps if steps is None else steps, temperature, part)
    x = driver.positions.detach().cpu().numpy()
    v = driver.velocities.detach().cpu().numpy()
    cell = driver.cell.detach().cpu().numpy().reshape(3, 3)
    ekin, p = driver.kinetic_energy, driver.pressure
    ex, ev = float(np.max(np.abs(x - ref.x))), float(np.max(np.abs(v - ref.v)))
    ec = float(np.max(np.abs(cell - ref.cell) / np.maximum(np.abs(ref.cell), 1e-300)))
    ek = abs(ekin - ref.kinetic_energy) / max(ref.kinetic_energy, 1e-300)
    print(f"{what}: x off by {ex:.3e} (atol {b['x_atol']:.3e} + rtol {RTOL:.0e}), v by {ev:.3e} (atol {b['v_atol']:.3e} + rtol "
          f"{RTOL:.0e}), cell by {ec:.3e} relative (bound {b['cell_rtol']:.3e}), K by {ek:.3e} relative (bound {RTOL:.0e}), "
          f"P by {abs(p - ref.pressure):.3e} (bound {b['p_atol']:.3e})")
    np.testing.assert_allclose(x, ref.x, rtol=RTOL, atol=b["x_atol"], err_msg=f"{what}: positions")
    np.testing.assert_allclose(v, ref.v, rtol=RTOL, atol=b["v_atol"], err_msg=f"{what}: velocities")
    np.testing.assert_allclose(cell, ref.cell, rtol=b["cell_rtol"], atol=0, err_msg=f"{what}: cell")
    np.testing.assert_allclose(ekin, ref.kinetic_energy, rtol=RTOL, atol=0, err_msg=f"{what}: kinetic energy")
    np.testing.assert_allclose(p, ref.pressure, rtol=0, atol=b["p_atol"], err_msg=f"{what}: pressure")
    np.testing.assert_allclose(driver.volume, ref.volume, rtol=3.0 * b["cell_rtol"] + 8 * EPS, atol=0, err_msg=f"{what}: volume")
    assert driver.nsteps == ref.nsteps, what
