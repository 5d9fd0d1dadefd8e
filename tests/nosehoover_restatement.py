"""What the Nose-Hoover tests share: a numpy float64 restatement of the scheme of ``nequip_amd/integrations/md.py`` (the
arithmetic of ``nequip/ase/nosehoover.py``, written out anew), the analytic test force and the comparison.

One step, with the force ``F`` at the positions of the start of the step and ``F'`` at the new ones (one evaluation per step:
the next step starts from ``F'``)::

    a = F/m - xi v;  x' = x + dt v + dt^2/2 a;  v_half = v + dt/2 a
    xi_half = xi + dt/2 (sum m v^2 - g)/(2 Q);  xi' = xi_half + dt/2 (sum m v_half^2 - g)/(2 Q);  g = (3N + 1) kB T
    v' = (v_half + dt/2 F'/m) / (1 + dt/2 xi')

The bound.  Driver and restatement carry out the same float64 operations element by element; only the two sums over the atoms
are added in another order.  A sum of N terms of one sign is off by at most about N eps relative (eps = 2^-53), that error enters
xi once per step and from there, times dt, every velocity and position: about N eps per step, growing linearly.  For the largest
case here (N = 5462, 25 steps) that is 1.5e-11 at the very worst and 1e-13 for the 7-atom CPU case; observed errors are at the
level of eps, since rounding errors do not all point the same way.  ``RTOL = 1e-10`` is the figure the tests hold, element by
element with no absolute term.
"""
import numpy as np
import torch

RTOL = 1e-10

# CODATA 2014 (the values behind ase.units), written out independently of the module under test
E_CHARGE, AMU, K_BOLTZMANN = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
KB = K_BOLTZMANN / E_CHARGE
FS = 1e-5 * np.sqrt(E_CHARGE / AMU)


class Restated:
    """Float64 numpy Nose-Hoover (``thermostat=False``: velocity Verlet).  ``force(x [N, 3]) -> F [N, 3]``."""

    def __init__(self, force, masses, dt, temperature, q, x, v, thermostat=True, dof_extra=1):
        self.force, self.m = force, np.asarray(masses, dtype=np.float64).copy()
        self.dt, self.temperature, self.q, self.thermostat = float(dt), float(temperature), float(q), thermostat
        self.x, self.v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
        self.xi, self.nsteps, self.dof_extra = 0.0, 0, dof_extra
        self.f = np.asarray(self.force(self.x), dtype=np.float64)

    def step(self, new_forces=None):
        """``new_forces``: the force at the new positions, where the caller has it (lockstep runs); else ``force`` is asked."""
        m, dt = self.m[:, None], self.dt
        g = (3 * len(self.m) + self.dof_extra) * KB * self.temperature
        a = self.f / m - self.xi * self.v
        x_new = self.x + dt * self.v + 0.5 * dt * dt * a
        v_half = self.v + 0.5 * dt * a
        if self.thermostat:
            xi_half = self.xi + 0.5 * dt * (0.5 * (np.sum(m * self.v * self.v) - g)) / self.q
            self.xi = xi_half + 0.5 * dt * (0.5 * (np.sum(m * v_half * v_half) - g)) / self.q
        self.x = x_new
        self.f = np.asarray(self.force(self.x) if new_forces is None else new_forces, dtype=np.float64)
        self.v = (v_half + 0.5 * dt * self.f / m) / (1.0 + 0.5 * dt * self.xi)
        self.nsteps += 1

    def run(self, n):
        for _ in range(n):
            self.step()

    @property
    def kinetic_energy(self):
        return 0.5 * float(np.sum(self.m[:, None] * self.v * self.v))


def velocity_verlet(force, masses, dt, x, v, n):
    """Plain velocity Verlet, written without any bath variable: ``(x, v)`` after ``n`` steps."""
    m = np.asarray(masses, dtype=np.float64)[:, None]
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    f = np.asarray(force(x), dtype=np.float64)
    for _ in range(n):
        v_half = v + 0.5 * dt * f / m
        x = x + dt * v_half
        f = np.asarray(force(x), dtype=np.float64)
        v = v_half + 0.5 * dt * f / m
    return x, v


# ---- the analytic force: a harmonic well about CENTRE plus a harmonic term between every pair of atoms ------------------------
K_WELL, CENTRE = 2.0, (0.3, -0.2, 0.1)


def pair_constant(n):
    return 0.5 / n


def force_numpy(x):
    n = x.shape[0]
    return -K_WELL * (x - np.asarray(CENTRE)) - pair_constant(n) * (n * x - x.sum(0))


def force_torch(x):
    """The same function on the tensor's device (float64)."""
    n = x.shape[0]
    centre = torch.tensor(CENTRE, dtype=torch.float64, device=x.device)
    return -K_WELL * (x - centre) - pair_constant(n) * (n * x - x.sum(0))


def energy_torch(x):
    n = x.shape[0]
    centre = torch.tensor(CENTRE, dtype=torch.float64, device=x.device)
    # sum over pairs of k/2 |xi - xj|^2 = k/2 (n sum |x|^2 - |sum x|^2)
    return 0.5 * K_WELL * ((x - centre) ** 2).sum() + 0.5 * pair_constant(n) * (n * (x * x).sum() - (x.sum(0) ** 2).sum())


def torch_force_step(force_dtype=torch.float64):
    """A ``force_step`` for the driver: forces rounded to ``force_dtype``."""

    def step(pos):
        return {"forces": force_torch(pos).to(force_dtype), "total_energy": energy_torch(pos).reshape(1, 1)}

    return step


def restated_force(device, force_dtype=torch.float64):
    """The force callback of the restatement that rounds like ``torch_force_step``: evaluated by the same function on the same
    device, so that a float32 force is the same float32 number on both sides."""

    def force(x):
        f = force_torch(torch.from_numpy(np.ascontiguousarray(x)).to(device)).to(force_dtype)
        return f.double().cpu().numpy()

    return force


def system(n, seed=0, temperature=600.0):
    """``n`` atoms of unequal mass around the well, Maxwell-Boltzmann velocities at ``temperature``: (masses, x, v) in numpy."""
    rng = np.random.default_rng(seed)
    masses = rng.uniform(1.0, 16.0, size=n)
    x = np.asarray(CENTRE) + rng.normal(size=(n, 3))
    v = rng.normal(size=(n, 3)) * np.sqrt(KB * temperature / masses)[:, None]
    return masses, x, v


def assert_close(driver, restated, what=""):
    """Positions, completed velocities and the bath variable of the driver against the restatement, element by element."""
    x = driver.positions.detach().cpu().numpy()
    v = driver.velocities.detach().cpu().numpy()
    worst = max(float(np.max(np.abs(x - restated.x) / np.abs(restated.x))), float(np.max(np.abs(v - restated.v) / np.abs(restated.v))))
    print(f"{what}: worst relative error of x, v {worst:.3e}; xi {driver.nvt_bath!r} against {restated.xi!r}")
    np.testing.assert_allclose(x, restated.x, rtol=RTOL, atol=0, err_msg=f"{what}: positions")
    np.testing.assert_allclose(v, restated.v, rtol=RTOL, atol=0, err_msg=f"{what}: velocities")
    np.testing.assert_allclose(driver.nvt_bath, restated.xi, rtol=RTOL, atol=0, err_msg=f"{what}: xi")
    assert driver.nsteps == restated.nsteps, what


class FakeAtoms:
    """The ``Atoms`` accessors the driver uses (ASE is not a dependency of the tests)."""

    def __init__(self, symbols, positions, masses, velocities=None, cell=None, pbc=False):
        self._s, self._p, self._m = list(symbols), np.array(positions, dtype=np.float64), np.array(masses, dtype=np.float64)
        self._v = None if velocities is None else np.array(velocities, dtype=np.float64)
        self._c = np.zeros((3, 3)) if cell is None else np.asarray(cell, dtype=np.float64)
        self._pbc = np.array([pbc] * 3, dtype=bool)

    def get_chemical_symbols(self):
        return self._s

    def get_positions(self):
        return self._p.copy()

    def get_velocities(self):
        return None if self._v is None else self._v.copy()

    def get_masses(self):
        return self._m.copy()

    def get_cell(self):
        return self._c

    def get_pbc(self):
        return self._pbc

    def set_positions(self, p):
        self._p = np.array(p, dtype=np.float64)

    def set_velocities(self, v):
        self._v = np.array(v, dtype=np.float64)
