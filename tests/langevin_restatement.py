"""What the Langevin tests share: a numpy float64 restatement of the BAOAB scheme of ``nequip_amd/integrations/md.py`` and of
its noise, written from the equations, and the comparison.  The test system, the analytic force, ``FakeAtoms`` and the constants
are those of ``nosehoover_restatement``.

One step, with the force ``F`` at the positions of the start of the step and ``F'`` at the new ones (one evaluation per step)::

    B  v1 = v + dt/2 F/m;   A  x = x + dt/2 v1;   O  v2 = c1 v1 + (c2 sqrt(kB T / m)) z;   A  x = x + dt/2 v2;   B  v' = v2 + dt/2 F'/m
    c1 = exp(-friction dt),  c2 = sqrt(1 - c1^2)   (``math.exp``, ``math.sqrt``: the bits the driver writes to its record)

The noise of flat component ``i`` (of atom ``i // 3``) at step ``s`` (the count of completed steps) with the 64-bit ``seed``::

    (w0, w1, w2, w3) = philox4x32_10(counter=(i & 0xffffffff, i >> 32, s & 0xffffffff, s >> 32), key=(seed & 0xffffffff, seed >> 32))
    u1 = ((w0 >> 5) * 67108864.0 + (w1 >> 6) + 1.0) * 2^-53;   u2 = ((w2 >> 5) * 67108864.0 + (w3 >> 6)) * 2^-53
    z  = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2)

The bounds.  The Philox words are integers: bit for bit.  ``u1``, ``u2`` and the product with 2 pi are formed by the same exactly
rounded operations on both sides; ``log`` and ``cos`` of the device library and numpy's differ by a few ulp, and with
``sqrt(-2 log u1) <= 8.6`` the normals differ by less than about 6e-15: ``NORMAL_ATOL = 1e-13``, no relative term.
Unlike Nose-Hoover, no sum over the atoms feeds back into the trajectory, so driver and restatement carry out the same float64
operations per component and differ only by that error of z, times ``c2 sqrt(kB T / m)``, accumulated over the steps: over 25 steps
at worst about 2.5e-13 of the thermal velocity ``sqrt(kB T / 1 amu)`` (the lightest mass here).  Single components come out as small
as 1e-5 of the thermal scale, so the comparison needs an absolute term: ``rtol = 1e-10`` plus ``1e-12`` Angstrom for positions
and ``1e-11 sqrt(kB T / 1 amu)`` for velocities.  The kinetic energy is a sum of N positive terms in another order (N eps) of
velocities that are off by the above: rtol 1e-10.
"""
import math

import numpy as np

from nosehoover_restatement import (  # noqa: F401  (re-exported: the tests take everything from here)
    CENTRE, FS, KB, FakeAtoms, energy_torch, force_numpy, force_torch, restated_force, system, torch_force_step, velocity_verlet)

RTOL = 1e-10
X_ATOL = 1e-12
NORMAL_ATOL = 1e-13
SEED = 20261020

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def v_atol(temperature):
    return 1e-11 * math.sqrt(KB * temperature / 1.0)


def philox4x32_10(counter, key):
    """Philox4x32-10 of Salmon et al. on arrays of 32-bit words held in ``uint64`` (a product of two words fits in 64 bits).
    ``counter``: four arrays (or integers), ``key``: two.  Returns the four output words, ``uint64`` arrays below 2^32."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) for w in counter]
    k = [int(w) for w in key]
    for r in range(10):
        if r > 0:  # the key is bumped between rounds
            k = [(k[0] + W0) & 0xFFFFFFFF, (k[1] + W1) & 0xFFFFFFFF]
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> S32, p0 & MASK, p1 >> S32, p1 & MASK
        c = [hi1 ^ c[1] ^ np.uint64(k[0]), lo1, hi0 ^ c[3] ^ np.uint64(k[1]), lo0]
    return c


def words(seed, step, count):
    """The words ``[count, 4]`` (uint64) of components ``0 .. count - 1``."""
    i = np.arange(count, dtype=np.uint64)
    full = lambda v: np.full(count, v, dtype=np.uint64)  # noqa: E731
    w = philox4x32_10((i & MASK, i >> S32, full(step & 0xFFFFFFFF), full(step >> 32)), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(w, axis=1)


def normals_of(w):
    w = np.asarray(w, dtype=np.uint64)
    u1 = ((w[:, 0] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[:, 1] >> np.uint64(6)).astype(np.float64) + 1.0) * 2.0 ** -53
    u2 = ((w[:, 2] >> np.uint64(5)).astype(np.float64) * 67108864.0 + (w[:, 3] >> np.uint64(6)).astype(np.float64)) * 2.0 ** -53
    assert u1.min(initial=1.0) > 0.0 and u1.max(initial=1.0) <= 1.0 and u2.min(initial=0.0) >= 0.0 and u2.max(initial=0.0) < 1.0
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def noise(seed, step, count):
    return normals_of(words(seed, step, count))


class Restated:
    """Float64 numpy BAOAB with the last line undeferred.  ``force(x [N, 3]) -> F [N, 3]``."""

    def __init__(self, force, masses, dt, temperature, friction, x, v, seed=0, nsteps=0):
        self.force, self.m = force, np.asarray(masses, dtype=np.float64).copy()
        self.dt, self.temperature, self.friction, self.seed = float(dt), float(temperature), float(friction), int(seed)
        self.x, self.v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
        self.nsteps = nsteps
        self.f = np.asarray(self.force(self.x), dtype=np.float64)

    def step(self, new_forces=None):
        """``new_forces``: the force at the new positions, where the caller has it (lockstep runs); else ``force`` is asked."""
        m, hdt = self.m[:, None], 0.5 * self.dt
        c1 = math.exp(-self.friction * self.dt)
        c2 = math.sqrt(1.0 - c1 * c1)
        z = noise(self.seed, self.nsteps, 3 * len(self.m)).reshape(-1, 3)
        v1 = self.v + hdt * (self.f / m)
        x = self.x + hdt * v1
        v2 = c1 * v1 + (c2 * np.sqrt(KB * self.temperature / m)) * z
        self.x = x + hdt * v2
        self.f = np.asarray(self.force(self.x) if new_forces is None else new_forces, dtype=np.float64)
        self.v = v2 + hdt * (self.f / m)
        self.nsteps += 1

    def run(self, n):
        for _ in range(n):
            self.step()

    @property
    def kinetic_energy(self):
        return 0.5 * float(np.sum(self.m[:, None] * self.v * self.v))

    @property
    def kinetic_temperature(self):
        return 2.0 * self.kinetic_energy / (3 * len(self.m) * KB)


def assert_close(driver, restated, what="", temperature=300.0):
    """Positions, completed velocities, kinetic energy, temperature and step count of the driver against the restatement.
    ``temperature``: the largest target of the run so far, which sets the thermal scale of the velocities' absolute term."""
    x = driver.positions.detach().cpu().numpy()
    v = driver.velocities.detach().cpu().numpy()
    ex, ev = float(np.max(np.abs(x - restated.x))), float(np.max(np.abs(v - restated.v)))
    ekin, temp = driver.kinetic_energy, driver.temperature
    print(f"{what}: worst absolute error of x {ex:.3e} A, of v {ev:.3e} (thermal scale {v_atol(temperature) * 1e11:.3e}); "
          f"Ekin {ekin!r} against {restated.kinetic_energy!r}")
    np.testing.assert_allclose(x, restated.x, rtol=RTOL, atol=X_ATOL, err_msg=f"{what}: positions")
    np.testing.assert_allclose(v, restated.v, rtol=RTOL, atol=v_atol(temperature), err_msg=f"{what}: velocities")
    np.testing.assert_allclose(ekin, restated.kinetic_energy, rtol=RTOL, atol=0, err_msg=f"{what}: kinetic energy")
    np.testing.assert_allclose(temp, restated.kinetic_temperature, rtol=RTOL, atol=0, err_msg=f"{what}: temperature")
    assert driver.nsteps == restated.nsteps, what
