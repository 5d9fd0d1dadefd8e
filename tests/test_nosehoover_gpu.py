"""The Nose-Hoover / velocity-Verlet kernels (csrc/md.hip: nqa_md_step + nqa_md_bath) under the driver of
nequip_amd/integrations/md.py, against the float64 restatement of tests/nosehoover_restatement.py at the bound its docstring
derives (rtol 1e-10, element by element), and bit for bit against themselves.

Sizes: 1, 85, 86 and 5462 atoms are 3, 255, 258 and 16 386 flat components: a fraction of one 256-thread workgroup, one
workgroup short of one component, the first component of a second workgroup, and 65 workgroups, i.e. more rows of partial sums
than the 64 lanes of the bath kernel take one each.  Forces come from one analytic function evaluated in torch on the device
(restatement included, so that a float32 force is the same number on both sides): only the integrator is under test."""
import copy
import functools

import numpy as np
import pytest
import torch

import nosehoover_restatement as R
from nequip_amd.integrations import NoseHoover, VelocityVerlet

pytestmark = pytest.mark.gpu

DT, T = 0.5 * R.FS, 300.0


def q_of(n):
    """The bath's inertia, in proportion to the number of atoms.  The bath is driven by ``sum m v^2 - g``, which grows with N (the
    atoms start at 600 K, the target is 300 K): a fixed Q would let ``xi dt`` pass 1 at the larger sizes within a few steps, where
    ``1 + dt/2 xi`` changes sign and the scheme itself (restatement included) multiplies every rounding error.  With Q = 0.01 N,
    ``xi dt / 2`` stays near 0.1 for every size, which is the regime the derivation of the bound assumes."""
    return 0.01 * n

SIZES = (1, 85, 86, 5462)
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def driver(device, n, fdtype, backend="hip", thermostat=True, cls=NoseHoover):
    m, x, v = R.system(n, seed=n)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    if cls is VelocityVerlet:
        return cls(R.torch_force_step(fdtype), t(m), DT, t(x), t(v), remove_drift=False, backend=backend)
    return cls(R.torch_force_step(fdtype), t(m), DT, T, q_of(n), t(x), t(v), thermostat=thermostat, remove_drift=False, backend=backend)


@functools.lru_cache(maxsize=None)
def reference(device, n, fname, thermostat=True):
    """The restatement after 1 and after 25 steps (computed once per case, never modified)."""
    m, x, v = R.system(n, seed=n)
    ref = R.Restated(R.restated_force(device, DTYPES[fname]), m, DT, T, q_of(n), x, v, thermostat=thermostat)
    ref.run(1)
    one = copy.copy(ref)
    ref.run(24)
    return one, ref


def same_bits(a, b):
    return (torch.equal(a.positions, b.positions) and torch.equal(a.velocities.clone(), b.velocities.clone())
            and a.nvt_bath == b.nvt_bath and a.nsteps == b.nsteps)


@pytest.mark.parametrize("fname", sorted(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_kernels_match_the_restatement(device, n, fname):
    one, last = reference(device, n, fname)
    drv = driver(device, n, DTYPES[fname])
    assert drv.forces.dtype == DTYPES[fname] and drv._hip
    drv.step()
    R.assert_close(drv, one, f"N={n} {fname} after 1 step")
    drv.run(24)
    R.assert_close(drv, last, f"N={n} {fname} after 25 steps")
    np.testing.assert_allclose(drv.kinetic_energy, last.kinetic_energy, rtol=R.RTOL)
    np.testing.assert_allclose(drv.temperature, 2.0 * last.kinetic_energy / (3 * n * R.KB), rtol=R.RTOL)
    assert abs(drv.nvt_bath) > 1e-4  # (the bath did something)


@pytest.mark.parametrize("n", (86, 5462))
def test_thermostat_off_is_velocity_verlet(device, n):
    m, x, v = R.system(n, seed=n)
    want_x, want_v = R.velocity_verlet(R.restated_force(device), m, DT, x, v, 25)
    for drv in (driver(device, n, torch.float64, thermostat=False), driver(device, n, torch.float64, cls=VelocityVerlet)):
        drv.run(25)
        assert drv.nvt_bath == 0.0 and drv.nsteps == 25
        np.testing.assert_allclose(drv.positions.cpu().numpy(), want_x, rtol=R.RTOL, atol=0)
        np.testing.assert_allclose(drv.velocities.cpu().numpy(), want_v, rtol=R.RTOL, atol=0)
        ekin = 0.5 * float(np.sum(m[:, None] * want_v * want_v))
        np.testing.assert_allclose(drv.kinetic_energy, ekin, rtol=R.RTOL)  # (the bath launch still reports it)


@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_two_runs_give_the_same_bits_and_reading_changes_nothing(device, fname):
    a, b, c = (driver(device, 5462, DTYPES[fname]) for _ in range(3))
    a.run(25)
    b.run(25)
    for _ in range(25):
        c.step()
        c.velocities, c.temperature, c.nvt_bath, c.kinetic_energy
    assert same_bits(a, b), "two runs of the same inputs differ"
    assert same_bits(a, c), "reading velocities / temperature / nvt_bath at every step changed the trajectory"


@pytest.mark.parametrize("n", (86, 5462))
def test_state_dict_round_trip_continues_bit_for_bit(device, n):
    whole = driver(device, n, torch.float32)
    whole.run(20)
    first = driver(device, n, torch.float32)
    first.run(10)
    state = first.state_dict()
    assert state["nsteps"] == 10
    second = driver(device, n, torch.float32)
    second.run(3)
    second.set_temperature(1.0)
    second.set_timestep(2.0 * DT)
    second.load_state_dict(state)
    second.run(10)
    assert second.nsteps == 20 and same_bits(second, whole)


def test_set_temperature_and_timestep_in_mid_run(device):
    n = 258
    m, x, v = R.system(n, seed=n)
    ref = R.Restated(R.restated_force(device, torch.float32), m, DT, T, q_of(n), x, v)
    drv = driver(device, n, torch.float32)
    drv.run(5), ref.run(5)
    drv.set_temperature(900.0)
    ref.temperature = 900.0
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the temperature change")
    drv.set_timestep(0.5 * DT)
    ref.dt = 0.5 * DT
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the time-step change")


@pytest.mark.parametrize("n", (85, 5462))
def test_kernel_path_and_aten_path_agree(device, n):
    hip, aten = driver(device, n, torch.float32), driver(device, n, torch.float32, backend="aten")
    assert hip._hip and not aten._hip and aten.positions.is_cuda
    hip.run(25), aten.run(25)
    for got, want in ((hip.positions, aten.positions), (hip.velocities, aten.velocities)):
        np.testing.assert_allclose(got.cpu().numpy(), want.cpu().numpy(), rtol=R.RTOL, atol=0)
    np.testing.assert_allclose(hip.nvt_bath, aten.nvt_bath, rtol=R.RTOL)
    np.testing.assert_allclose(hip.kinetic_energy, aten.kinetic_energy, rtol=R.RTOL)
    assert hip.nsteps == aten.nsteps == 25


def test_lockstep_with_the_real_model_on_a_graphed_step(device):
    """10 steps of a water box under ``GraphedStep``.  The model's forces are not reproducible to the bit (atomic accumulation),
    so the restatement is fed, at every step, the forces the driver just obtained: the integrator alone is compared."""
    from nequip_amd.integrations.graphed_step import GraphedStep
    from nequip_amd.integrations.md import maxwell_boltzmann_velocities
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=3, seed=3)
    model = NequIPGNNModel(seed=1, model_dtype="float32", r_max=4.0, type_names=names, num_layers=2, l_max=2,
                           parity=False, num_features=16, radial_mlp_depth=1, radial_mlp_width=64,
                           avg_num_neighbors=20.0).to(device).eval()
    masses = torch.tensor([1.008, 15.999], dtype=torch.float64)[torch.as_tensor(types)]
    vel = maxwell_boltzmann_velocities(masses, 600.0, generator=torch.Generator().manual_seed(1))
    atoms = R.FakeAtoms([names[t] for t in types], pos, masses.numpy(), vel.numpy(), cell, pbc=True)
    drv = NoseHoover.from_atoms(atoms, model, DT, T, q_of(len(pos)), device=device, r_max=4.0)
    step = drv.force_step
    assert isinstance(step, GraphedStep)
    assert drv._hip and drv.forces.is_cuda  # (the forces come out in the dtype of the positions the model was handed)
    given = lambda x: drv.forces.double().cpu().numpy()  # noqa: E731
    ref = R.Restated(given, masses.numpy(), DT, T, q_of(len(pos)), pos, drv.velocities.cpu().numpy())
    for k in range(10):
        drv.step()
        ref.step(new_forces=given(None))
        R.assert_close(drv, ref, f"water box, step {k + 1}")
    assert np.isfinite(drv.potential_energy) and drv.nsteps == 10
    assert step.num_eager_fallbacks == 0
