"""The Langevin kernels (csrc/md.hip: nqa_md_langevin_step + nqa_md_bath, and the generator alone through nqa_md_noise) under the
driver of nequip_amd/integrations/md.py, against the float64 restatement of tests/langevin_restatement.py at the bounds its
docstring derives, and bit for bit against themselves.

Sizes: 1, 85, 86 and 5462 atoms are 3, 255, 258 and 16 386 flat components: a fraction of one 256-thread workgroup, one
workgroup short of one component, the first component of a second workgroup, and 65 workgroups, i.e. more rows of partial sums
than the 64 lanes of the bath kernel take one each.  Forces come from one analytic function evaluated in torch on the device
(restatement included, so that a float32 force is the same number on both sides): only the integrator is under test."""
import copy
import functools

import numpy as np
import pytest
import torch

import langevin_restatement as R
from nequip_amd.integrations import Langevin, langevin_noise

pytestmark = pytest.mark.gpu

DT, T = 0.5 * R.FS, 300.0
FRICTION = 0.01 / R.FS
SIZES = (1, 85, 86, 5462)
DTYPES = {"f32": torch.float32, "f64": torch.float64}


def driver(device, n, fdtype, backend="hip", friction=FRICTION, seed=R.SEED):
    m, x, v = R.system(n, seed=n)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return Langevin(R.torch_force_step(fdtype), t(m), DT, T, friction, t(x), t(v), seed=seed, backend=backend)


@functools.lru_cache(maxsize=None)
def reference(device, n, fname):
    """The restatement after 1 and after 25 steps (computed once per case, never modified)."""
    m, x, v = R.system(n, seed=n)
    ref = R.Restated(R.restated_force(device, DTYPES[fname]), m, DT, T, FRICTION, x, v, seed=R.SEED)
    ref.run(1)
    one = copy.copy(ref)
    ref.run(24)
    return one, ref


def same_bits(a, b):
    return (torch.equal(a.positions, b.positions) and torch.equal(a.velocities.clone(), b.velocities.clone())
            and a.kinetic_energy == b.kinetic_energy and a.nsteps == b.nsteps)


# ---- the generator ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed, step", [(0, 0), (R.SEED, 7), (2 ** 32 + 7, 3), (R.SEED, 2 ** 32), (2 ** 64 - 1, 2 ** 64 - 1)])
def test_noise_kernel_matches_the_restatement(device, seed, step):
    for count in (1, 255, 256, 257, 16386):
        z, w = langevin_noise(seed, step, count, device, return_words=True)
        assert z.is_cuda and z.shape == (count,) and w.shape == (count, 4)
        want = R.words(seed, step, count)
        assert np.array_equal(w.cpu().numpy().astype(np.uint64), want), f"Philox words, count {count}"
        zw = R.normals_of(want)
        print(f"seed {seed} step {step} count {count}: worst error of the normals {np.max(np.abs(z.cpu().numpy() - zw)):.3e}")
        np.testing.assert_allclose(z.cpu().numpy(), zw, rtol=0, atol=R.NORMAL_ATOL)
        # the normals alone (no words asked for) are the same bits
        assert torch.equal(langevin_noise(seed, step, count, device), z)
    if (seed, step) == (0, 0):  # Random123's known answer for counter 0, key 0
        assert w[0].tolist() == [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]


def test_noise_entry_refusals(device):
    from nequip_amd import _lib as L

    lib = L.load()
    z = torch.zeros(4, dtype=torch.float64, device=device)
    stream = L.stream_ptr(device)
    assert lib.nqa_md_noise(0, 0, 0, None, L.ptr(z), stream) != 0 and b"count" in lib.nqa_last_error()
    assert lib.nqa_md_noise(0, 0, 4, None, None, stream) != 0 and b"words or normals" in lib.nqa_last_error()
    drv = driver(device, 3, torch.float64)
    args = lambda mode, par: (L.NQA_F64, L.ptr(drv.forces), L.ptr(drv._m), L.ptr(drv._pos), L.ptr(drv._vel),  # noqa: E731
                              L.ptr(drv._vel_out), 3, L.ptr(drv._rec), par, L.ptr(drv._partials), mode, stream)
    assert lib.nqa_md_langevin_step(*args(2, L.ptr(drv._par))) != 0 and b"mode bits" in lib.nqa_last_error()
    assert lib.nqa_md_langevin_step(*args(0, None)) != 0 and b"params" in lib.nqa_last_error()
    torch.cuda.synchronize()
    assert drv.nsteps == 0  # (nothing ran)


# ---- the step ---------------------------------------------------------------------------------------------------------------------
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
    assert drv.nsteps == 25


@pytest.mark.parametrize("n", (86, 5462))
def test_friction_zero_is_velocity_verlet(device, n):
    m, x, v = R.system(n, seed=n)
    want_x, want_v = R.velocity_verlet(R.restated_force(device), m, DT, x, v, 25)
    drv = driver(device, n, torch.float64, friction=0.0)
    drv.run(25)
    assert drv.nsteps == 25
    np.testing.assert_allclose(drv.positions.cpu().numpy(), want_x, rtol=R.RTOL, atol=0)
    np.testing.assert_allclose(drv.velocities.cpu().numpy(), want_v, rtol=R.RTOL, atol=0)
    ekin = 0.5 * float(np.sum(m[:, None] * want_v * want_v))
    np.testing.assert_allclose(drv.kinetic_energy, ekin, rtol=R.RTOL)


@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_two_runs_give_the_same_bits_and_reading_changes_nothing(device, fname):
    a, b, c = (driver(device, 5462, DTYPES[fname]) for _ in range(3))
    a.run(25)
    b.run(25)
    for _ in range(25):
        c.step()
        c.velocities, c.temperature, c.kinetic_energy, c.potential_energy, c.nsteps
    assert same_bits(a, b), "two runs of the same inputs differ"
    assert same_bits(a, c), "reading velocities / temperature / kinetic_energy at every step changed the trajectory"
    other = driver(device, 5462, DTYPES[fname], seed=R.SEED + 1)
    other.run(25)
    assert not torch.equal(other.positions, a.positions)  # (the seed matters)


@pytest.mark.parametrize("n", (86, 5462))
def test_state_dict_round_trip_continues_bit_for_bit(device, n):
    whole = driver(device, n, torch.float32)
    whole.run(20)
    first = driver(device, n, torch.float32)
    first.run(10)
    state = first.state_dict()
    assert state["nsteps"] == 10 and state["seed"] == R.SEED
    second = driver(device, n, torch.float32, seed=5)
    second.run(3)
    second.set_temperature(1.0)
    second.set_friction(3.0 * FRICTION)
    second.set_timestep(2.0 * DT)
    second.load_state_dict(state)
    second.run(10)
    assert second.nsteps == 20 and same_bits(second, whole)


def test_set_temperature_friction_and_timestep_in_mid_run(device):
    n = 258
    m, x, v = R.system(n, seed=n)
    ref = R.Restated(R.restated_force(device, torch.float32), m, DT, T, FRICTION, x, v, seed=R.SEED)
    drv = driver(device, n, torch.float32)
    drv.run(5), ref.run(5)
    drv.set_temperature(900.0)
    ref.temperature = 900.0
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the temperature change")
    drv.set_friction(7.0 * FRICTION)
    ref.friction = 7.0 * FRICTION
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the friction change")
    drv.set_timestep(0.5 * DT)
    ref.dt = 0.5 * DT
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the time-step change")


@pytest.mark.parametrize("n", (85, 5462))
def test_kernel_path_and_aten_path_agree(device, n):
    hip, aten = driver(device, n, torch.float32), driver(device, n, torch.float32, backend="aten")
    assert hip._hip and not aten._hip and aten.positions.is_cuda
    hip.run(25), aten.run(25)
    np.testing.assert_allclose(hip.positions.cpu().numpy(), aten.positions.cpu().numpy(), rtol=R.RTOL, atol=R.X_ATOL)
    np.testing.assert_allclose(hip.velocities.cpu().numpy(), aten.velocities.cpu().numpy(), rtol=R.RTOL, atol=R.v_atol(T))
    np.testing.assert_allclose(hip.kinetic_energy, aten.kinetic_energy, rtol=R.RTOL)
    assert hip.nsteps == aten.nsteps == 25


def test_a_captured_step_draws_fresh_noise_at_every_replay(device):
    """The step's two launches captured once (a linear graph), the forces in a static buffer that an eager force call refreshes
    between replays: five replays are five eager steps of a twin, bit for bit.  The step count, and with it the noise, lives in
    the device record, so nothing of it is frozen into the graph."""
    n = 5462
    twin = driver(device, n, torch.float64)
    twin.run(5)  # (first, so that the kernels are loaded before anything is captured)
    drv = driver(device, n, torch.float64)
    force = R.torch_force_step(torch.float64)
    static_forces = drv.forces.clone()
    drv._forces = static_forces
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        drv._launch(finish_only=False)
    assert drv.nsteps == 0  # (capturing ran nothing)
    for _ in range(5):
        graph.replay()
        static_forces.copy_(force(drv.positions)["forces"])
    torch.cuda.synchronize()
    assert drv.nsteps == 5
    assert same_bits(drv, twin)


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
    drv = Langevin.from_atoms(atoms, model, DT, T, FRICTION, device=device, r_max=4.0, seed=R.SEED)
    step = drv.force_step
    assert isinstance(step, GraphedStep)
    assert drv._hip and drv.forces.is_cuda
    given = lambda x: drv.forces.double().cpu().numpy()  # noqa: E731
    ref = R.Restated(given, masses.numpy(), DT, T, FRICTION, pos, drv.velocities.cpu().numpy(), seed=R.SEED)
    for k in range(10):
        drv.step()
        ref.step(new_forces=given(None))
        R.assert_close(drv, ref, f"water box, step {k + 1}")
    assert np.isfinite(drv.potential_energy) and drv.nsteps == 10
    assert step.num_eager_fallbacks == 0
