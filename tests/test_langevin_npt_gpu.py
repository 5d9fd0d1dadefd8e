"""The NPT kernels (csrc/md.hip: nqa_md_langevin_step + nqa_md_npt_bath + nqa_md_npt_scale) under the driver of
nequip_amd/integrations/md.py (LangevinNPT), against the float64 restatement of tests/npt_restatement.py at the bounds its
docstring derives, and bit for bit against themselves and against Langevin.

Sizes: 1, 85, 86 and 5462 atoms are 3, 255, 258 and 16 386 flat components: a fraction of one 256-thread workgroup, one
workgroup short of one component, the first component of a second workgroup, and 65 workgroups, i.e. more rows of partial sums
than the 64 lanes of the bath wavefront take one each.  Forces and stress come from one analytic function evaluated in torch on
the device (restatement included, so that a float32 value is the same number on both sides): only the integrator is under test."""
import functools
import math

import numpy as np
import pytest
import torch

import cell_fire_restatement as C
import langevin_restatement as LR
import npt_restatement as R
from nequip_amd.integrations import Langevin, LangevinNPT, langevin_noise
from nequip_amd.integrations import md as M

pytestmark = pytest.mark.gpu

DT, T = 0.5 * R.FS, 300.0
FRICTION = 0.01 / R.FS
# a stiff barostat: a = compressibility dt / taup = 0.01 against pressures of 0.1 to a few eV/A^3 moves the cell by parts in a
# thousand per step
P0, COMPRESSIBILITY, TAUP = 0.01, 0.5, 50.0 * DT
SIZES = (1, 85, 86, 5462)
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@functools.lru_cache(maxsize=None)
def case(n):
    return R.site_case(n)


def driver(device, n, fdtype, backend="hip", compressibility=COMPRESSIBILITY, seed=R.SEED, friction=FRICTION, pressure=P0):
    part, m, x, cell, v = case(n)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return LangevinNPT(C.torch_force_step([part], device, fdtype), t(m), DT, T, friction, pressure, compressibility, TAUP, t(x),
                       t(cell), t(v), seed=seed, backend=backend)


@functools.lru_cache(maxsize=None)
def reference(device, n, fname):
    """The restatement after 1 and after 25 steps (computed once per case, never modified)."""
    part, m, x, cell, v = case(n)
    ref = R.Restated(C.restated_force(part, device, DTYPES[fname]), m, DT, T, FRICTION, P0, COMPRESSIBILITY, TAUP, x, cell, v,
                     seed=R.SEED)
    ref.run(1)
    one = ref.snapshot()
    ref.run(24)
    return one, ref


def same_bits(a, b):
    return (torch.equal(a.positions, b.positions) and torch.equal(a.velocities.clone(), b.velocities.clone())
            and torch.equal(a.cell, b.cell) and a.kinetic_energy == b.kinetic_energy and a.nsteps == b.nsteps)


# 1 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_kernels_match_the_restatement(device, n, fname):
    one, last = reference(device, n, fname)
    part = case(n)[0]
    moved = float(np.max(np.abs(last.cell - part["c0"]) / np.abs(part["c0"])))
    print(f"N={n} {fname}: the reference cell moved by {moved:.3e} relative in 25 steps")
    assert moved > 1e-4
    drv = driver(device, n, DTYPES[fname])
    assert drv._hip and drv.forces.dtype == DTYPES[fname] and drv.stress.dtype == DTYPES[fname] and drv.cell.is_cuda
    drv.step()
    R.assert_close(drv, one, f"N={n} {fname} after 1 step", T, part)
    drv.run(24)
    R.assert_close(drv, last, f"N={n} {fname} after 25 steps", T, part)
    assert drv.nsteps == 25


# 2 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (86, 5462))
def test_barostat_off_gives_the_bits_of_langevin(device, n):
    part, m, x, cell, v = case(n)
    npt = driver(device, n, torch.float32, compressibility=0.0)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    fixed_cell, inner = t(cell).reshape(1, 3, 3), C.torch_force_step([part], device, torch.float32)
    nvt = Langevin(lambda pos: inner(pos, fixed_cell), t(m), DT, T, FRICTION, t(x), t(v), seed=R.SEED)
    assert npt._hip and nvt._hip
    npt.run(25), nvt.run(25)
    assert torch.equal(npt.positions, nvt.positions) and torch.equal(npt.velocities.clone(), nvt.velocities.clone())
    assert npt.kinetic_energy == nvt.kinetic_energy and npt.nsteps == nvt.nsteps == 25
    assert float(npt._rec[M._EKIN]) == float(nvt._rec[M._EKIN])  # (the K of the bath launch itself)
    assert torch.equal(npt.cell, fixed_cell)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_two_runs_give_the_same_bits_and_reading_changes_nothing(device, fname):
    a, b, c = (driver(device, 5462, DTYPES[fname]) for _ in range(3))
    a.run(25)
    b.run(25)
    for _ in range(25):
        c.step()
        c.velocities, c.temperature, c.pressure, c.volume, c.cell, c.kinetic_energy, c.nsteps
    assert same_bits(a, b), "two runs of the same inputs differ"
    assert same_bits(a, c), "reading velocities / temperature / pressure / volume / cell at every step changed the trajectory"
    assert a.pressure == b.pressure == c.pressure and a.volume == c.volume
    other = driver(device, 5462, DTYPES[fname], seed=R.SEED + 1)
    other.run(25)
    assert not torch.equal(other.cell, a.cell)  # (the seed matters to the barostat)


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", (86, 5462))
def test_state_dict_round_trip_continues_bit_for_bit(device, n):
    whole = driver(device, n, torch.float32)
    whole.run(25)
    first = driver(device, n, torch.float32)
    first.run(10)
    state = first.state_dict()
    assert state["nsteps"] == 10 and state["seed"] == R.SEED and state["cell"].shape == (1, 3, 3)
    second = driver(device, n, torch.float32, seed=5)
    second.run(3)
    second.set_pressure(3.0 * P0)
    second.set_barostat(2.0 * COMPRESSIBILITY, 3.0 * TAUP)
    second.set_timestep(2.0 * DT)
    second.load_state_dict(state)
    second.run(15)
    assert second.nsteps == 25 and same_bits(second, whole)


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", (0, 7, 2 ** 32))
def test_the_barostat_draws_component_3n_of_the_steps_noise(device, step):
    """Zero force and stress, ``friction = 0`` and ``p0 = P`` (``P = 2K / 3V`` from the same float64 operations on the host, so
    ``a (p0 - P) = 0``): ``mu = exp(sqrt(2 kT a / V) xi / 3)``, read from the record.  ``a = 1`` makes the factor 0.03; ``mu`` is
    within a few ulp (``exp`` and its own rounding, 8 eps allowed), so ``xi`` comes back to ``NORMAL_ATOL + 3 * 8 eps / factor``."""
    n = 86
    _, m, x, cell, v = case(n)
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    drv = LangevinNPT(R.zero_force_step, t(m), DT, T, 0.0, 0.0, 50.0, 50.0 * DT, t(x), t(cell), t(v), seed=R.SEED)
    assert drv._a == 1.0
    state = drv.state_dict()
    state["nsteps"] = step
    drv.load_state_dict(state)
    vol = abs(R.det3(cell))
    p = (2.0 * drv.kinetic_energy) / (3.0 * vol)
    drv.set_pressure(p)
    drv.step()
    assert drv.nsteps == step + 1 and drv.pressure == p
    mu = float(drv._npt[M._NPT_MU])
    factor = math.sqrt((2.0 * R.KB * T * 1.0) / vol)
    xi = 3.0 * math.log(mu) / factor
    want = LR.noise(R.SEED, step, 3 * n + 1)[3 * n]
    on_device = float(langevin_noise(R.SEED, step, 3 * n + 1, device)[3 * n])
    atol = LR.NORMAL_ATOL + 3.0 * 8.0 * R.EPS / factor
    print(f"step {step}: xi {xi!r} from mu, {want!r} from the restatement, {on_device!r} from nqa_md_noise; off by "
          f"{abs(xi - want):.3e} (bound {atol:.3e})")
    assert abs(xi - want) <= atol and abs(on_device - want) <= LR.NORMAL_ATOL
    assert mu != 1.0 and torch.equal(drv.cell.cpu(), mu * torch.from_numpy(cell).reshape(1, 3, 3))


# 6 ---------------------------------------------------------------------------------------------------------------------------------
def test_a_captured_step_draws_fresh_noise_and_moves_the_cell_at_every_replay(device):
    """The step's three launches captured once (one stream: a linear chain), forces and stress in static buffers that an eager
    call refreshes between replays: five replays are five eager steps of a twin, bit for bit.  The step count, the cell and mu
    live in device memory, so nothing of them is frozen into the graph."""
    n = 5462
    twin = driver(device, n, torch.float64)
    twin.run(5)  # (first, so that the kernels are loaded before anything is captured)
    drv = driver(device, n, torch.float64)
    force = C.torch_force_step([case(n)[0]], device, torch.float64)
    static_forces, static_stress = drv.forces.clone(), drv.stress.clone()
    drv._forces, drv._stress = static_forces, static_stress
    cell0 = drv.cell.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        drv._launch(finish_only=False)
    assert drv.nsteps == 0 and torch.equal(drv.cell, cell0)  # (capturing ran nothing)
    cells = []
    for _ in range(5):
        graph.replay()
        out = force(drv.positions, drv.cell)
        static_forces.copy_(out["forces"])
        static_stress.copy_(out["stress"].reshape(3, 3))
        cells.append(drv.cell.clone())
    torch.cuda.synchronize()
    assert drv.nsteps == 5
    assert all(not torch.equal(cells[k], cells[k + 1]) for k in range(4))
    assert same_bits(drv, twin)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
def test_entry_refusals(device):
    from nequip_amd import _lib as L

    lib = L.load()
    drv = driver(device, 3, torch.float64)
    stream, null = L.stream_ptr(device), L.ptr(None)
    pa, rec, par, npt, sig, cell, x, v = (L.ptr(t) for t in (drv._partials, drv._rec, drv._par, drv._npt, drv.stress, drv.cell,
                                                             drv._pos, drv._vel))
    before = [t.clone() for t in (drv._pos, drv._vel, drv.cell, drv._npt, drv._rec)]
    refused = lambda rc, word: rc != 0 and word in lib.nqa_last_error()  # noqa: E731
    F64, np_ = L.NQA_F64, drv._n_partials
    assert refused(lib.nqa_md_npt_bath(pa, np_, rec, par, null, F64, sig, cell, stream), b"npt record")
    assert refused(lib.nqa_md_npt_bath(pa, np_, null, par, npt, F64, sig, cell, stream), b"state")
    assert refused(lib.nqa_md_npt_bath(pa, np_, rec, null, npt, F64, sig, cell, stream), b"params")
    assert refused(lib.nqa_md_npt_bath(null, np_, rec, par, npt, F64, sig, cell, stream), b"partials")
    assert refused(lib.nqa_md_npt_bath(pa, 0, rec, par, npt, F64, sig, cell, stream), b"num_partials")
    assert refused(lib.nqa_md_npt_bath(pa, np_, rec, par, npt, F64, sig, null, stream), b"cell")
    assert refused(lib.nqa_md_npt_bath(pa, np_, rec, par, npt, F64, null, cell, stream), b"stress")
    assert refused(lib.nqa_md_npt_bath(pa, np_, rec, par, npt, 7, sig, cell, stream), b"float32 or float64")
    assert refused(lib.nqa_md_npt_scale(x, v, 0, npt, stream), b"num_atoms")
    assert refused(lib.nqa_md_npt_scale(x, v, -3, npt, stream), b"num_atoms")
    assert refused(lib.nqa_md_npt_scale(x, v, 3, null, stream), b"npt record")
    assert refused(lib.nqa_md_npt_scale(null, v, 3, npt, stream), b"positions")
    assert refused(lib.nqa_md_npt_scale(x, null, 3, npt, stream), b"velocities")
    torch.cuda.synchronize()
    assert drv.nsteps == 0  # (nothing ran)
    assert all(torch.equal(a, b) for a, b in zip(before, (drv._pos, drv._vel, drv.cell, drv._npt, drv._rec)))


def test_a_failed_barostat_raises_at_the_next_read(device):
    """A target that makes ``mu`` overflow: the kernel leaves ``mu = 1``, sets the flag, the flag stays, the reads raise."""
    drv = driver(device, 86, torch.float64)
    cell0 = drv.cell.clone()
    drv.set_pressure(-1e308)
    drv.step()
    assert torch.equal(drv.cell, cell0) and float(drv._npt[M._NPT_MU]) == 1.0
    drv.set_pressure(P0)
    drv.step()
    assert not torch.equal(drv.cell, cell0)
    for read in (lambda: drv.nsteps, lambda: drv.pressure, lambda: drv.volume):
        with pytest.raises(RuntimeError, match="barostat"):
            read()


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_path_and_aten_path_agree(device):
    n = 86
    part = case(n)[0]
    _, last = reference(device, n, "f32")
    hip, aten = driver(device, n, torch.float32), driver(device, n, torch.float32, backend="aten")
    assert hip._hip and not aten._hip and aten.positions.is_cuda and aten.cell.is_cuda
    hip.run(25), aten.run(25)
    R.assert_close(aten, last, "ATen path on the device after 25 steps", T, part)
    b = R.bounds(last, 25, T, part)
    np.testing.assert_allclose(hip.positions.cpu().numpy(), aten.positions.cpu().numpy(), rtol=R.RTOL, atol=b["x_atol"])
    np.testing.assert_allclose(hip.velocities.cpu().numpy(), aten.velocities.cpu().numpy(), rtol=R.RTOL, atol=b["v_atol"])
    np.testing.assert_allclose(hip.cell.cpu().numpy(), aten.cell.cpu().numpy(), rtol=b["cell_rtol"], atol=0)
    np.testing.assert_allclose(hip.kinetic_energy, aten.kinetic_energy, rtol=R.RTOL)
    np.testing.assert_allclose(hip.pressure, aten.pressure, rtol=0, atol=b["p_atol"])
    assert hip.nsteps == aten.nsteps == 25


# 9 ---------------------------------------------------------------------------------------------------------------------------------
class Atoms(R.FakeAtoms):
    def set_cell(self, cell, scale_atoms=False):
        assert not scale_atoms
        self._c = np.array(cell, dtype=np.float64)


def test_lockstep_with_the_real_model_on_a_graphed_step(device):
    """5 steps of a water box: the kernels around a ``GraphedStep`` (energy, forces, stress; the cell goes in by
    ``set_cell_from_device``) against the ATen form, which is handed, at every step, the forces and the stress the kernel route
    just obtained (the model's forces are not reproducible to the bit): the integrator alone is compared, at the tolerance of
    the Langevin lockstep test, the cell at its relative one."""
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
    atoms = Atoms([names[t] for t in types], pos, masses.numpy(), vel.numpy(), cell, pbc=True)
    args = (DT, T, FRICTION, 1.0 * R.GPA, COMPRESSIBILITY, TAUP)
    drv = LangevinNPT.from_atoms(atoms, model, *args, device=device, r_max=4.0, seed=R.SEED)
    step = drv.force_step.graphed_step
    assert isinstance(step, GraphedStep) and drv._hip and drv.forces.is_cuda and drv.stress.shape == (3, 3)

    def given(positions, cell_buffer):
        return {"forces": drv.forces.clone(), "stress": drv.stress.clone(), "total_energy": drv._out["total_energy"]}

    aten = LangevinNPT(given, drv.masses, *args, drv.positions, drv.cell, drv.velocities, seed=R.SEED, backend="aten")
    cell0 = drv.cell.clone()
    for k in range(5):
        drv.step()
        aten.step()
        what = f"water box, step {k + 1}"
        x, v = drv.positions.cpu().numpy(), drv.velocities.cpu().numpy()
        ex = float(np.max(np.abs(x - aten.positions.cpu().numpy())))
        ev = float(np.max(np.abs(v - aten.velocities.cpu().numpy())))
        ec = float(((drv.cell - aten.cell).abs() / aten.cell.abs().clamp_min(1e-300)).max())
        print(f"{what}: x off by {ex:.3e}, v by {ev:.3e}, cell by {ec:.3e} relative; P {drv.pressure!r} against {aten.pressure!r}")
        np.testing.assert_allclose(x, aten.positions.cpu().numpy(), rtol=LR.RTOL, atol=LR.X_ATOL, err_msg=f"{what}: positions")
        np.testing.assert_allclose(v, aten.velocities.cpu().numpy(), rtol=LR.RTOL, atol=LR.v_atol(T), err_msg=f"{what}: velocities")
        np.testing.assert_allclose(drv.cell.cpu().numpy(), aten.cell.cpu().numpy(), rtol=LR.RTOL, atol=LR.X_ATOL,
                                   err_msg=f"{what}: cell")
        np.testing.assert_allclose(drv.kinetic_energy, aten.kinetic_energy, rtol=LR.RTOL, err_msg=f"{what}: kinetic energy")
        np.testing.assert_allclose(drv.pressure, aten.pressure, rtol=LR.RTOL, atol=1e-12, err_msg=f"{what}: pressure")
    assert drv.nsteps == aten.nsteps == 5 and not torch.equal(drv.cell, cell0)
    assert np.isfinite(drv.potential_energy) and step.num_eager_fallbacks == 0
    drv.write_back(atoms)
    assert np.array_equal(atoms.get_cell(), drv.cell[0].cpu().numpy())
