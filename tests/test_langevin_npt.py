"""LangevinNPT (nequip_amd/integrations/md.py), ATen form on the CPU, against the float64 restatement of tests/npt_restatement.py
(whose docstring derives the bounds), the scheme itself against the exact volume distribution of an ideal gas, and the host logic
that needs no GPU.  The kernels are tested in tests/test_langevin_npt_gpu.py."""
import functools
import math
import os
import re

import numpy as np
import pytest
import torch

import cell_fire_restatement as C
import npt_restatement as R
from nequip_amd.integrations import Langevin, LangevinNPT, units
from nequip_amd.integrations import md as md_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, T = 0.5 * R.FS, 300.0
FRICTION = 0.01 / R.FS
# a stiff barostat: a = compressibility dt / taup = 0.01 against pressures of 0.1 to a few eV/A^3 moves the cell by parts in a
# thousand per step
P0, COMPRESSIBILITY, TAUP = 0.01, 0.5, 50.0 * DT


def make(n=7, fdtype=torch.float64, seed=R.SEED, compressibility=COMPRESSIBILITY, **kw):
    part, m, x, cell, v = R.site_case(n)
    t = torch.from_numpy
    drv = LangevinNPT(C.torch_force_step([part], "cpu", fdtype), t(m), DT, T, FRICTION, P0, compressibility, TAUP, t(x),
                      t(cell), t(v), seed=seed, **kw)
    ref = R.Restated(C.restated_force(part, "cpu", fdtype), m, DT, T, FRICTION, P0, compressibility, TAUP, x, cell, v, seed=seed)
    return drv, ref, part


def same_bits(a, b):
    return (torch.equal(a.positions, b.positions) and torch.equal(a.velocities.clone(), b.velocities.clone())
            and torch.equal(a.cell, b.cell) and a.kinetic_energy == b.kinetic_energy and a.nsteps == b.nsteps)


@pytest.mark.parametrize("fname", ("f32", "f64"))
@pytest.mark.parametrize("n", (1, 86))
def test_aten_driver_matches_the_restatement(n, fname):
    fdtype = {"f32": torch.float32, "f64": torch.float64}[fname]
    drv, ref, part = make(n, fdtype)
    assert not drv._hip and drv.forces.dtype == fdtype and drv.stress.dtype == fdtype and drv.cell.shape == (1, 3, 3)
    cell0 = drv.cell.clone()
    for steps in (1, 24):
        drv.run(steps), ref.run(steps)
        R.assert_close(drv, ref, f"{n} atoms {fname}, after {ref.nsteps} steps", T, part)
    moved = float(np.max(np.abs(ref.cell - part["c0"]) / np.abs(part["c0"])))
    print(f"the reference cell moved by {moved:.3e} relative")
    assert moved > 1e-4 and not torch.equal(drv.cell, cell0)
    assert drv.nsteps == 25 and drv.target_pressure == P0
    np.testing.assert_allclose(drv.stress.double().numpy(), ref.sigma, rtol=1e-6, atol=1e-9)


@pytest.mark.parametrize("n", (7, 86))
def test_barostat_off_is_langevin_bit_for_bit(n):
    npt, _, part = make(n, compressibility=0.0)
    m, x, v = (torch.from_numpy(a) for a in (R.site_case(n)[1], part["x"], R.site_case(n)[4]))
    cell = torch.from_numpy(part["c0"]).reshape(1, 3, 3)
    inner = C.torch_force_step([part], "cpu")
    nvt = Langevin(lambda pos: inner(pos, cell), m, DT, T, FRICTION, x, v, seed=R.SEED, backend="aten")
    npt.run(25), nvt.run(25)
    assert torch.equal(npt.positions, nvt.positions) and torch.equal(npt.velocities, nvt.velocities)
    assert npt.kinetic_energy == nvt.kinetic_energy and npt.nsteps == nvt.nsteps == 25
    assert torch.equal(npt.cell, cell)


def test_state_dict_round_trip_continues_bit_for_bit():
    whole, _, _ = make(7)
    whole.run(25)
    first, _, _ = make(7)
    first.run(10)
    state = first.state_dict()
    assert state["nsteps"] == 10 and state["seed"] == R.SEED and state["compressibility"] == COMPRESSIBILITY
    assert set(state) == {"positions", "velocities", "nsteps", "timestep", "temperature", "friction", "seed", "cell", "pressure",
                          "compressibility", "taup"}
    second, _, _ = make(7, seed=5)
    second.run(3)
    second.set_pressure(2.0 * P0)
    second.set_barostat(3.0 * COMPRESSIBILITY, 2.0 * TAUP)
    second.set_timestep(2.0 * DT)
    second.load_state_dict(state)
    second.run(15)
    assert second.nsteps == 25 and second.taup == TAUP and second.target_pressure == P0
    assert same_bits(second, whole)
    with pytest.raises(ValueError, match="LangevinNPT"):
        second.load_state_dict({k: v for k, v in state.items() if k not in ("cell", "compressibility")})
    with pytest.raises(ValueError, match="atoms"):
        make(3)[0].load_state_dict(state)


def test_set_pressure_barostat_and_timestep_in_mid_run():
    drv, ref, part = make(7)
    drv.run(5), ref.run(5)
    drv.set_pressure(-2.0 * P0)
    ref.p0 = -2.0 * P0
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the pressure change", T, part)
    drv.set_barostat(0.5 * COMPRESSIBILITY, 3.0 * TAUP)
    ref.compressibility, ref.taup = 0.5 * COMPRESSIBILITY, 3.0 * TAUP
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the barostat change", T, part)
    drv.set_timestep(0.5 * DT)
    ref.dt = 0.5 * DT
    assert drv._a == 0.5 * COMPRESSIBILITY * (0.5 * DT) / (3.0 * TAUP)
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the time-step change", T, part)


def test_argument_refusals_say_which():
    part, m, x, cell, v = R.site_case(4)
    m, x, cell, v = (torch.from_numpy(a) for a in (m, x, cell, v))
    step = C.torch_force_step([part], "cpu")
    new = lambda p=P0, c=COMPRESSIBILITY, tau=TAUP, cl=cell, s=step, **kw: LangevinNPT(  # noqa: E731
        s, m, DT, T, FRICTION, p, c, tau, x, cl, v, **kw)
    for bad in (math.inf, math.nan):
        with pytest.raises(ValueError, match="pressure must be finite"):
            new(p=bad)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="compressibility must be non-negative and finite"):
            new(c=bad)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="taup must be positive and finite"):
            new(tau=bad)
    singular = cell.clone()
    singular[2] = singular[0] + singular[1]
    with pytest.raises(ValueError, match="cell is singular"):
        new(cl=singular)
    with pytest.raises(ValueError, match=r"cell must be a tensor of shape \[3, 3\] or \[1, 3, 3\]"):
        new(cl=cell.reshape(9))
    with pytest.raises(ValueError, match="mixed devices.*cell on meta"):
        new(cl=cell.to("meta"))
    with pytest.raises(ValueError, match="stress: force_step must return it"):
        new(s=lambda pos, c: {"forces": torch.zeros_like(pos), "total_energy": pos.sum()})
    with pytest.raises(ValueError, match="friction must be non-negative and finite"):
        LangevinNPT(step, m, DT, T, -1.0, P0, COMPRESSIBILITY, TAUP, x, cell)
    with pytest.raises(ValueError, match="backend='hip' needs device tensors"):
        new(backend="hip")
    drv = new()
    for call, word in ((lambda: drv.set_pressure(math.nan), "pressure"), (lambda: drv.set_barostat(-1.0, TAUP), "compressibility"),
                       (lambda: drv.set_barostat(COMPRESSIBILITY, 0.0), "taup")):
        with pytest.raises(ValueError, match=word):
            call()
    # a GraphedStep whose cell is not fully periodic is refused before anything is built around it
    from nequip_amd.integrations.graphed_step import GraphedStep

    graphed = object.__new__(GraphedStep)
    graphed._pbc, graphed.outputs = (True, True, False), ("total_energy", "forces", "stress")
    with pytest.raises(ValueError, match="all three directions periodic"):
        new(s=graphed)


def test_a_failed_barostat_raises_at_the_next_read():
    """A pressure that makes ``mu`` overflow: ``mu`` stays 1, the flag is set and stays, the reads raise."""
    drv, _, _ = make(7)
    cell0 = drv.cell.clone()
    drv.set_pressure(-1e308)
    drv.step()
    assert torch.equal(drv.cell, cell0)
    drv.set_pressure(P0)
    drv.step()
    for read in (lambda: drv.nsteps, lambda: drv.pressure, lambda: drv.volume):
        with pytest.raises(RuntimeError, match="barostat"):
            read()


def test_units():
    assert units.GPa == 1e-21 / 1.6021766208e-19 == R.GPA
    assert units.bar == 1e-25 / 1.6021766208e-19 == R.BAR
    assert units.kB == R.KB and units.fs == R.FS


class Atoms(R.FakeAtoms):
    def set_cell(self, cell, scale_atoms=False):
        assert not scale_atoms
        self._c = np.array(cell, dtype=np.float64)


def test_from_atoms_and_write_back():
    part, m, x, cell, v = R.site_case(5)
    atoms = Atoms(["H"] * 5, x, m, v, cell, pbc=True)
    drv = LangevinNPT.from_atoms(atoms, C.torch_force_step([part], "cpu"), DT, T, FRICTION, P0, COMPRESSIBILITY, TAUP,
                                 device="cpu", seed=11)
    ref = R.Restated(C.numpy_force(part), m, DT, T, FRICTION, P0, COMPRESSIBILITY, TAUP, x, cell, v, seed=11)
    drv.run(3), ref.run(3)
    R.assert_close(drv, ref, "from_atoms", T, part)
    drv.write_back(atoms)
    b = R.bounds(ref, 3, T, part)
    np.testing.assert_allclose(atoms.get_cell(), ref.cell, rtol=b["cell_rtol"])
    np.testing.assert_allclose(atoms.get_positions(), ref.x, rtol=R.RTOL, atol=b["x_atol"])
    np.testing.assert_allclose(atoms.get_velocities(), ref.v, rtol=R.RTOL, atol=b["v_atol"])
    model = torch.nn.Linear(1, 1).eval()
    model.type_names = ["H"]
    with pytest.raises(ValueError, match="r_max"):
        LangevinNPT.from_atoms(atoms, model, DT, T, FRICTION, P0, COMPRESSIBILITY, TAUP, device="cpu")
    with pytest.raises(ValueError, match="all three directions periodic"):
        LangevinNPT.from_atoms(Atoms(["H"] * 5, x, m, v, cell, pbc=False), model, DT, T, FRICTION, P0, COMPRESSIBILITY, TAUP,
                               device="cpu", r_max=3.0)


def test_kernels_are_declared_bound_and_built():
    from nequip_amd import _lib

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nequip_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("nqa_md_npt_bath", "nqa_md_npt_scale"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in nequip_amd.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert len(_lib.SIGNATURES["nqa_md_npt_bath"][1]) == 9 and len(_lib.SIGNATURES["nqa_md_npt_scale"][1]) == 5
    fields = re.search(r"typedef struct nqa_md_npt_state \{(.*?)\}", header, flags=re.S).group(1)
    names = re.findall(r"\b([a-zA-Z0-9_]+)\s*[,;]", fields)
    assert names == ["a", "p0", "noise_index", "mu", "pressure", "kinetic_energy", "volume", "failed"]
    M = md_module
    assert [M._NPT_A, M._NPT_P0, M._NPT_INDEX, M._NPT_MU, M._NPT_P, M._NPT_EKIN, M._NPT_VOLUME, M._NPT_FAILED] == list(range(8))
    source = open(os.path.join(ROOT, "nequip_amd", "csrc", "md.hip")).read()
    size = re.search(r"static_assert\(sizeof\(nqa_md_npt_state\) == (\d+)", source)
    assert size and int(size.group(1)) == 8 * len(names)


# ---- the scheme against the exact ensemble of an ideal gas ---------------------------------------------------------------------------
GAS_N, GAS_STEPS, GAS_DROP, GAS_SEED = 8, 44000, 4000, 20261021


@functools.lru_cache(maxsize=None)
def ideal_gas():
    """Natural units ``m = kT = p0 = 1``: ``V0 = 9``, ``dt = 0.02 sqrt(m / kT) V0^(1/3)``, ``friction dt = 0.02``, ``compressibility
    = 1 / p0``, ``taup = 25 dt``.  Returns the parameters, the start and the noise of all steps (one vectorised Philox call)."""
    kt, p0 = 1.0, 1.0
    v0 = 9.0 * kt / p0
    dt = 0.02 * math.sqrt(1.0 / kt) * v0 ** (1.0 / 3.0)
    rng = np.random.default_rng(GAS_SEED)
    cell = np.eye(3) * v0 ** (1.0 / 3.0)
    x = rng.uniform(0.0, 1.0, size=(GAS_N, 3)) @ cell
    v = rng.normal(size=(GAS_N, 3)) * math.sqrt(kt / 1.0)
    args = dict(masses=np.ones(GAS_N), dt=dt, temperature=kt / R.KB, friction=0.02 / dt, pressure=p0, compressibility=1.0 / p0,
                taup=25.0 * dt, x=x, cell=cell, v=v, seed=GAS_SEED)
    return args, kt, p0, R.noise_table(GAS_SEED, 0, GAS_STEPS, 3 * GAS_N + 1)


def test_the_scheme_samples_the_ideal_gas_volume_distribution():
    """The restatement alone (this judges the scheme, not the code under test).  Exact: ``<V> = (N + 1) kT / p0`` and ``Var V =
    (N + 1) (kT / p0)^2``.  44 000 steps, the first 4 000 dropped; the mean within 4 standard errors (from 20 block means), the
    variance within 25 %."""
    args, kt, p0, table = ideal_gas()
    ref = R.Restated(R.zero_force_numpy, table=table, **args)
    vols = np.empty(GAS_STEPS)
    for k in range(GAS_STEPS):
        ref.step()
        vols[k] = ref.volume
    vols = vols[GAS_DROP:]
    want_mean, want_var = (GAS_N + 1) * kt / p0, (GAS_N + 1) * (kt / p0) ** 2
    blocks = vols.reshape(20, -1).mean(axis=1)
    mean, stderr, var = float(vols.mean()), float(blocks.std(ddof=1) / math.sqrt(20)), float(vols.var())
    print(f"<V> = {mean:.4f} against {want_mean} ({(mean - want_mean) / stderr:+.2f} standard errors of {stderr:.4f}); "
          f"Var V = {var:.4f} against {want_var} ({var / want_var - 1.0:+.1%})")
    assert abs(mean - want_mean) < 4.0 * stderr
    assert abs(var - want_var) < 0.25 * want_var


def test_aten_driver_follows_the_ideal_gas_restatement():
    """The first 200 steps of the run above through the driver: what was judged is what the driver does."""
    args, kt, p0, table = ideal_gas()
    ref = R.Restated(R.zero_force_numpy, table=table, **args)
    t = torch.from_numpy
    drv = LangevinNPT(R.zero_force_step, t(args["masses"]), args["dt"], args["temperature"], args["friction"], p0,
                      args["compressibility"], args["taup"], t(args["x"]), t(args["cell"]), t(args["v"]), seed=GAS_SEED)
    for steps in (1, 199):
        drv.run(steps), ref.run(steps)
        R.assert_close(drv, ref, f"ideal gas after {ref.nsteps} steps", args["temperature"])
    assert drv.nsteps == 200
