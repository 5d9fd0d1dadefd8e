"""The device-resident Nose-Hoover / velocity-Verlet driver (nequip_amd/integrations/md.py), ATen form on the CPU: against the
float64 restatement of tests/nosehoover_restatement.py (whose docstring derives the bound), plus the host logic that needs no GPU.
The kernels are tested in tests/test_nosehoover_gpu.py."""
import math
import os
import re

import numpy as np
import pytest
import torch

import nosehoover_restatement as R
from nequip_amd.integrations import NoseHoover, VelocityVerlet, maxwell_boltzmann_velocities, units
from nequip_amd.integrations import md as md_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT, T, Q = 0.5 * R.FS, 300.0, 0.05


def make(n=7, seed=0, thermostat=True, remove_drift=False, cls=NoseHoover, **kw):
    m, x, v = R.system(n, seed)
    args = (DT, T, Q) if cls is NoseHoover else (DT,)
    drv = cls(R.torch_force_step(), torch.from_numpy(m), *args, positions=torch.from_numpy(x), velocities=torch.from_numpy(v),
              remove_drift=remove_drift, **({"thermostat": thermostat} if cls is NoseHoover else {}), **kw)
    ref = R.Restated(R.force_numpy, m, DT, T, Q, x, drv.velocities.numpy(), thermostat=thermostat)
    return drv, ref


def test_units_are_ases_codata_2014_values():
    e, amu, k = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
    assert units.kB == k / e and units.fs == 1e-5 * math.sqrt(e / amu)
    assert abs(units.kB - 8.6173303e-05) < 1e-12 and abs(units.fs - 0.0982269479) < 1e-10


def test_aten_form_matches_the_restatement():
    drv, ref = make(7)
    for steps in (1, 19):
        drv.run(steps)
        ref.run(steps)
        R.assert_close(drv, ref, f"7 atoms, after {ref.nsteps} steps")
    assert drv.nsteps == 20 and abs(drv.nvt_bath) > 1e-3  # (the bath did something)
    np.testing.assert_allclose(drv.kinetic_energy, ref.kinetic_energy, rtol=R.RTOL)
    np.testing.assert_allclose(drv.temperature, 2.0 * ref.kinetic_energy / (21 * R.KB), rtol=R.RTOL)
    np.testing.assert_allclose(drv.forces.numpy(), ref.f, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(drv.potential_energy, float(R.energy_torch(torch.from_numpy(ref.x))), rtol=1e-9)


def test_one_atom_counts_3n_plus_1_degrees_of_freedom():
    drv, ref = make(1)
    wrong = R.Restated(R.force_numpy, ref.m, DT, T, Q, ref.x, ref.v, dof_extra=0)
    drv.step(), ref.step(), wrong.step()
    R.assert_close(drv, ref, "1 atom")
    assert abs(wrong.xi - ref.xi) > 0.1 * abs(ref.xi), "the case does not tell 3N from 3N + 1"


def test_thermostat_off_is_velocity_verlet():
    for cls, kw in ((NoseHoover, {}), (VelocityVerlet, {})):
        drv, ref = make(7, thermostat=False, cls=cls)
        x, v = R.velocity_verlet(R.force_numpy, ref.m, DT, ref.x, ref.v, 20)
        drv.run(20)
        assert drv.nvt_bath == 0.0 and not drv.thermostat
        np.testing.assert_allclose(drv.positions.numpy(), x, rtol=R.RTOL, atol=0)
        np.testing.assert_allclose(drv.velocities.numpy(), v, rtol=R.RTOL, atol=0)


def test_set_temperature_and_timestep_in_mid_run():
    drv, ref = make(7)
    drv.run(5), ref.run(5)
    drv.set_temperature(900.0)
    ref.temperature = 900.0
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the temperature change")
    drv.set_timestep(0.5 * DT)
    ref.dt = 0.5 * DT
    drv.run(5), ref.run(5)
    R.assert_close(drv, ref, "after the time-step change")


def test_reading_does_not_disturb_the_trajectory():
    quiet, _ = make(7)
    read, _ = make(7)
    for _ in range(10):
        quiet.step()
        read.step()
        read.velocities, read.temperature, read.nvt_bath, read.kinetic_energy
    assert torch.equal(quiet.positions, read.positions) and torch.equal(quiet.velocities, read.velocities)
    assert quiet.nvt_bath == read.nvt_bath


def test_state_dict_round_trip_continues_bit_for_bit():
    whole, _ = make(7)
    whole.run(20)
    first, _ = make(7)
    first.run(10)
    state = first.state_dict()
    assert state["nsteps"] == 10 and set(state) >= {"positions", "velocities", "nvt_bath", "timestep", "temperature", "nvt_q"}
    second, _ = make(7)  # (the same atoms somewhere else: everything but the masses must come from the state)
    second.run(3)
    second.set_temperature(1.0)
    second.set_timestep(2.0 * DT)
    second.load_state_dict(state)
    second.run(10)
    assert second.nsteps == 20
    assert torch.equal(second.positions, whole.positions) and torch.equal(second.velocities, whole.velocities)
    assert second.nvt_bath == whole.nvt_bath
    with pytest.raises(ValueError, match="atoms"):
        make(3)[0].load_state_dict(state)


def test_remove_drift_zeroes_linear_and_angular_momentum():
    m, x, v = R.system(7, seed=2)
    v = v + np.array([0.3, -0.1, 0.2]) + np.cross(np.array([0.05, 0.02, -0.07]), x)
    drv = NoseHoover(R.torch_force_step(), torch.from_numpy(m), DT, T, Q, torch.from_numpy(x), torch.from_numpy(v))
    w = drv.velocities.numpy()
    p = m[:, None] * w
    r = x - (m[:, None] * x).sum(0) / m.sum()
    assert np.abs(p.sum(0)).max() < 1e-12 * np.abs(p).sum()
    assert np.abs(np.cross(r, p).sum(0)).max() < 1e-12 * np.abs(np.cross(r, p)).sum()
    assert np.abs(w - v).max() > 0.1  # (there was drift to remove)
    # a singular inertia tensor (one atom; atoms on a line): only the translation goes
    one = NoseHoover(R.torch_force_step(), torch.tensor([2.0], dtype=torch.float64), DT, T, Q, torch.ones(1, 3), torch.ones(1, 3))
    assert torch.equal(one.velocities, torch.zeros(1, 3, dtype=torch.float64))
    line = torch.tensor([[0.0, 0, 0], [1, 0, 0], [3, 0, 0]], dtype=torch.float64)
    vl = torch.tensor([[0.0, 1, 0], [0, -2, 0.5], [0.1, 0, 0]], dtype=torch.float64)
    drv = NoseHoover(R.torch_force_step(), torch.ones(3, dtype=torch.float64), DT, T, Q, line, vl)
    np.testing.assert_allclose(drv.velocities.numpy(), (vl - vl.mean(0)).numpy(), rtol=0, atol=1e-15)
    off = NoseHoover(R.torch_force_step(), torch.from_numpy(m), DT, T, Q, torch.from_numpy(x), torch.from_numpy(v),
                     remove_drift=False)
    assert np.array_equal(off.velocities.numpy(), v)


def test_argument_refusals_say_which():
    m, x, v = (torch.from_numpy(a) for a in R.system(4))
    step = R.torch_force_step()
    with pytest.raises(ValueError, match="masses must be positive"):
        NoseHoover(step, torch.tensor([1.0, 0.0, 1.0, 1.0], dtype=torch.float64), DT, T, Q, x)
    with pytest.raises(ValueError, match="masses must be positive"):
        NoseHoover(step, -m, DT, T, Q, x)
    with pytest.raises(ValueError, match="N == 0"):
        NoseHoover(step, m[:0], DT, T, Q, x[:0])
    with pytest.raises(ValueError, match=r"masses must have shape \[4\]"):
        NoseHoover(step, m[:3], DT, T, Q, x)
    with pytest.raises(ValueError, match=r"velocities must have shape \[4, 3\]"):
        NoseHoover(step, m, DT, T, Q, x, v[:3])
    with pytest.raises(ValueError, match=r"positions must have shape \[N, 3\]"):
        NoseHoover(step, m, DT, T, Q, x.reshape(-1))
    with pytest.raises(ValueError, match="mixed devices.*masses on meta"):
        NoseHoover(step, m.to("meta"), DT, T, Q, x)
    with pytest.raises(ValueError, match="mixed devices.*velocities on meta"):
        NoseHoover(step, m, DT, T, Q, x, v.to("meta"))
    with pytest.raises(ValueError, match="mixed devices.*forces on meta"):
        NoseHoover(lambda p: {"forces": p.to("meta"), "total_energy": p.sum()}, m, DT, T, Q, x)
    with pytest.raises(ValueError, match="timestep"):
        NoseHoover(step, m, 0.0, T, Q, x)
    with pytest.raises(ValueError, match="nvt_q"):
        NoseHoover(step, m, DT, T, 0.0, x)
    with pytest.raises(ValueError, match="backend='hip' needs device tensors"):
        NoseHoover(step, m, DT, T, Q, x, backend="hip")
    with pytest.raises(ValueError, match="float32 or float64 forces"):
        NoseHoover(lambda p: {"forces": p[:2], "total_energy": p.sum()}, m, DT, T, Q, x)
    with pytest.raises(TypeError, match="callable"):
        NoseHoover(None, m, DT, T, Q, x)


def test_maxwell_boltzmann_velocities():
    m = torch.linspace(1.0, 16.0, 4000, dtype=torch.float64)
    g = torch.Generator().manual_seed(3)
    v = maxwell_boltzmann_velocities(m, 400.0, generator=g)
    assert v.shape == (4000, 3) and v.dtype == torch.float64
    t = float((m[:, None] * v * v).sum() / (3 * 4000 * units.kB))
    assert abs(t - 400.0) < 5 * 400.0 * math.sqrt(2.0 / 12000)  # (a chi-square mean, five standard deviations)
    assert torch.equal(v, maxwell_boltzmann_velocities(m, 400.0, generator=torch.Generator().manual_seed(3)))


def test_from_atoms_and_write_back():
    m, x, v = R.system(5, seed=4)
    atoms = R.FakeAtoms(["H"] * 5, x, m, v)
    drv = NoseHoover.from_atoms(atoms, R.torch_force_step(), DT, T, Q, device="cpu", remove_drift=False)
    ref = R.Restated(R.force_numpy, m, DT, T, Q, x, v)
    drv.run(3), ref.run(3)
    R.assert_close(drv, ref, "from_atoms")
    drv.write_back(atoms)
    np.testing.assert_allclose(atoms.get_positions(), ref.x, rtol=R.RTOL)
    np.testing.assert_allclose(atoms.get_velocities(), ref.v, rtol=R.RTOL)
    # no velocities on the atoms: they start at rest; the NVE class takes the same route
    nve = VelocityVerlet.from_atoms(R.FakeAtoms(["H"] * 5, x, m), R.torch_force_step(), DT, device="cpu")
    assert not nve.thermostat and torch.equal(nve.velocities, torch.zeros(5, 3, dtype=torch.float64))
    # a model needs a cutoff and a periodic cell to build its GraphedStep from
    model = torch.nn.Linear(1, 1).eval()
    model.type_names = ["H"]
    with pytest.raises(ValueError, match="r_max"):
        NoseHoover.from_atoms(atoms, model, DT, T, Q, device="cpu")
    with pytest.raises(ValueError, match="periodic"):
        NoseHoover.from_atoms(atoms, model, DT, T, Q, device="cpu", r_max=4.0)
    with pytest.raises(ValueError, match="'Xx'"):
        NoseHoover.from_atoms(R.FakeAtoms(["Xx"] * 5, x, m, v, np.eye(3) * 9, True), model, DT, T, Q, device="cpu", r_max=4.0)


def test_kernels_are_declared_bound_and_built():
    from nequip_amd import _lib
    from nequip_amd.csrc import build

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nequip_amd.h")).read(), flags=re.S)
    for name in ("nqa_md_step", "nqa_md_bath", "nqa_md_num_partials"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in nequip_amd.h"
        assert name in _lib.SIGNATURES
    assert "md.hip" in build.SOURCES
    # the record the host writes word by word is the struct of the header
    fields = re.search(r"typedef struct nqa_md_state \{(.*?)\}", header, flags=re.S).group(1)
    names = re.findall(r"\b([a-z_]+)\s*[,;]", fields)
    assert names == ["dt", "g", "q", "xi", "kinetic_energy", "nsteps", "fresh", "observed_kinetic_energy"]
    assert [md_module._DT, md_module._G, md_module._Q, md_module._XI, md_module._EKIN, md_module._NSTEPS, md_module._FRESH,
            md_module._EKIN_OBSERVED] == list(range(8))
    lib = _lib.load()
    assert [lib.nqa_md_num_partials(n) for n in (0, 1, 85, 86, 5462)] == [0, 1, 1, 2, 65]
