"""BatchedLangevin and BatchedLangevinNPT (nequip_amd/integrations/md_batched.py), ATen form on the CPU: against the float64
restatements of tests/langevin_restatement.py and tests/npt_restatement.py per system, against the single-system drivers, and the
host logic that needs no GPU (the chunk table, the seed rule, the checks of the arguments, checkpoints, ``from_torchsim``).  The
kernels are tested in tests/test_langevin_batched_gpu.py.

Bit for bit where every operation is element-wise (NVT: positions and velocities; the restatement draws its normals with the same
numpy functions); under NPT a per-system sum feeds back through ``mu``, and the bounds of ``npt_restatement`` apply, as they do in
tests/test_langevin_npt.py."""
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import batched_md_cases as B
import langevin_restatement as LR
import npt_restatement as NR
from nequip_amd.integrations import BatchedLangevin, BatchedLangevinNPT, Langevin
from nequip_amd.integrations import md_batched as MB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTS = (1, 85, 86, 3, 171)
CPU = torch.device("cpu")


# ---- the chunk table ---------------------------------------------------------------------------------------------------------------
def test_chunk_table():
    counts = [1, 85, 86, 171, 5462]
    chunks, begin = MB.md_chunk_table(counts, 256)
    assert begin.tolist() == [0, 1, 2, 4, 7, 72] and np.diff(begin).tolist() == [1, 1, 2, 3, 65]
    assert chunks.dtype.itemsize == 24 and len(chunks) == 72
    first_component = np.concatenate([[0], np.cumsum(3 * np.asarray(counts))])
    for s, n in enumerate(counts):
        mine = chunks[begin[s]:begin[s + 1]]
        assert (mine["system"] == s).all()
        assert mine["local0"].tolist() == [256 * k for k in range(len(mine))]
        assert mine["component0"].tolist() == [int(first_component[s]) + 256 * k for k in range(len(mine))]
        assert mine["count"][:-1].tolist() == [256] * (len(mine) - 1)
        assert mine["count"][-1] == 3 * n - 256 * (len(mine) - 1) and 0 < mine["count"][-1] <= 256
        # no chunk crosses a system: its components lie inside the system's, and together they cover them once
        assert mine["component0"][0] == first_component[s]
        assert mine["component0"][-1] + mine["count"][-1] == first_component[s + 1]
        assert int(mine["count"].sum()) == 3 * n
    # component 255 and 256 of an 86-atom system belong to one atom: the second chunk begins inside an atom
    assert chunks[3]["local0"] == 256 and chunks[3]["local0"] % 3 == 1 and chunks[3]["count"] == 2
    one, begin_one = MB.md_chunk_table([5462])
    assert len(one) == 65 and begin_one.tolist() == [0, 65] and one["count"][-1] == 16386 - 64 * 256


# ---- against the restatements ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(B.DTYPES))
def test_aten_nvt_matches_the_restatement_bit_for_bit(fname):
    systems, dtype = B.batch(COUNTS), B.DTYPES[fname]
    drv = B.batched_nvt(systems, CPU, dtype)
    refs = [B.restated_nvt(q, CPU, dtype) for q in systems]
    assert not drv._hip and drv.forces.dtype == dtype and drv.num_systems == len(COUNTS)
    for steps in (1, 11):
        drv.run(steps)
        for s, ref in enumerate(refs):
            ref.run(steps)
            view = B.View(drv, s)
            assert np.array_equal(view.positions.numpy(), ref.x), f"system {s} after {ref.nsteps} steps: positions"
            assert np.array_equal(view.velocities.numpy(), ref.v), f"system {s} after {ref.nsteps} steps: velocities"
            LR.assert_close(view, ref, f"system {s} ({systems[s]['n']} atoms) {fname}", systems[s]["temperature"])
    assert drv.nsteps.tolist() == [12] * len(COUNTS) and drv.potential_energy.shape == (len(COUNTS),)


@pytest.mark.parametrize("fname", sorted(B.DTYPES))
def test_aten_npt_matches_the_restatement(fname):
    systems, dtype = B.batch(COUNTS), B.DTYPES[fname]
    drv = B.batched_npt(systems, CPU, dtype)
    refs = [B.restated_npt(q, CPU, dtype) for q in systems]
    assert drv.cell.shape == (len(COUNTS), 3, 3) and drv.stress.dtype == dtype
    cell0 = drv.cell.clone()
    for steps in (1, 24):
        drv.run(steps)
        for s, ref in enumerate(refs):
            ref.run(steps)
            NR.assert_close(B.View(drv, s), ref, f"system {s} ({systems[s]['n']} atoms) {fname}, after {ref.nsteps} steps",
                            systems[s]["temperature"], systems[s]["part"])
    assert all(not torch.equal(drv.cell[s], cell0[s]) for s in range(len(COUNTS)))
    assert np.array_equal(drv.target_pressure, [q["pressure"] for q in systems])


# ---- against the single-system drivers ---------------------------------------------------------------------------------------------
def test_aten_batch_and_single_drivers_agree_bit_for_bit():
    systems = B.batch(COUNTS)
    drv = B.batched_nvt(systems, CPU, torch.float32)
    alone = [B.single_nvt(q, CPU, torch.float32) for q in systems]
    for _ in range(10):
        drv.step()
        for s, one in enumerate(alone):
            one.step()
            view = B.View(drv, s)
            assert torch.equal(view.positions, one.positions) and torch.equal(view.stored_velocities, one._vel)
            assert torch.equal(view.velocities.clone(), one.velocities.clone()) and view.nsteps == one.nsteps
            np.testing.assert_allclose(view.kinetic_energy, one.kinetic_energy, rtol=LR.RTOL)  # (a sum in another order)
            np.testing.assert_allclose(view.temperature, one.temperature, rtol=LR.RTOL)


def test_zero_compressibility_is_the_nvt_batch_bit_for_bit():
    systems = B.batch(COUNTS)
    npt = B.batched_npt(systems, CPU, compressibility=[0.0, 0.0, q_c := systems[2]["compressibility"], 0.0, 0.0])
    cells = npt.cell.clone()
    inner = npt.force_step
    x = torch.from_numpy(np.concatenate([q["part"]["x"] for q in systems]))
    nvt = BatchedLangevin(lambda pos: inner(pos, cells), npt.masses, npt.timestep, npt.target_temperature, npt.friction, x,
                          npt.system_idx, B._cat(systems, "v", CPU), seed=npt.seeds)
    npt.run(10), nvt.run(10)
    lo, hi = (int(v) for v in B.offsets(systems)[2:4])
    for s in (0, 1, 3, 4):
        a, b = B.View(npt, s), B.View(nvt, s)
        assert torch.equal(a.positions, b.positions) and torch.equal(a.velocities.clone(), b.velocities.clone())
        assert a.kinetic_energy == b.kinetic_energy and torch.equal(npt.cell[s], cells[s]) and a.scaling == 1.0
    assert q_c > 0.0 and not torch.equal(npt.cell[2], cells[2]) and not torch.equal(npt.positions[lo:hi], nvt.positions[lo:hi])


# ---- seeds and broadcasting --------------------------------------------------------------------------------------------------------
def test_seed_rule():
    assert MB.batch_seeds(5, 3) == [5, 6, 7]
    assert MB.batch_seeds(2 ** 64 - 1, 3) == [2 ** 64 - 1, 0, 1]  # (wraps around)
    assert MB.batch_seeds([9, 2 ** 64 - 1, 9], 3) == [9, 2 ** 64 - 1, 9]  # (taken as given)
    assert MB.batch_seeds(torch.tensor([3, 1]), 2) == [3, 1] and MB.batch_seeds(np.int64(4), 2) == [4, 5]
    for bad, word in ((-1, "seed"), (2 ** 64, "seed"), ([1, 2], "one per system"), ([1, 2, -3], "seed of system 2"),
                      ([1, 2, 0.5], "seed of system 2"), (1.5, "seed"), (True, "seed")):
        with pytest.raises(ValueError, match=word):
            MB.batch_seeds(bad, 3)
    # an int seed gives system s the trajectory of a single run with seed + s, wrap-around included
    systems = B.batch((3, 5, 4))
    drv = B.batched_nvt(systems, CPU, seed=2 ** 64 - 2)
    assert drv.seeds == [2 ** 64 - 2, 2 ** 64 - 1, 0]
    drv.run(3)
    for s, q in enumerate(systems):
        one = B.single_nvt(dict(q, seed=drv.seeds[s]), CPU)
        one.run(3)
        assert torch.equal(B.View(drv, s).positions, one.positions)


def test_scalars_are_broadcast_to_every_system():
    systems = B.batch((3, 5, 4))
    a = B.batched_nvt(systems, CPU, timestep=B.DT, temperature=250.0, friction=B.FRICTION)
    b = B.batched_nvt(systems, CPU, timestep=[B.DT] * 3, temperature=torch.full((3,), 250.0), friction=np.full(3, B.FRICTION))
    a.run(4), b.run(4)
    assert torch.equal(a.positions, b.positions) and torch.equal(a.velocities.clone(), b.velocities.clone())
    assert a.timestep.tolist() == [B.DT] * 3 and a.target_temperature.tolist() == [250.0] * 3
    a.set_temperature(100.0), b.set_temperature([100.0] * 3)
    a.set_friction(2.0 * B.FRICTION), b.set_friction([2.0 * B.FRICTION] * 3)
    a.set_timestep(0.5 * B.DT), b.set_timestep([0.5 * B.DT] * 3)
    a.run(4), b.run(4)
    assert torch.equal(a.positions, b.positions) and a.friction.tolist() == [2.0 * B.FRICTION] * 3
    npt = B.batched_npt(systems, CPU, pressure=B.P0, compressibility=B.COMPRESSIBILITY, taup=B.TAUP)
    assert npt.target_pressure.tolist() == [B.P0] * 3 and npt.taup.tolist() == [B.TAUP] * 3
    npt.set_pressure(2.0 * B.P0), npt.set_barostat(0.25, [B.TAUP, 2 * B.TAUP, 3 * B.TAUP])
    assert npt.target_pressure.tolist() == [2.0 * B.P0] * 3 and npt.compressibility.tolist() == [0.25] * 3
    assert npt._a_h.tolist() == [0.25 * q["dt"] / (k * B.TAUP) for k, q in zip((1, 2, 3), systems)]


def test_setters_in_mid_run_follow_the_restatement_and_touch_the_named_systems_only():
    systems = B.batch((3, 86, 4))
    drv, twin = B.batched_nvt(systems, CPU), B.batched_nvt(systems, CPU)
    refs = [B.restated_nvt(q, CPU) for q in systems]
    drv.run(3), twin.run(3)
    for ref in refs:
        ref.run(3)
    temperature, friction, dt = drv.target_temperature, drv.friction, drv.timestep
    temperature[1], friction[1], dt[1] = 900.0, 5.0 * friction[1], 0.5 * dt[1]
    drv.set_temperature(temperature), drv.set_friction(friction), drv.set_timestep(dt)
    refs[1].temperature, refs[1].friction, refs[1].dt = 900.0, friction[1], dt[1]
    drv.run(4), twin.run(4)
    for s, ref in enumerate(refs):
        ref.run(4)
        LR.assert_close(B.View(drv, s), ref, f"system {s} after the setters", 900.0)
    for s in (0, 2):
        assert torch.equal(B.View(drv, s).positions, B.View(twin, s).positions)
        assert torch.equal(B.View(drv, s).velocities.clone(), B.View(twin, s).velocities.clone())
    assert not torch.equal(B.View(drv, 1).positions, B.View(twin, 1).positions)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def test_argument_refusals_say_which():
    systems = B.batch((3, 5, 4))
    m, x, v = (B._cat(systems, name, CPU) for name in ("m", "x", "v"))
    sidx, step = B._sidx(systems, CPU), B.spring_force_step(systems, CPU)
    new = lambda dt=B.DT, t=B.T, fr=B.FRICTION, idx=sidx, mm=m, vv=v, **kw: BatchedLangevin(  # noqa: E731
        step, mm, dt, t, fr, x, idx, vv, **kw)
    with pytest.raises(ValueError, match="system_idx must start at 0, never decrease"):
        new(idx=torch.tensor([0] * 3 + [2] * 5 + [1] * 4))
    with pytest.raises(ValueError, match="system_idx must start at 0"):
        new(idx=sidx + 1)
    with pytest.raises(ValueError, match="no system without atoms"):
        new(idx=torch.tensor([0] * 3 + [1] * 5 + [3] * 4))
    with pytest.raises(ValueError, match=r"system_idx must be a tensor of shape \[12\]"):
        new(idx=sidx[:-1])
    with pytest.raises(ValueError, match="system_idx must hold integers"):
        new(idx=sidx.double())
    with pytest.raises(ValueError, match=r"masses must have shape \[12\]"):
        new(mm=m[:-1])
    with pytest.raises(ValueError, match=r"velocities must have shape \[12, 3\]"):
        new(vv=v[:-1])
    with pytest.raises(ValueError, match="mixed devices.*system_idx on meta"):
        new(idx=sidx.to("meta"))
    with pytest.raises(ValueError, match="mixed devices.*masses on meta"):
        new(mm=m.to("meta"))
    for bad in (-1.0, math.inf, math.nan, [300.0, -1.0, 300.0]):
        with pytest.raises(ValueError, match="temperature must be non-negative and finite"):
            new(t=bad)
    for bad in (-1.0, math.inf, [0.0, 0.0, math.nan]):
        with pytest.raises(ValueError, match="friction must be non-negative and finite"):
            new(fr=bad)
    for bad in (0.0, -1.0, math.inf, [B.DT, 0.0, B.DT]):
        with pytest.raises(ValueError, match="timestep must be positive"):
            new(dt=bad)
    with pytest.raises(ValueError, match=r"temperature must be a number or hold one value per system \(\[3\]\), got 2 values"):
        new(t=[300.0, 300.0])
    with pytest.raises(ValueError, match=r"got -1.0 for system 1"):
        new(t=[300.0, -1.0, 300.0])
    with pytest.raises(ValueError, match="backend='hip' needs device tensors"):
        new(backend="hip")
    with pytest.raises(ValueError, match="backend must be"):
        new(backend="triton")
    drv = new()
    for call, word in ((lambda: drv.set_temperature(-1.0), "temperature"), (lambda: drv.set_friction([0.0, -1.0, 0.0]), "friction"),
                       (lambda: drv.set_timestep(0.0), "timestep"), (lambda: drv.set_timestep([B.DT] * 2), "one value per system")):
        with pytest.raises(ValueError, match=word):
            call()

    parts = [q["part"] for q in systems]
    xs = torch.from_numpy(np.concatenate([p["x"] for p in parts]))
    cells = torch.from_numpy(np.stack([p["c0"] for p in parts]))
    import cell_fire_restatement as C

    cstep = C.torch_force_step(parts, "cpu")
    npt = lambda p=B.P0, c=B.COMPRESSIBILITY, tau=B.TAUP, cl=cells, st=cstep: BatchedLangevinNPT(  # noqa: E731
        st, m, B.DT, B.T, B.FRICTION, p, c, tau, xs, cl, sidx, v)
    for bad in (math.inf, math.nan, [B.P0, math.nan, B.P0]):
        with pytest.raises(ValueError, match="pressure must be finite"):
            npt(p=bad)
    for bad in (-1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="compressibility must be non-negative and finite"):
            npt(c=bad)
    for bad in (0.0, -1.0, math.inf, math.nan):
        with pytest.raises(ValueError, match="taup must be positive and finite"):
            npt(tau=bad)
    with pytest.raises(ValueError, match=r"cell must be a tensor of shape \[3, 3, 3\]"):
        npt(cl=cells[:2])
    with pytest.raises(ValueError, match=r"cell must be a tensor of shape \[3, 3, 3\]"):
        npt(cl=cells[0])
    singular = cells.clone()
    singular[1, 2] = singular[1, 0] + singular[1, 1]
    with pytest.raises(ValueError, match="cell of system 1 is singular"):
        npt(cl=singular)
    with pytest.raises(ValueError, match="mixed devices.*cell on meta"):
        npt(cl=cells.to("meta"))
    with pytest.raises(ValueError, match="stress: force_step must return it"):
        npt(st=lambda pos, c: {"forces": torch.zeros_like(pos), "total_energy": torch.zeros(3)})
    with pytest.raises(ValueError, match=r"stress: force_step must return float32 or float64 \[3, 3, 3\]"):
        npt(st=lambda pos, c: {"forces": torch.zeros_like(pos), "total_energy": torch.zeros(3), "stress": torch.zeros(3, 3)})
    ok = npt()
    for call, word in ((lambda: ok.set_pressure(math.nan), "pressure"), (lambda: ok.set_barostat(-1.0, B.TAUP), "compressibility"),
                       (lambda: ok.set_barostat(B.COMPRESSIBILITY, [B.TAUP, 0.0, B.TAUP]), "taup")):
        with pytest.raises(ValueError, match=word):
            call()


# ---- checkpoints -------------------------------------------------------------------------------------------------------------------
def test_state_dict_round_trip_continues_bit_for_bit():
    systems = B.batch((3, 86, 4))
    whole = B.batched_nvt(systems, CPU)
    whole.run(12)
    first = B.batched_nvt(systems, CPU)
    first.run(5)
    state = first.state_dict()
    assert set(state) == {"positions", "velocities", "nsteps", "timestep", "temperature", "friction", "seeds"}
    assert state["nsteps"].tolist() == [5, 5, 5] and state["seeds"] == [q["seed"] for q in systems]
    assert state["friction"].tolist() == [q["friction"] for q in systems]
    second = B.batched_nvt(systems, CPU, seed=3, temperature=10.0)
    second.run(2)
    second.set_friction(0.0), second.set_timestep(2.0 * B.DT)
    second.load_state_dict(state)
    second.run(7)
    assert second.nsteps.tolist() == [12] * 3 and second.seeds == whole.seeds
    assert torch.equal(second.positions, whole.positions) and torch.equal(second.velocities.clone(), whole.velocities.clone())
    assert torch.equal(second.kinetic_energy, whole.kinetic_energy)
    with pytest.raises(ValueError, match="atoms"):
        B.batched_nvt(B.batch((3, 5)), CPU).load_state_dict(state)
    with pytest.raises(ValueError, match="batched Langevin run of 3 systems"):
        second.load_state_dict({k: v for k, v in state.items() if k != "seeds"})

    whole = B.batched_npt(systems, CPU)
    whole.run(12)
    first = B.batched_npt(systems, CPU)
    first.run(5)
    state = first.state_dict()
    assert set(state) == {"positions", "velocities", "nsteps", "timestep", "temperature", "friction", "seeds", "cell", "pressure",
                          "compressibility", "taup"}
    second = B.batched_npt(systems, CPU, seed=3)
    second.run(2)
    second.set_pressure(3.0 * B.P0), second.set_barostat(0.1, 7.0 * B.TAUP)
    second.load_state_dict(state)
    second.run(7)
    assert torch.equal(second.positions, whole.positions) and torch.equal(second.cell, whole.cell)
    assert torch.equal(second.velocities.clone(), whole.velocities.clone()) and torch.equal(second.pressure, whole.pressure)
    with pytest.raises(ValueError, match="BatchedLangevinNPT"):
        second.load_state_dict({k: v for k, v in state.items() if k not in ("cell", "compressibility")})
    with pytest.raises(ValueError, match="BatchedLangevinNPT"):
        B.batched_nvt(systems, CPU).load_state_dict(state)


def test_a_cell_without_volume_fails_its_own_system_only():
    systems = B.batch((3, 86, 4))
    drv, twin = B.batched_npt(systems, CPU), B.batched_npt(systems, CPU)
    state = drv.state_dict()
    state["cell"][1, 2] = 0.0  # a lattice vector of zeros: every term of the determinant is exactly 0
    drv.load_state_dict(state)
    drv.step(), twin.step()
    assert drv.failed.tolist() == [False, True, False] and float(drv.scaling[1]) == 1.0
    for s in (0, 2):
        assert torch.equal(drv.cell[s], twin.cell[s]) and torch.equal(B.View(drv, s).positions, B.View(twin, s).positions)
    for read in (lambda: drv.nsteps, lambda: drv.pressure, lambda: drv.volume):
        with pytest.raises(RuntimeError, match=r"barostat of system\(s\) \[1\]"):
            read()
    assert twin.nsteps.tolist() == [1, 1, 1]


# ---- torch-sim ---------------------------------------------------------------------------------------------------------------------
class StubCalc:
    """What ``from_torchsim`` needs of a ``NequIPTorchSimCalc``: called with a state, returns forces, energies and stresses."""

    def __init__(self, systems, in_init=False):
        import cell_fire_restatement as C

        self.atomic_numbers_in_init, self.compute_stress, self.states = in_init, False, []
        self._step = C.torch_force_step([q["part"] for q in systems], "cpu")

    def __call__(self, state):
        self.states.append(SimpleNamespace(**vars(state)))
        out = self._step(state.positions, state.row_vector_cell)
        res = {"forces": out["forces"], "energy": out["total_energy"]}
        if self.compute_stress:
            res["stress"] = out["stress"]
        return res


def test_from_torchsim_hands_the_calculator_its_state():
    systems = B.batch((3, 5, 4))
    parts = [q["part"] for q in systems]
    x = torch.from_numpy(np.concatenate([p["x"] for p in parts]))
    cells = torch.from_numpy(np.stack([p["c0"] for p in parts]))
    m, v, sidx = B._cat(systems, "m", CPU), B._cat(systems, "v", CPU), B._sidx(systems, CPU)
    numbers = torch.arange(1, 13)
    calc = StubCalc(systems)
    drv = BatchedLangevin.from_torchsim(calc, x, cells, True, numbers, sidx, m, B.DT, [100.0, 200.0, 300.0], B.FRICTION,
                                        velocities=v, seed=[1, 2, 3])
    assert isinstance(drv, BatchedLangevin) and drv.seeds == [1, 2, 3] and not calc.compute_stress
    drv.run(2)
    seen = calc.states[-1]
    assert seen.positions is drv.positions and seen.row_vector_cell is cells and seen.pbc is True
    assert seen.atomic_numbers is numbers and seen.system_idx is sidx and len(calc.states) == 3
    assert drv.potential_energy.shape == (3,) and drv.target_temperature.tolist() == [100.0, 200.0, 300.0]
    calc = StubCalc(systems, in_init=True)
    BatchedLangevin.from_torchsim(calc, x, cells, True, numbers, sidx, m, B.DT, B.T, B.FRICTION)
    assert calc.states[-1].atomic_numbers is None

    calc = StubCalc(systems)
    npt = BatchedLangevinNPT.from_torchsim(calc, x, cells, True, numbers, sidx, m, B.DT, B.T, B.FRICTION, B.P0, B.COMPRESSIBILITY,
                                           B.TAUP, velocities=v, seed=7)
    assert calc.compute_stress and npt.seeds == [7, 8, 9]
    npt.run(2)
    seen = calc.states[-1]
    assert seen.row_vector_cell is npt.cell and seen.positions is npt.positions and seen.atomic_numbers is numbers
    assert not torch.equal(npt.cell, cells) and npt.stress.shape == (3, 3, 3)
    # the same sign as the driver's own force_step: the run is the one around the analytic step itself
    same = B.batched_npt(systems, CPU, dt=B.DT, temperature=B.T, friction=B.FRICTION, pressure=B.P0,
                         compressibility=B.COMPRESSIBILITY, taup=B.TAUP, seed=7)
    same.run(2)
    assert torch.equal(same.positions, npt.positions) and torch.equal(same.cell, npt.cell)
    calc = StubCalc(systems, in_init=True)
    BatchedLangevinNPT.from_torchsim(calc, x, cells, True, numbers, sidx, m, B.DT, B.T, B.FRICTION, B.P0, B.COMPRESSIBILITY, B.TAUP)
    assert calc.states[-1].atomic_numbers is None and calc.compute_stress


def test_remove_drift_acts_per_system():
    systems = B.batch((3, 5, 4))
    drv = B.batched_nvt(systems, CPU, remove_drift=True)
    for s, q in enumerate(systems):
        view = B.View(drv, s)
        p = (torch.from_numpy(q["m"])[:, None] * view.velocities).sum(0)
        assert float(p.abs().max()) < 1e-12 * float(np.abs(q["m"][:, None] * q["v"]).sum())
    one = Langevin(B.spring_force_step([systems[1]], CPU), torch.from_numpy(systems[1]["m"]), B.DT, B.T, B.FRICTION,
                   torch.from_numpy(systems[1]["x"]), torch.from_numpy(systems[1]["v"]), remove_drift=True)
    assert torch.equal(B.View(drv, 1).velocities.clone(), one.velocities.clone())


# ---- declared, bound and built -----------------------------------------------------------------------------------------------------
def test_kernels_are_declared_bound_and_built():
    from nequip_amd import _lib
    from nequip_amd.csrc import build

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nequip_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    arity = {"nqa_md_batched_langevin_step": 13, "nqa_md_batched_bath": 6, "nqa_md_batched_npt_bath": 10,
             "nqa_md_batched_npt_scale": 6}
    for name, count in arity.items():
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in nequip_amd.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == count
        declared = re.search(rf"\b{name}\s*\((.*?)\);", header, flags=re.S).group(1)
        assert declared.count(",") + 1 == count, f"{name}: the header declares another number of arguments"
    assert "md_batched.hip" in build.SOURCES and "md.hip" in build.SOURCES
    # the chunk the host writes word by word is the struct of the header, and its size is the one md_batched.hip asserts
    fields = re.search(r"typedef struct nqa_md_chunk \{(.*?)\}", header, flags=re.S).group(1)
    names = re.findall(r"\b([a-zA-Z0-9_]+)\s*[,;]", fields)
    assert names == list(MB._CHUNK_DTYPE.names) == ["component0", "local0", "count", "system"]
    source = open(os.path.join(ROOT, "nequip_amd", "csrc", "md_batched.hip")).read()
    size = re.search(r"static_assert\(sizeof\(nqa_md_chunk\) == (\d+)", source)
    assert size and int(size.group(1)) == MB._CHUNK_DTYPE.itemsize == 24
    assert MB.MD_THREADS == int(re.search(r"#define NQA_MD_THREADS (\d+)", header).group(1))
    # one definition of the generator and of the lane-0 arithmetic, in the header both files include
    shared = open(os.path.join(ROOT, "nequip_amd", "csrc", "md_device.h")).read()
    single = open(os.path.join(ROOT, "nequip_amd", "csrc", "md.hip")).read()
    for function in ("md_philox", "md_normal", "md_langevin_component", "md_bath_update", "md_npt_bath_update", "md_sum_rows"):
        assert len(re.findall(rf"void {function}\(|double {function}\(", shared)) == 1, function
        assert not re.search(rf"(void|double) {function}\(", single + source), f"{function} is defined twice"
        assert function in single + source
    assert '#include "md_device.h"' in single and '#include "md_device.h"' in source
