"""The device-resident FIRE optimizer (nequip_amd/integrations/relax.py), ATen form on the CPU: the driver against the float64
restatement of tests/fire_restatement.py (whose docstring derives the bounds), the restatement against the textbook loop, and
the host logic that needs no GPU.  The kernels are tested in tests/test_fire_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import fire_restatement as R
from nequip_amd.integrations import FIRE
from nequip_amd.integrations import relax as relax_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 300, 7)  # the systems of the batch below; alone, each is a single-system case


def make(n=7, seed=None, fdtype=torch.float64, fixed=None, fmax=1e-8, **params):
    """One system: the ATen driver on the CPU and its restatement."""
    k, x0, x = R.wells(n, seed=n if seed is None else seed)
    drv = FIRE(R.torch_force_step(k, x0, "cpu", fdtype), torch.from_numpy(x),
               fixed=None if fixed is None else torch.from_numpy(fixed), **params)
    drv._set_target(fmax)
    ref = R.Restated(R.restated_force(k, x0, "cpu", fdtype), x, fixed=fixed, fmax_target=fmax, **params)
    return drv, ref


def make_batch(sizes=SIZES, fdtype=torch.float64, fmax=1e-8, **params):
    """The systems of ``sizes`` concatenated, plus one that starts at its minimum; the restatements one by one."""
    parts = [R.wells(n, seed=n) for n in sizes]
    k_min, x0_min, _ = R.wells(4, seed=99)
    parts.append((k_min, x0_min, x0_min.copy()))
    k, x0, x = (np.concatenate([p[i] for p in parts]) for i in range(3))
    sidx = np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts])
    drv = FIRE(R.torch_force_step(k, x0, "cpu", fdtype), torch.from_numpy(x), system_idx=torch.from_numpy(sidx), **params)
    drv._set_target(fmax)
    refs = [R.Restated(R.restated_force(pk, px0, "cpu", fdtype), px, fmax_target=fmax, **params) for pk, px0, px in parts]
    return drv, refs


def run_all(refs, n):
    for ref in refs:
        ref.run(n)


# ---- the driver against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname, fdtype", [("f32", torch.float32), ("f64", torch.float64)])
@pytest.mark.parametrize("n", (1, 7, 300))
def test_aten_driver_matches_the_restatement(n, fname, fdtype):
    drv, ref = make(n, fdtype=fdtype)
    assert not drv._hip and drv.forces.dtype == fdtype
    drv.step(), ref.step()
    R.assert_close(drv, [ref], f"N={n} {fname} after 1 step")
    for _ in range(24):
        drv.step()
    ref.run(24)
    R.assert_close(drv, [ref], f"N={n} {fname} after 25 steps")
    assert int(drv.nsteps[0]) == 25 and min(ref.margins.values()) >= R.MARGIN


def test_a_batch_is_its_systems_one_by_one():
    drv, refs = make_batch()
    assert drv.num_systems == 4 and drv.fmax.shape == (4,) and drv.converged.dtype == torch.bool
    for _ in range(25):
        drv.step()
    run_all(refs, 25)
    R.assert_close(drv, refs, "batch after 25 steps")
    assert drv.nsteps.tolist() == [25, 25, 25, 0] and drv.converged.tolist() == [False, False, False, True]
    # every system alone takes the steps it takes inside the batch
    off = 0
    for s, n in enumerate(SIZES):
        alone, _ = make(n)
        for _ in range(25):
            alone.step()
        np.testing.assert_allclose(alone.positions.numpy(), drv.positions[off:off + n].numpy(), rtol=0, atol=R.bounds(refs[s], 25)[0])
        assert alone.dt[0] == drv.dt[s] and alone.a[0] == drv.a[s]
        off += n


def test_restatement_is_the_textbook_loop():
    """Over 50 steps and to 1e-12 relative: the step length from the three sums differs from the direct norm by rounding only.
    Positions element by element.  A velocity component is a sum of terms of either sign (cv v + cf F + dt F) that can cancel to
    far below the size of each, so the velocities are held to 1e-12 of the largest component of the velocity.  The runs pass
    through both branches, the growth of dt and the cap."""
    for n, params in ((7, {}), (40, {}), (7, dict(maxstep=0.05, dt=0.3))):
        k, x0, x = R.wells(n, seed=n)
        force = lambda y: R.force_numpy(y, k, x0)  # noqa: E731
        ref = R.Restated(force, x, fmax_target=1e-12, **params)
        ref.run(50)
        assert ref.nsteps == 50 and not ref.converged
        tx, tv = R.textbook(force, x, 50, **params)
        vmax = float(np.max(np.abs(tv)))
        worst = max(float(np.max(np.abs(ref.x - tx) / np.abs(tx))), float(np.max(np.abs(ref.v - tv))) / vmax)
        print(f"N={n} {params}: worst relative difference to the textbook loop {worst:.3e}; capped steps {ref.capped}, dt {ref.dt}")
        np.testing.assert_allclose(ref.x, tx, rtol=1e-12, atol=0)
        np.testing.assert_allclose(ref.v, tv, rtol=0, atol=1e-12 * vmax)
        assert ref.dt != R.DEFAULTS["dt"]  # (the time step moved)
    assert ref.capped > 0  # (the last case: the cap bound)


@pytest.mark.parametrize("n", (1, 7, 40))
def test_convergence_in_the_steps_of_the_restatement(n):
    drv, ref = make(n)
    want = ref.relax(1e-3)
    assert drv.run(fmax=1e-3, steps=2000) is True
    assert int(drv.nsteps[0]) == want and bool(drv.converged[0]) and float(drv.fmax[0]) < 1e-3
    R.assert_close(drv, [ref], f"N={n} converged after {want} steps")
    k, x0, _ = R.wells(n, seed=n)
    assert float(np.max(np.abs(drv.positions.numpy() - x0))) < 2e-3 / 0.5  # (|F| >= k |d|, k >= 0.5)
    # too few steps: the verdict says so, and check_every reads the same verdicts less often
    few, _ = make(n)
    assert few.run(fmax=1e-3, steps=3) is False and int(few.nsteps[0]) == 3
    sparse, _ = make(n)
    assert sparse.run(fmax=1e-3, steps=2000, check_every=7) is True
    assert int(sparse.nsteps[0]) == want and torch.equal(sparse.positions, drv.positions)


def test_the_cap_binds_when_maxstep_is_small():
    drv, ref = make(40, maxstep=0.01)
    first = drv.positions.clone()
    drv.step(), ref.step()
    assert ref.capped == 1
    moved = float(torch.linalg.norm(drv.positions - first))
    np.testing.assert_allclose(moved, 0.01, rtol=1e-12)
    for _ in range(9):
        before = drv.positions.clone()
        drv.step(), ref.step()
        assert float(torch.linalg.norm(drv.positions - before)) <= 0.01 * (1 + 1e-12)
    assert ref.capped == 10
    R.assert_close(drv, [ref], "maxstep = 0.01 after 10 steps")
    loose, loose_ref = make(40, maxstep=100.0)
    loose.step(), loose_ref.step()
    assert loose_ref.capped == 0 and float(torch.linalg.norm(loose.positions - first)) > 0.01


def test_fixed_atoms_never_move_and_do_not_enter_fmax():
    n = 12
    fixed = np.zeros(n, dtype=bool)
    fixed[[0, 5, 11]] = True
    k, x0, x = R.wells(n, seed=n)
    x[5] = x0[5] + np.array([3.0, 0.0, 0.0])  # by far the largest force of the system, on a fixed atom
    step, force = R.torch_force_step(k, x0, "cpu"), R.restated_force(k, x0, "cpu")
    drv = FIRE(step, torch.from_numpy(x), fixed=torch.from_numpy(fixed))
    ref = R.Restated(force, x, fixed=fixed)
    free = FIRE(step, torch.from_numpy(x))
    for _ in range(25):
        drv.step(), ref.step(), free.step()
    R.assert_close(drv, [ref], "three fixed atoms after 25 steps")
    assert np.array_equal(drv.positions.numpy()[fixed], x[fixed]) and not drv.velocities.numpy()[fixed].any()
    f_free_atoms = np.sqrt((R.force_numpy(ref.x, k, x0) ** 2).sum(1))
    assert float(drv.fmax[0]) < 0.5 * f_free_atoms[5] and float(free.fmax[0]) != float(drv.fmax[0])
    assert drv.run(fmax=1e-3, steps=2000) and np.array_equal(drv.positions.numpy()[fixed], x[fixed])


def test_a_system_at_its_minimum_converges_at_step_zero_without_nan():
    k, x0, _ = R.wells(9, seed=9)
    drv = FIRE(R.torch_force_step(k, x0, "cpu"), torch.from_numpy(x0.copy()))
    assert not drv.forces.any()
    assert drv.run(fmax=0.05, steps=10) is True
    assert int(drv.nsteps[0]) == 0 and float(drv.fmax[0]) == 0.0 and bool(drv.converged[0])
    assert np.array_equal(drv.positions.numpy(), x0) and not drv.velocities.any()
    for t in (drv.positions, drv.velocities, drv.dt, drv.a, drv.fmax):
        assert torch.isfinite(t).all()
    assert float(drv.dt[0]) == 0.1 and float(drv.a[0]) == 0.1


def test_state_dict_round_trip_continues_bit_for_bit():
    whole, _ = make_batch(fmax=1e-3)
    for _ in range(30):
        whole.step()
    first, _ = make_batch(fmax=1e-3)
    for _ in range(13):
        first.step()
    state = first.state_dict()
    assert state["nsteps"].tolist() == [13, 13, 13, 0]
    second, _ = make_batch(fmax=0.7, dt=0.03, maxstep=0.01, nmin=1)
    for _ in range(4):
        second.step()
    second.load_state_dict(state)
    for _ in range(17):
        second.step()
    for name in ("positions", "velocities", "dt", "a", "nsteps", "fmax", "converged", "_npos"):
        assert torch.equal(getattr(second, name), getattr(whole, name)), name
    with pytest.raises(ValueError, match="atoms"):
        make(5)[0].load_state_dict(state)


def test_a_nan_force_is_reported():
    k, x0, x = R.wells(5, seed=5)
    good = R.torch_force_step(k, x0, "cpu")
    calls = []

    def step(pos):
        out = good(pos)
        calls.append(1)
        if len(calls) == 4:
            out["forces"][2, 1] = float("nan")
        return out

    drv = FIRE(step, torch.from_numpy(x))
    with pytest.raises(FloatingPointError, match="fmax of system 0"):
        drv.run(fmax=1e-3, steps=50)


# ---- host logic ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    k, x0, x = R.wells(6, seed=6)
    step, pos = R.torch_force_step(k, x0, "cpu"), torch.from_numpy(x)
    sidx = torch.tensor([0, 0, 1, 1, 2, 2])
    with pytest.raises(ValueError, match="system_idx must .* never decrease"):
        FIRE(step, pos, system_idx=torch.tensor([0, 0, 1, 0, 2, 2]))
    with pytest.raises(ValueError, match=r"positions must have shape \[N, 3\]"):
        FIRE(step, pos.reshape(3, 6))
    with pytest.raises(ValueError, match=r"system_idx must be a tensor of shape \[6\]"):
        FIRE(step, pos, system_idx=sidx[:5])
    with pytest.raises(ValueError, match=r"fixed must be a tensor of shape \[6\]"):
        FIRE(step, pos, fixed=torch.zeros(6, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="mixed devices: positions on cpu, system_idx on meta"):
        FIRE(step, pos, system_idx=sidx.to("meta"))
    with pytest.raises(ValueError, match="mixed devices: positions on cpu, fixed on meta"):
        FIRE(step, pos, fixed=torch.zeros(6, dtype=torch.bool, device="meta"))
    for kwargs, message in ((dict(dt=0.0), "dt must be positive"), (dict(dt=-0.1), "dt must be positive"),
                            (dict(maxstep=0.0), "maxstep must be positive"), (dict(fdec=1.0), r"fdec must lie in \(0, 1\)"),
                            (dict(fdec=0.0), r"fdec must lie in \(0, 1\)"), (dict(finc=0.9), "finc must be at least 1"),
                            (dict(nmin=-1), "nmin must be a non-negative integer"), (dict(backend="cuda"), "backend must be"),
                            (dict(backend="hip"), "backend='hip' needs device tensors")):
        with pytest.raises(ValueError, match=message):
            FIRE(step, pos, **kwargs)
    with pytest.raises(TypeError, match="force_step must be callable"):
        FIRE(None, pos)
    drv = FIRE(step, pos)
    with pytest.raises(ValueError, match="fmax must be positive"):
        drv.run(fmax=0.0)
    with pytest.raises(ValueError, match="check_every"):
        drv.run(check_every=0)
    with pytest.raises(ValueError, match="force_step must return float32 or float64 forces"):
        FIRE(lambda p: {"forces": p[:3], "total_energy": p.sum()}, pos)


def test_chunk_table_never_straddles_two_systems():
    chunks, begin = relax_module.fire_chunk_table(np.array([1, 257, 0, 256, 600]), 256)
    assert begin.tolist() == [0, 1, 3, 3, 4, 7]
    assert chunks["atom0"].tolist() == [0, 1, 257, 258, 514, 770, 1026]
    assert chunks["count"].tolist() == [1, 256, 1, 256, 256, 256, 88]
    assert chunks["system"].tolist() == [0, 1, 1, 3, 4, 4, 4]
    assert chunks.dtype.itemsize == 16 and int(chunks["count"].sum()) == 1114


def test_from_atoms_and_write_back():
    from nosehoover_restatement import FakeAtoms

    k, x0, x = R.wells(5, seed=5)
    atoms = FakeAtoms(["H"] * 5, x, np.ones(5))
    drv = FIRE.from_atoms(atoms, R.torch_force_step(k, x0, "cpu"), device="cpu", maxstep=0.1)
    ref = R.Restated(R.restated_force(k, x0, "cpu"), x, maxstep=0.1)
    for _ in range(5):
        drv.step(), ref.step()
    R.assert_close(drv, [ref], "from_atoms")
    drv.write_back(atoms)
    assert np.array_equal(atoms.get_positions(), drv.positions.numpy())
    assert drv.potential_energy.shape == (1,) and torch.isfinite(drv.potential_energy).all()
    model = torch.nn.Linear(1, 1).eval()
    model.type_names = ["H"]
    with pytest.raises(ValueError, match="r_max"):
        FIRE.from_atoms(atoms, model, device="cpu")


def test_kernels_are_declared_bound_and_built():
    from nequip_amd import _lib
    from nequip_amd.csrc import build

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nequip_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ("nqa_fire_chunk_atoms", "nqa_fire_reduce", "nqa_fire_decide", "nqa_fire_move"):
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in nequip_amd.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert [len(_lib.SIGNATURES[n][1]) for n in ("nqa_fire_reduce", "nqa_fire_decide", "nqa_fire_move")] == [8, 5, 9]
    assert "relax.hip" in build.SOURCES
    chunk = int(re.search(r"#define NQA_FIRE_CHUNK (\d+)", header).group(1))
    assert lib.nqa_fire_chunk_atoms() == chunk == 256
    # the record the host writes word by word is the struct of the header, and its size is the one relax.hip asserts
    fields = re.search(r"typedef struct nqa_fire_system \{(.*?)\}", header, flags=re.S).group(1)
    names = re.findall(r"\b([a-zA-Z0-9_]+)\s*[,;]", fields)
    assert names == ["dt", "a", "npos", "nsteps", "dtmax", "maxstep", "finc", "fdec", "astart", "fa", "fmax_target", "nmin",
                     "converged", "cv", "cf", "scale", "fmax"]
    assert re.search(r"int32_t nmin, converged;", fields)  # (the two halves of word 11)
    M = relax_module
    assert [M._DT, M._A, M._NPOS, M._NSTEPS, M._DTMAX, M._MAXSTEP, M._FINC, M._FDEC, M._ASTART, M._FA, M._TARGET,
            M._NMIN_CONVERGED, M._CV, M._CF, M._SCALE, M._FMAX] == list(range(16))
    source = open(os.path.join(ROOT, "nequip_amd", "csrc", "relax.hip")).read()
    assert re.search(r"static_assert\(sizeof\(nqa_fire_system\) == 128", source)
    assert re.search(r"static_assert\(sizeof\(nqa_fire_chunk\) == 16", source)
    assert "#pragma clang fp contract(off)" in source and "atomic" not in re.sub(r"//.*", "", source)
