"""The variable-cell FIRE optimizer (nequip_amd.integrations.CellFIRE), ATen form on the CPU: the test potential against finite
differences, the restatement of tests/cell_fire_restatement.py (whose docstring derives the bounds) against the literal filter
and FIRE loop, the driver against the restatement, and the host logic that needs no GPU.  The kernels are tested in
tests/test_cell_fire_gpu.py."""
import os
import re

import numpy as np
import pytest
import torch

import cell_fire_restatement as R
from nequip_amd.integrations import FIRE, CellFIRE
from nequip_amd.integrations import relax as relax_module

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1, 40, 7)
C_AXIS_FROZEN = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
CONSTRAINTS = {"scalar_pressure": dict(scalar_pressure=0.1), "hydrostatic_strain": dict(hydrostatic_strain=True),
               "constant_volume": dict(constant_volume=True), "mask": dict(mask=C_AXIS_FROZEN)}


def batch_parts(sizes=SIZES):
    return [R.site_system(n, seed=n) for n in sizes]


def make(parts, fdtype=torch.float64, fmax=1e-8, fixed=None, **options):
    """The ATen driver on the CPU over the systems of ``parts`` and their restatements one by one."""
    c = R.concatenated(parts)
    drv = CellFIRE(R.torch_force_step(parts, "cpu", fdtype), torch.from_numpy(c["x"]), torch.from_numpy(c["c0"]),
                   system_idx=torch.from_numpy(c["sidx"]) if len(parts) > 1 else None,
                   fixed=None if fixed is None else torch.from_numpy(fixed),
                   **{k: (torch.from_numpy(v) if isinstance(v, np.ndarray) else v) for k, v in options.items()})
    drv._set_target(fmax)
    off = c["offsets"]
    per_system = isinstance(options.get("cell_factor"), np.ndarray)
    refs = [R.Restated(R.restated_force(p, "cpu", fdtype), p["x"], p["c0"], fmax_target=fmax,
                       fixed=None if fixed is None else fixed[off[s]:off[s + 1]],
                       **dict(options, **({"cell_factor": float(options["cell_factor"][s])} if per_system else {})))
            for s, p in enumerate(parts)]
    return drv, refs


def run(drv, refs, n):
    for _ in range(n):
        drv.step()
    for ref in refs:
        ref.run(n)


# ---- the potential and the restatement -------------------------------------------------------------------------------------------
def test_potential_forces_and_stress_are_derivatives_of_the_energy():
    """Central differences with h = 1e-5: the truncation error is h^2 / 6 times a third derivative of order 10, the rounding
    error eps |E| / h with |E| of order 10: both below 1e-8, held to 1e-7."""
    part = R.site_system(7, seed=7)
    x, cell = part["x"], part["c0"]
    force = R.numpy_force(part)
    f, sigma = force(x, cell)
    h, worst_f, worst_s = 1e-5, 0.0, 0.0
    for i in range(7):
        for j in range(3):
            dx = np.zeros_like(x)
            dx[i, j] = h
            fd = -(R.numpy_energy(part, x + dx, cell) - R.numpy_energy(part, x - dx, cell)) / (2 * h)
            worst_f = max(worst_f, abs(fd - f[i, j]))
    vol = abs(np.linalg.det(cell))
    for i in range(3):
        for j in range(i, 3):
            eps = np.zeros((3, 3))
            eps[i, j] += 0.5 * h
            eps[j, i] += 0.5 * h
            plus, minus = np.eye(3) + eps, np.eye(3) - eps
            fd = (R.numpy_energy(part, x @ plus, cell @ plus) - R.numpy_energy(part, x @ minus, cell @ minus)) / (2 * h) / vol
            worst_s = max(worst_s, abs(fd - sigma[i, j]))
    print(f"forces off by {worst_f:.3e}, stress off by {worst_s:.3e}")
    assert worst_f < 1e-7 and worst_s < 1e-7
    assert np.array_equal(sigma, sigma.T) and float(np.abs(sigma).max()) > 1e-3


@pytest.mark.parametrize("n", (1, 7))
def test_restatement_is_the_literal_filter_and_fire_loop(n):
    """Over 60 steps: the three-launch form (q carried, the step length from the sums of the old velocities) against the
    filter's get_positions / get_forces / set_positions around FIRE with q re-solved from x at every step."""
    part = R.site_system(n, seed=n)
    force = R.numpy_force(part)
    ref = R.Restated(force, part["x"], part["c0"], fmax_target=1e-12)
    ref.run(60)
    assert ref.nsteps == 60 and not ref.converged and ref.dt != R.DEFAULTS["dt"]
    tx, tcell, tv = R.textbook(force, part["x"], part["c0"], 60)
    worst = max(float(np.max(np.abs(ref.x - tx))), float(np.max(np.abs(ref.cell - tcell))))
    print(f"n={n}: positions and cell within {worst:.3e} A of the literal loop; margins {ref.margins}")
    np.testing.assert_allclose(ref.x, tx, rtol=1e-12, atol=0)
    np.testing.assert_allclose(ref.cell, tcell, rtol=0, atol=1e-12)
    vmax = float(np.max(np.abs(tv)))
    np.testing.assert_allclose(np.concatenate([ref.v, ref.vD]), tv, rtol=0, atol=1e-12 * vmax)


def test_restatement_converges_and_lowers_the_enthalpy():
    part = R.site_system(7, seed=7)
    ref = R.Restated(R.numpy_force(part), part["x"], part["c0"])
    e0 = R.numpy_energy(part, ref.x, ref.cell)
    steps = ref.relax(1e-3)
    print(f"7 atoms: fmax < 1e-3 after {steps} steps")
    assert steps < 400 and R.numpy_energy(part, ref.x, ref.cell) < e0


# ---- the driver against the restatement ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname, fdtype", [("f32", torch.float32), ("f64", torch.float64)])
@pytest.mark.parametrize("n", (1, 7, 300))
def test_aten_driver_matches_the_restatement(n, fname, fdtype):
    drv, refs = make([R.site_system(n, seed=n)], fdtype=fdtype)
    assert not drv._hip and drv.forces.dtype == fdtype and drv.stress.dtype == fdtype and drv.stress.shape == (1, 3, 3)
    run(drv, refs, 1)
    R.assert_close(drv, refs, f"N={n} {fname} after 1 step")
    run(drv, refs, 24)
    R.assert_close(drv, refs, f"N={n} {fname} after 25 steps")
    assert int(drv.nsteps[0]) == 25 and min(refs[0].margins.values()) >= R.MARGIN
    assert not torch.equal(drv.cell[0], drv.reference_cell[0])  # (the cell moved)
    np.testing.assert_allclose(drv.volume.numpy(), [abs(np.linalg.det(refs[0].cell))], rtol=1e-12)


def test_a_batch_is_its_systems_one_by_one():
    parts = batch_parts() + [R.site_system(4, seed=99, at_minimum=True)]
    drv, refs = make(parts)
    assert drv.num_systems == 4 and drv.cell.shape == (4, 3, 3) and drv.deform_grad.shape == (4, 3, 3)
    run(drv, refs, 25)
    R.assert_close(drv, refs, "batch after 25 steps")
    assert drv.nsteps.tolist() == [25, 25, 25, 0] and drv.converged.tolist() == [False, False, False, True]
    off = 0
    for s, part in enumerate(parts[:3]):
        n = len(part["k"])
        alone, _ = make([part])
        for _ in range(25):
            alone.step()
        x_atol, _, d_atol, _, _ = R.bounds(refs[s], 25)
        np.testing.assert_allclose(alone.positions.numpy(), drv.positions[off:off + n].numpy(), rtol=0, atol=2 * x_atol)
        np.testing.assert_allclose(alone.deform_grad[0].numpy(), drv.deform_grad[s].numpy(), rtol=0, atol=2 * d_atol)
        assert alone.dt[0] == drv.dt[s] and alone.a[0] == drv.a[s]
        off += n


def test_a_converged_system_is_never_touched_again():
    """The fourth system starts at its minimum, atoms and cell: no step moves its atoms, its cell or its record."""
    parts = batch_parts() + [R.site_system(4, seed=99, at_minimum=True)]
    drv, _ = make(parts, fmax=1e-3)
    assert not drv.forces[-4:].any() and not drv.stress[3].any()
    for _ in range(10):
        drv.step()
    assert drv.nsteps.tolist() == [10, 10, 10, 0] and float(drv.fmax[3]) == 0.0 and bool(drv.converged[3])
    assert np.array_equal(drv.positions[-4:].numpy(), parts[3]["x"]) and not drv.velocities[-4:].any()
    assert np.array_equal(drv.cell[3].numpy(), parts[3]["c0"]) and np.array_equal(drv.deform_grad[3].numpy(), np.eye(3))
    assert not drv.cell_velocities[3].any() and float(drv.dt[3]) == 0.1 and float(drv.a[3]) == 0.1
    # a run to convergence stops moving every system it has found converged
    one, refs = make([R.site_system(7, seed=7)], fmax=1e-3)
    want = refs[0].relax(1e-3)
    assert one.run(fmax=1e-3, steps=2000) is True and int(one.nsteps[0]) == want
    R.assert_close(one, refs, f"converged after {want} steps")
    before = {name: getattr(one, name).clone() for name in ("positions", "velocities", "cell", "deform_grad", "cell_velocities")}
    for _ in range(3):
        one.step()
    assert int(one.nsteps[0]) == want and all(torch.equal(before[name], getattr(one, name)) for name in before)


@pytest.mark.parametrize("name", sorted(CONSTRAINTS))
def test_each_constraint_changes_the_trajectory_the_way_the_restatement_says(name):
    part = R.site_system(7, seed=7)
    options = CONSTRAINTS[name]
    drv, refs = make([part], **options)
    free, free_refs = make([part])
    run(drv, refs, 25)
    run(free, free_refs, 25)
    R.assert_close(drv, refs, f"{name} after 25 steps")
    D, D_free = drv.deform_grad[0].numpy(), free.deform_grad[0].numpy()
    assert float(np.abs(D - D_free).max()) > 1e-6, "the constraint changed nothing"
    if name == "hydrostatic_strain":  # G = (tr G / 3) I: the cell scales, and nothing else
        assert D[0, 0] == D[1, 1] == D[2, 2] != 1.0 and not (D - np.diag(np.diag(D))).any()
    if name == "mask":
        assert np.array_equal(D[2], [0.0, 0.0, 1.0]) and not np.array_equal(D[0], [1.0, 0.0, 0.0])
        assert np.array_equal(drv.cell[0].numpy()[:, 2], part["c0"][:, 2])
    if name == "constant_volume":  # the cell velocity is traceless up to rounding
        vD = drv.cell_velocities[0].numpy()
        assert abs(np.trace(vD)) <= 1e-12 * np.abs(vD).max() and abs(np.trace(free.cell_velocities[0].numpy())) > 1e-6
    if name == "scalar_pressure":  # an outer pressure leaves a smaller cell
        assert float(drv.volume[0]) < float(free.volume[0])


def test_fixed_atoms_follow_the_cell_and_do_not_enter_fmax():
    n = 12
    part = R.site_system(n, seed=n)
    fixed = np.zeros(n, dtype=bool)
    fixed[[0, 5, 11]] = True
    part["x"][5] += np.array([2.0, 0.0, 0.0])  # by far the largest force of the system, on a fixed atom
    drv, refs = make([part], fixed=fixed)
    free, _ = make([part])
    run(drv, refs, 1)
    free.step()
    assert float(drv.fmax[0]) < 0.5 * float(free.fmax[0])
    run(drv, refs, 24)
    R.assert_close(drv, refs, "three fixed atoms after 25 steps")
    assert not drv.velocities.numpy()[fixed].any()
    # q of a fixed atom is its first position; x follows the cell
    want = part["x"][fixed] @ drv.deform_grad[0].numpy().T
    np.testing.assert_allclose(drv.positions.numpy()[fixed], want, rtol=1e-14)
    assert not np.array_equal(drv.positions.numpy()[fixed], part["x"][fixed])


def test_cell_factor_defaults_to_the_number_of_atoms():
    parts = batch_parts()
    default, _ = make(parts)
    explicit, refs = make(parts, cell_factor=np.array([float(n) for n in SIZES]))
    other, other_refs = make(parts, cell_factor=3.0)
    assert [ref.cell_factor for ref in refs] == [1.0, 40.0, 7.0] and [ref.cell_factor for ref in other_refs] == [3.0] * 3
    run(default, [], 10)
    run(explicit, refs, 10)
    run(other, other_refs, 10)
    assert torch.equal(default.positions, explicit.positions) and torch.equal(default.cell, explicit.cell)
    R.assert_close(explicit, refs, "cell_factor per system")
    R.assert_close(other, other_refs, "cell_factor = 3")
    assert not torch.equal(other.cell[1], default.cell[1])


def test_state_dict_round_trip_continues_bit_for_bit():
    parts = batch_parts() + [R.site_system(4, seed=99, at_minimum=True)]
    whole, _ = make(parts, fmax=1e-3, hydrostatic_strain=True)
    for _ in range(30):
        whole.step()
    first, _ = make(parts, fmax=1e-3, hydrostatic_strain=True)
    for _ in range(13):
        first.step()
    state = first.state_dict()
    assert state["nsteps"].tolist() == [13, 13, 13, 0]
    assert {"q", "velocities", "D", "vD", "C0", "dt", "a", "npos", "nsteps"} <= set(state)
    second, _ = make(parts, fmax=0.7, dt=0.03, maxstep=0.01, nmin=1, constant_volume=True)
    for _ in range(4):
        second.step()
    second.load_state_dict(state)
    for _ in range(17):
        second.step()
    for name in ("positions", "velocities", "cell", "deform_grad", "cell_velocities", "dt", "a", "nsteps", "fmax", "converged",
                 "_npos", "stress"):
        assert torch.equal(getattr(second, name), getattr(whole, name)), name
    with pytest.raises(ValueError, match="atoms"):
        make([R.site_system(5, seed=5)])[0].load_state_dict(state)


FROZEN_SIZES = (1, 40, 7, 257)  # 257: one atom past a chunk of NQA_FIRE_CHUNK = 256, so a system with two rows to merge


def frozen_cell_pair(device, fdtype, backend):
    """``(CellFIRE, FIRE, C0)`` over one batch of ``FROZEN_SIZES`` atoms with every fifth atom from atom 2 fixed: ``CellFIRE``
    with ``mask = 0``, ``FIRE`` around the same potential evaluated at the constant initial cells ``C0``."""
    parts = [R.site_system(n, seed=n) for n in FROZEN_SIZES]
    c = R.concatenated(parts)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    step = R.torch_force_step(parts, device, fdtype)
    fixed = np.zeros(len(c["x"]), dtype=bool)
    fixed[2::5] = True
    c0 = on(c["c0"])
    cell_fire = CellFIRE(step, on(c["x"]), c0, system_idx=on(c["sidx"]), fixed=on(fixed), mask=torch.zeros(3, 3), backend=backend)
    fire = FIRE(lambda pos: step(pos, c0), on(c["x"]), system_idx=on(c["sidx"]), fixed=on(fixed), backend=backend)
    return cell_fire, fire, c0


def assert_frozen_cell_is_fire(cell_fire, fire, c0, steps=40):
    """``steps`` steps of both towards ``fmax = 1e-9`` (nothing converges except by the dynamics), then the whole FIRE state bit
    for bit and the cell where it was."""
    for drv in (cell_fire, fire):
        drv._set_target(1e-9)
        for _ in range(steps):
            drv.step()
    assert fire.nsteps.tolist() == [steps] * len(FROZEN_SIZES) and bool((fire.dt != 0.1).all())  # (every system took branches)
    for name in ("positions", "velocities", "dt", "a", "fmax", "nsteps", "_npos"):
        assert torch.equal(getattr(cell_fire, name), getattr(fire, name)), name
    assert torch.equal(cell_fire.cell, c0)


@pytest.mark.parametrize("fname, fdtype", [("f32", torch.float32), ("f64", torch.float64)])
def test_cell_fire_with_a_frozen_cell_is_fire_bit_for_bit(fname, fdtype):
    """With ``mask = 0`` the cell's force is ``G = +-0``: ``D`` stays the identity, ``g = F I = F`` and ``x = q I = q`` exactly,
    and the cell's rows add ``+-0`` to ``P, FF, VV`` and 0 to the max.  What is left is the decision both optimizers share."""
    cell_fire, fire, c0 = frozen_cell_pair("cpu", fdtype, "aten")
    assert not cell_fire._hip and not fire._hip
    assert_frozen_cell_is_fire(cell_fire, fire, c0)


def test_a_nan_stress_is_reported():
    part = R.site_system(5, seed=5)
    good = R.torch_force_step([part], "cpu")
    calls = []

    def step(pos, cell):
        out = good(pos, cell)
        calls.append(1)
        if len(calls) == 4:
            out["stress"][0, 1, 2] = float("nan")
        return out

    drv = CellFIRE(step, torch.from_numpy(part["x"]), torch.from_numpy(part["c0"]))
    with pytest.raises(FloatingPointError, match="fmax of system 0"):
        drv.run(fmax=1e-3, steps=50)


# ---- host logic ------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_argument():
    part = R.site_system(6, seed=6)
    step, pos, cell = R.torch_force_step([part], "cpu"), torch.from_numpy(part["x"]), torch.from_numpy(part["c0"])
    no_stress = lambda p, c: {k: v for k, v in step(p, c).items() if k != "stress"}  # noqa: E731
    with pytest.raises(ValueError, match="stress"):
        CellFIRE(no_stress, pos, cell)
    with pytest.raises(ValueError, match=r"stress: .* \[1, 3, 3\], got .*\(3,\)"):
        CellFIRE(lambda p, c: dict(step(p, c), stress=step(p, c)["stress"][0, 0]), pos, cell)
    singular = cell.clone()
    singular[2] = singular[0] + singular[1]
    with pytest.raises(ValueError, match="cell of system 0 is singular"):
        CellFIRE(step, pos, singular)
    with pytest.raises(ValueError, match=r"cell must be a tensor of shape \[3, 3\] or \[1, 3, 3\]"):
        CellFIRE(step, pos, cell.reshape(9))
    with pytest.raises(ValueError, match=r"mask must have shape \[3, 3\]"):
        CellFIRE(step, pos, cell, mask=torch.ones(6))
    with pytest.raises(ValueError, match="mask must hold zeros and ones"):
        CellFIRE(step, pos, cell, mask=0.5 * torch.ones(3, 3))
    with pytest.raises(ValueError, match="cell_factor must be positive"):
        CellFIRE(step, pos, cell, cell_factor=0.0)
    with pytest.raises(ValueError, match="cell_factor must be a number or hold one per system"):
        CellFIRE(step, pos, cell, cell_factor=[1.0, 2.0])
    with pytest.raises(ValueError, match="scalar_pressure must be finite"):
        CellFIRE(step, pos, cell, scalar_pressure=float("inf"))
    with pytest.raises(ValueError, match="mixed devices: positions on cpu, cell on meta"):
        CellFIRE(step, pos, cell.to("meta"))
    with pytest.raises(ValueError, match="dt must be positive"):
        CellFIRE(step, pos, cell, dt=0.0)
    with pytest.raises(ValueError, match="backend='hip' needs device tensors"):
        CellFIRE(step, pos, cell, backend="hip")
    with pytest.raises(TypeError, match="force_step must be callable"):
        CellFIRE(None, pos, cell)


def test_set_cell_from_device_refuses_a_non_periodic_direction():
    from nequip_amd.integrations.graphed_step import GraphedStep

    step = object.__new__(GraphedStep)  # (the check of the periodicity comes first: no GPU is needed to meet it)
    step._pbc = (True, True, False)
    with pytest.raises(ValueError, match="all three directions periodic"):
        step.set_cell_from_device(torch.eye(3, dtype=torch.float64))


class _Atoms:
    def __init__(self, positions, cell):
        self.p, self.c = np.array(positions), np.array(cell)

    def get_positions(self):
        return self.p.copy()

    def get_cell(self):
        return self.c

    def get_pbc(self):
        return np.array([True] * 3)

    def set_positions(self, p):
        self.p = np.array(p, dtype=np.float64)

    def set_cell(self, c, scale_atoms=False):
        assert not scale_atoms
        self.c = np.array(c, dtype=np.float64)


def test_from_atoms_and_write_back():
    part = R.site_system(5, seed=5)
    atoms = _Atoms(part["x"], part["c0"])
    drv = CellFIRE.from_atoms(atoms, R.torch_force_step([part], "cpu"), device="cpu", maxstep=0.1)
    ref = R.Restated(R.restated_force(part, "cpu"), part["x"], part["c0"], maxstep=0.1)
    for _ in range(5):
        drv.step(), ref.step()
    R.assert_close(drv, [ref], "from_atoms")
    drv.write_back(atoms)
    assert np.array_equal(atoms.get_positions(), drv.positions.numpy()) and np.array_equal(atoms.get_cell(), drv.cell[0].numpy())
    assert drv.potential_energy.shape == (1,) and torch.isfinite(drv.potential_energy).all()


def test_kernels_are_declared_bound_and_built():
    from nequip_amd import _lib
    from nequip_amd.csrc import build

    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "nequip_amd.h")).read(), flags=re.S)
    lib = _lib.load()
    names = ("nqa_cellfire_reduce", "nqa_cellfire_decide", "nqa_cellfire_move")
    for name in names:
        declaration = re.search(rf"\bint {name}\s*\((.*?)\);", header, flags=re.S)
        assert declaration, f"{name} is not declared in nequip_amd.h"
        assert name in _lib.SIGNATURES and hasattr(lib, name)
        assert len(_lib.SIGNATURES[name][1]) == declaration.group(1).count(",") + 1, f"{name}: arguments bound and declared"
    assert [len(_lib.SIGNATURES[n][1]) for n in names] == [9, 8, 10]
    assert "relax_cell.hip" in build.SOURCES and "relax.hip" in build.SOURCES
    # the record the host writes word by word is the struct of the header
    fields = re.search(r"typedef struct nqa_cellfire_system \{(.*?)\}", header, flags=re.S).group(1)
    words, at = {}, 0
    for ctype, decl in re.findall(r"\b(double|int64_t|int32_t)\s+([^;]+);", fields):
        for item in decl.split(","):
            name, count = re.match(r"\s*([a-zA-Z0-9_]+)(?:\[(\d+)\])?", item).groups()
            words[name] = at / 8
            at += (4 if ctype == "int32_t" else 8) * int(count or 1)
    assert at == 512
    M = relax_module
    assert [words[k] for k in ("dt", "a", "npos", "nsteps", "dtmax", "maxstep", "finc", "fdec", "astart", "fa", "fmax_target", "nmin",
                               "converged", "cv", "cf", "scale", "fmax")] == \
        [M._DT, M._A, M._NPOS, M._NSTEPS, M._DTMAX, M._MAXSTEP, M._FINC, M._FDEC, M._ASTART, M._FA, M._TARGET, M._NMIN_CONVERGED,
         M._NMIN_CONVERGED + 0.5, M._CV, M._CF, M._SCALE, M._FMAX]
    assert [words[k] for k in ("cell_factor", "pressure", "hydrostatic", "constant_volume", "mask", "c0", "d_old", "d_new", "vd")] == \
        [M._CELL_FACTOR, M._PRESSURE, M._HYDROSTATIC_CONSTVOL, M._HYDROSTATIC_CONSTVOL + 0.5, M._MASK, M._C0, M._D_OLD, M._D_NEW,
         M._VD]
    assert M._CELL_WORDS * 8 == at and len(words) == 26
    source = open(os.path.join(ROOT, "nequip_amd", "csrc", "relax_cell.hip")).read()
    assert re.search(r"static_assert\(sizeof\(nqa_cellfire_system\) == 512", source)
    assert re.search(r"static_assert\(sizeof\(nqa_cellfire_system\) % 8 == 0", source)
    assert "#pragma clang fp contract(off)" in source and "atomic" not in re.sub(r"//.*", "", source)
    # the fixed-cell record is what it was
    fire = re.search(r"typedef struct nqa_fire_system \{(.*?)\}", header, flags=re.S).group(1)
    assert re.findall(r"\b([a-zA-Z0-9_]+)\s*[,;]", fire) == ["dt", "a", "npos", "nsteps", "dtmax", "maxstep", "finc", "fdec", "astart",
                                                            "fa", "fmax_target", "nmin", "converged", "cv", "cf", "scale", "fmax"]
    assert M._WORDS == 16 and re.search(r"static_assert\(sizeof\(nqa_fire_system\) == 128",
                                        open(os.path.join(ROOT, "nequip_amd", "csrc", "relax.hip")).read())
