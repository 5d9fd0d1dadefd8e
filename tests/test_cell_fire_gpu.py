"""The variable-cell FIRE kernels (csrc/relax_cell.hip: nqa_cellfire_reduce + nqa_cellfire_decide + nqa_cellfire_move) under
nequip_amd.integrations.CellFIRE, against the float64 restatement of tests/cell_fire_restatement.py at the bounds its docstring
derives, and bit for bit against themselves.

Sizes: with C = nqa_fire_chunk_atoms() atoms per chunk, 1, C - 1, C, C + 1 and 64 C + 1 atoms are a fraction of one chunk, one
atom short of a chunk, a full chunk, the first atom of a second chunk, and 65 chunks, i.e. more rows of partial sums than the 64
lanes of the decide wavefront take one each.  Forces and stress come from one analytic potential evaluated in torch on the device
(restatement included, so that a float32 force is the same number on both sides): only the optimizer is under test."""
import copy
import functools

import numpy as np
import pytest
import torch

import cell_fire_restatement as R
from nequip_amd.integrations import CellFIRE
from test_cell_fire import assert_frozen_cell_is_fire, frozen_cell_pair

pytestmark = pytest.mark.gpu

C = 256
SIZES = (1, C - 1, C, C + 1, 64 * C + 1)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
TIGHT = 1e-8  # a target no case here reaches in 25 steps
C_AXIS_FROZEN = np.array([[1.0, 1.0, 1.0], [1.0, 1.0, 1.0], [0.0, 0.0, 0.0]])
CONSTRAINTS = {"scalar_pressure": dict(scalar_pressure=0.1), "hydrostatic_strain": dict(hydrostatic_strain=True),
               "constant_volume": dict(constant_volume=True), "mask": dict(mask=C_AXIS_FROZEN)}


def minimum_system():
    return R.site_system(4, seed=99, at_minimum=True)


def driver(device, parts, fdtype, backend="hip", fmax=TIGHT, fixed=None, **options):
    c = R.concatenated(parts)
    on = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)  # noqa: E731
    drv = CellFIRE(R.torch_force_step(parts, device, fdtype), on(c["x"]), on(c["c0"]),
                   system_idx=on(c["sidx"]) if len(parts) > 1 else None, fixed=None if fixed is None else on(fixed),
                   backend=backend, **{k: (on(v) if isinstance(v, np.ndarray) else v) for k, v in options.items()})
    drv._set_target(fmax)
    return drv


def restatements(device, parts, fdtype, fmax=TIGHT, fixed=None, **options):
    assert fixed is None or len(parts) == 1
    return [R.Restated(R.restated_force(p, device, fdtype), p["x"], p["c0"], fmax_target=fmax, fixed=fixed, **options) for p in parts]


@functools.lru_cache(maxsize=None)
def reference(device, n, fname):
    """The restatement of the single system of ``n`` atoms after 1 and after 25 steps (computed once, never modified)."""
    (ref,) = restatements(device, [R.site_system(n, seed=n)], DTYPES[fname])
    ref.run(1)
    one = copy.copy(ref)
    ref.run(24)
    return one, ref


def _run(refs, n):
    for ref in refs:
        ref.run(n)
    return refs


def state_of(drv):
    """Every buffer of the driver, cloned."""
    return {"positions": drv.positions.clone(), "coords": drv._q.clone(), "velocities": drv.velocities.clone(),
            "record": drv._rec.view(torch.int64).clone(), "partials": drv._partials.clone(), "cell": drv.cell.clone()}


def same_bits(a, b):
    sa, sb = state_of(a), state_of(b)
    return all(torch.equal(sa[name], sb[name]) for name in sa)


# ---- against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_single_system_matches_the_restatement(device, n, fname):
    one, last = reference(device, n, fname)
    drv = driver(device, [R.site_system(n, seed=n)], DTYPES[fname])
    assert drv._hip and drv.forces.dtype == DTYPES[fname] and drv.stress.dtype == DTYPES[fname]
    assert drv._n_chunks == (n + C - 1) // C and drv._rec.shape == (1, 64)
    drv.step()
    R.assert_close(drv, [one], f"N={n} {fname} after 1 step")
    for _ in range(24):
        drv.step()
    R.assert_close(drv, [last], f"N={n} {fname} after 25 steps")
    assert last.nsteps == 25 and min(last.margins.values()) >= R.MARGIN
    assert not torch.equal(drv.cell, drv.reference_cell)  # (the cell moved)


@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_a_batch_is_bit_for_bit_its_systems_alone(device, fname):
    """Sizes (1, C + 1, 300) and a fourth system that starts at its minimum, atoms and cell.  Catches a chunk that straddles two
    systems, a merge over the wrong range of chunks, a record or a cell row of the wrong system and a converged system being moved."""
    parts = [R.site_system(n, seed=n) for n in (1, C + 1, 300)] + [minimum_system()]
    batch = driver(device, parts, DTYPES[fname])
    assert batch.num_systems == 4 and batch._n_chunks == 1 + 2 + 2 + 1
    for _ in range(25):
        batch.step()
    assert batch.nsteps.tolist() == [25, 25, 25, 0] and batch.converged.tolist() == [False, False, False, True]
    off = 0
    for s, part in enumerate(parts):
        n = len(part["k"])
        alone = driver(device, [part], DTYPES[fname])
        for _ in range(25):
            alone.step()
        for name in ("positions", "velocities", "_q"):
            assert torch.equal(getattr(alone, name), getattr(batch, name)[off:off + n]), f"{name} of system {s}"
        for name in ("dt", "a", "nsteps", "fmax", "converged", "_npos", "cell", "deform_grad", "cell_velocities", "stress"):
            assert torch.equal(getattr(alone, name)[0], getattr(batch, name)[s]), f"{name} of system {s}"
        off += n
    x_min, c_min = torch.from_numpy(parts[3]["x"]).to(device), torch.from_numpy(parts[3]["c0"]).to(device)
    assert torch.equal(batch.positions[off - 4:], x_min) and not batch.velocities[off - 4:].any()
    assert torch.equal(batch.cell[3], c_min) and torch.equal(batch.deform_grad[3].cpu(), torch.eye(3, dtype=torch.float64))
    R.assert_close(batch, _run(restatements(device, parts, DTYPES[fname]), 25), f"batch {fname} after 25 steps")


def test_seventy_small_systems_match_the_restatement(device):
    """More systems than a wavefront has lanes, one to five atoms each."""
    parts = [R.site_system(1 + s % 5, seed=1000 + s) for s in range(70)]
    drv = driver(device, parts, torch.float64)
    assert drv.num_systems == 70 and drv._n_chunks == 70
    refs = restatements(device, parts, torch.float64)
    drv.step()
    R.assert_close(drv, _run(refs, 1), "70 systems after 1 step")
    for _ in range(24):
        drv.step()
    R.assert_close(drv, _run(refs, 24), "70 systems after 25 steps")
    assert drv.nsteps.tolist() == [25] * 70


@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_cell_fire_with_a_frozen_cell_is_fire_bit_for_bit(device, fname):
    """The kernels of relax_cell.hip against those of relax.hip (the argument is that of the ATen form in test_cell_fire.py): with
    ``mask = 0`` only the decision both files call is left, over systems of 1, 40, 7 and 257 atoms (two rows to merge)."""
    cell_fire, fire, c0 = frozen_cell_pair(device, DTYPES[fname], "hip")
    assert cell_fire._hip and fire._hip and fire._n_chunks == cell_fire._n_chunks == 5
    assert_frozen_cell_is_fire(cell_fire, fire, c0)


def test_fixed_atoms_on_the_kernel_path(device):
    n = C + 5
    part = R.site_system(n, seed=n)
    fixed = np.zeros(n, dtype=bool)
    fixed[[0, 100, C - 1, C, n - 1]] = True
    part["x"][100] += np.array([2.0, 0.0, 0.0])  # the largest force of the system, on a fixed atom
    drv = driver(device, [part], torch.float64, fixed=fixed)
    free = driver(device, [part], torch.float64)
    (ref,) = restatements(device, [part], torch.float64, fixed=fixed)
    drv.step(), free.step(), ref.step()
    assert float(drv.fmax[0]) < 0.5 * float(free.fmax[0])
    for _ in range(24):
        drv.step()
    ref.run(24)
    R.assert_close(drv, [ref], "five fixed atoms after 25 steps")
    x, D = drv.positions.cpu().numpy(), drv.deform_grad[0].cpu().numpy()
    assert not drv.velocities.cpu().numpy()[fixed].any() and np.array_equal(drv._q.cpu().numpy()[fixed], part["x"][fixed])
    np.testing.assert_allclose(x[fixed], part["x"][fixed] @ D.T, rtol=1e-14)  # (a fixed atom follows the cell)
    assert not np.array_equal(x[fixed], part["x"][fixed])


@pytest.mark.parametrize("name", sorted(CONSTRAINTS))
def test_constraints_on_the_kernel_path(device, name):
    n = C + 5
    part = R.site_system(n, seed=n)
    options = CONSTRAINTS[name]
    drv = driver(device, [part], torch.float64, cell_factor=8.0, **options)
    free = driver(device, [part], torch.float64, cell_factor=8.0)
    (ref,) = restatements(device, [part], torch.float64, cell_factor=8.0, **options)
    for _ in range(25):
        drv.step()
        free.step()
    ref.run(25)
    R.assert_close(drv, [ref], f"{name} after 25 steps")
    D, D_free = drv.deform_grad[0].cpu().numpy(), free.deform_grad[0].cpu().numpy()
    assert float(np.abs(D - D_free).max()) > 1e-6, "the constraint changed nothing"
    if name == "hydrostatic_strain":
        assert D[0, 0] == D[1, 1] == D[2, 2] != 1.0 and not (D - np.diag(np.diag(D))).any()
    if name == "mask":
        assert np.array_equal(D[2], [0.0, 0.0, 1.0]) and not np.array_equal(D[0], [1.0, 0.0, 0.0])
    if name == "constant_volume":
        vD = drv.cell_velocities[0].cpu().numpy()
        assert abs(np.trace(vD)) <= 1e-12 * np.abs(vD).max()
    if name == "scalar_pressure":
        assert float(drv.volume[0]) < float(free.volume[0])


def test_convergence_in_the_steps_of_the_restatement(device):
    parts = [R.site_system(n, seed=n) for n in (7, 40)] + [minimum_system()]
    drv = driver(device, parts, torch.float64)
    refs = restatements(device, parts, torch.float64)
    want = [ref.relax(1e-3) for ref in refs]
    assert drv.run(fmax=1e-3, steps=2000, check_every=5) is True
    assert drv.nsteps.tolist() == want and want[2] == 0 and bool(drv.converged.all()) and float(drv.fmax.max()) < 1e-3
    R.assert_close(drv, refs, f"converged after {want} steps")


# ---- against themselves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_two_runs_give_the_same_bits_and_reading_changes_nothing(device, fname):
    parts = [R.site_system(n, seed=n) for n in (64 * C + 1, 300)] + [minimum_system()]
    a, b, c = (driver(device, parts, DTYPES[fname]) for _ in range(3))
    for _ in range(25):
        a.step()
        b.step()
        c.step()
        c.fmax.cpu(), c.converged.cpu(), c.velocities.cpu(), c.nsteps.cpu(), c.potential_energy.cpu()
        c.cell.cpu(), c.deform_grad.cpu(), c.cell_velocities.cpu(), c.stress.cpu(), c.volume.cpu()
    assert same_bits(a, b), "two runs of the same inputs differ"
    assert same_bits(a, c), "reading the accessors at every step changed the run"


def test_state_dict_round_trip_continues_bit_for_bit(device):
    parts = [R.site_system(n, seed=n) for n in (C + 1, 40)] + [minimum_system()]
    whole = driver(device, parts, torch.float32, fmax=1e-3, hydrostatic_strain=True)
    for _ in range(30):
        whole.step()
    first = driver(device, parts, torch.float32, fmax=1e-3, hydrostatic_strain=True)
    for _ in range(13):
        first.step()
    state = first.state_dict()
    second = driver(device, parts, torch.float32, fmax=0.7, dt=0.03, maxstep=0.01, nmin=1, constant_volume=True)
    for _ in range(4):
        second.step()
    second.load_state_dict(state)
    for _ in range(17):
        second.step()
    assert same_bits(second, whole) and torch.equal(second.stress, whole.stress)


def captured(drv, force):
    """The three launches and the analytic force step at the new positions and cell in one graph; forces and stress live in
    static buffers.  The caller keeps ``force`` alive as long as it replays: the graph reads what its closure holds."""
    static_forces, static_stress = drv.forces.clone(), drv.stress.clone()
    drv._forces, drv._stress = static_forces, static_stress
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        drv._launch()
        out = force(drv.positions, drv.cell)
        static_forces.copy_(out["forces"])
        static_stress.copy_(out["stress"])
    return graph, static_forces, static_stress


def test_captured_steps_are_eager_steps(device):
    parts = [R.site_system(n, seed=n) for n in (64 * C + 1, 300, 1)] + [minimum_system()]
    twin = driver(device, parts, torch.float64)
    for _ in range(25):  # (first, so that the kernels are loaded before anything is captured)
        twin.step()
    drv = driver(device, parts, torch.float64)
    before = state_of(drv)
    force = R.torch_force_step(parts, device, torch.float64)
    graph, static_forces, static_stress = captured(drv, force)
    after = state_of(drv)
    assert all(torch.equal(before[name], after[name]) for name in before)  # (capturing ran nothing)
    for _ in range(25):
        graph.replay()
    torch.cuda.synchronize()
    assert drv.nsteps.tolist() == [25, 25, 25, 0]
    assert same_bits(drv, twin) and torch.equal(static_forces, twin.forces) and torch.equal(static_stress, twin.stress)


def test_replays_after_convergence_change_nothing(device):
    parts = [R.site_system(n, seed=n) for n in (40, 7)] + [minimum_system()]
    refs = restatements(device, parts, torch.float64)
    want = [ref.relax(1e-3) for ref in refs]
    warm = driver(device, parts, torch.float64, fmax=1e-3)
    warm.step()
    drv = driver(device, parts, torch.float64, fmax=1e-3)
    force = R.torch_force_step(parts, device, torch.float64)
    graph, static_forces, static_stress = captured(drv, force)
    for _ in range(max(want) + 1):
        graph.replay()
    torch.cuda.synchronize()
    assert bool(drv.converged.all()) and drv.nsteps.tolist() == want
    R.assert_close(drv, refs, f"converged after {want} replayed steps")
    before, forces_before, stress_before = state_of(drv), static_forces.clone(), static_stress.clone()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    after = state_of(drv)
    assert all(torch.equal(before[name], after[name]) for name in before)
    assert torch.equal(forces_before, static_forces) and torch.equal(stress_before, static_stress)


def test_entry_refusals_launch_nothing(device):
    from nequip_amd import _lib as L

    lib = L.load()
    drv = driver(device, [R.site_system(5, seed=5), R.site_system(3, seed=3)], torch.float64)
    before = state_of(drv)
    stream = L.stream_ptr(device)
    f, v, x, q, ch, pa, cb, rec, sig, cell = (L.ptr(t) for t in (drv.forces, drv._vel, drv._pos, drv._q, drv._chunks, drv._partials,
                                                                  drv._chunk_begin, drv._rec, drv.stress, drv.cell))
    null = L.ptr(None)
    refused = lambda rc, word: rc != 0 and word in lib.nqa_last_error()  # noqa: E731
    F64 = L.NQA_F64
    assert refused(lib.nqa_cellfire_reduce(F64, null, v, null, ch, 2, rec, pa, stream), b"forces")
    assert refused(lib.nqa_cellfire_reduce(F64, f, null, null, ch, 2, rec, pa, stream), b"velocities")
    assert refused(lib.nqa_cellfire_reduce(F64, f, v, null, null, 2, rec, pa, stream), b"chunks")
    assert refused(lib.nqa_cellfire_reduce(F64, f, v, null, ch, 2, null, pa, stream), b"systems")
    assert refused(lib.nqa_cellfire_reduce(F64, f, v, null, ch, 2, rec, null, stream), b"partials")
    assert refused(lib.nqa_cellfire_reduce(F64, f, v, null, ch, 0, rec, pa, stream), b"n_chunks")
    assert refused(lib.nqa_cellfire_reduce(7, f, v, null, ch, 2, rec, pa, stream), b"float32 or float64")
    assert refused(lib.nqa_cellfire_decide(null, cb, F64, sig, rec, cell, 2, stream), b"partials")
    assert refused(lib.nqa_cellfire_decide(pa, null, F64, sig, rec, cell, 2, stream), b"chunk_begin")
    assert refused(lib.nqa_cellfire_decide(pa, cb, F64, null, rec, cell, 2, stream), b"stress")
    assert refused(lib.nqa_cellfire_decide(pa, cb, F64, sig, null, cell, 2, stream), b"systems")
    assert refused(lib.nqa_cellfire_decide(pa, cb, F64, sig, rec, null, 2, stream), b"cell")
    assert refused(lib.nqa_cellfire_decide(pa, cb, F64, sig, rec, cell, 0, stream), b"n_systems")
    assert refused(lib.nqa_cellfire_decide(pa, cb, F64, sig, rec, cell, -3, stream), b"n_systems")
    assert refused(lib.nqa_cellfire_decide(pa, cb, 9, sig, rec, cell, 2, stream), b"float32 or float64")
    assert refused(lib.nqa_cellfire_move(F64, null, x, q, v, null, ch, 2, rec, stream), b"forces")
    assert refused(lib.nqa_cellfire_move(F64, f, null, q, v, null, ch, 2, rec, stream), b"positions")
    assert refused(lib.nqa_cellfire_move(F64, f, x, null, v, null, ch, 2, rec, stream), b"coords")
    assert refused(lib.nqa_cellfire_move(F64, f, x, q, null, null, ch, 2, rec, stream), b"velocities")
    assert refused(lib.nqa_cellfire_move(F64, f, x, q, v, null, null, 2, rec, stream), b"chunks")
    assert refused(lib.nqa_cellfire_move(F64, f, x, q, v, null, ch, 2, null, stream), b"systems")
    assert refused(lib.nqa_cellfire_move(F64, f, x, q, v, null, ch, 0, rec, stream), b"n_chunks")
    assert refused(lib.nqa_cellfire_move(-1, f, x, q, v, null, ch, 2, rec, stream), b"float32 or float64")
    torch.cuda.synchronize()
    after = state_of(drv)
    assert all(torch.equal(before[name], after[name]) for name in before)  # (nothing ran)


# ---- with a model ----------------------------------------------------------------------------------------------------------------
PRESSURE = 0.005  # eV / A^3


def analytic_bound(n_max, n_min, xmax, steps=10):
    """``(x_atol, D_atol)`` of cell_fire_restatement.py for the largest and the smallest system of a batch (maxstep 0.2, |D| <= 1.5)."""
    m, scale = 3 * (n_max + 3), R.AMP * steps * R.EPS
    d_atol = scale * ((m + R.CELL_OPS) * 0.2 / n_min + 3.0 * R.R_NORM)
    return scale * (m * 0.2 + (1.0 + 3.0 * R.R_NORM ** 2) * xmax) + 3.0 * R.R_NORM * xmax * d_atol, d_atol


@functools.lru_cache(maxsize=None)
def water(device):
    """Three perturbed periodic water boxes (24, 81 and 24 atoms), cells strained by 3 %, the small model of test_fire_gpu.py and
    its torch-sim calculator."""
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn

    rng = np.random.default_rng(7)
    boxes = []
    for seed, n_side in ((0, 2), (1, 3), (2, 2)):
        p, types, cell, names = syn.water_box(n_side, seed=seed)
        strain = rng.uniform(-1.0, 1.0, size=(3, 3))
        strain = np.eye(3) + 0.03 * 0.5 * (strain + strain.T)
        boxes.append(dict(x=(p + 0.05 * rng.normal(size=p.shape)) @ strain, cell=cell @ strain, types=types, names=names))
    model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=2, l_max=1, parity=False,
                           num_features=8, radial_mlp_width=64, radial_mlp_depth=1, avg_num_neighbors=20.0).to(device).eval()
    return boxes, model, NequIPTorchSimCalc(model, device=device)


def torchsim_run(device, boxes, calc, backend, steps=10):
    z_of = {"H": 1, "O": 8}
    t = lambda a, dtype: torch.tensor(np.asarray(a), dtype=dtype, device=device)  # noqa: E731
    numbers = [z_of[b["names"][k]] for b in boxes for k in b["types"]]
    sidx = np.repeat(np.arange(len(boxes)), [len(b["x"]) for b in boxes])
    drv = CellFIRE.from_torchsim(calc, t(np.concatenate([b["x"] for b in boxes]), torch.float64),
                                 t(np.stack([b["cell"] for b in boxes]), torch.float64), True, t(numbers, torch.long),
                                 t(sidx, torch.long), scalar_pressure=PRESSURE, backend=backend)
    drv._set_target(TIGHT)
    start = (drv.potential_energy.double() + PRESSURE * drv.volume).clone()
    for _ in range(steps):
        drv.step()
    assert drv.nsteps.tolist() == [steps] * len(boxes) and torch.isfinite(drv.positions).all() and torch.isfinite(drv.cell).all()
    assert drv.potential_energy.shape == (len(boxes),) and drv.stress.shape == (len(boxes), 3, 3)
    return drv, start, drv.potential_energy.double() + PRESSURE * drv.volume


def test_batched_cell_relaxation_of_water_boxes_through_the_torchsim_calculator(device):
    """Three perturbed periodic water boxes (24, 81 and 24 atoms, cells strained by 3 %), 10 steps through
    ``CellFIRE.from_torchsim``: the kernels against the ATen form around the same calculator.  The tolerance is the rule of
    test_fire_gpu.py: ten times the largest difference between two ATen runs (the force path's own scatter), or, if that is
    exactly zero, the analytic bound of cell_fire_restatement.py.  The enthalpy E + p V of no system ends above where it started.

    Measured on an MI355X: the two ATen runs agree bit for bit (scatter 0.0 in positions and cell), so the analytic bounds
    apply, 3.6e-12 Angstrom for the positions and 1.7e-12 for the cell; the kernels differ from the ATen form by 8.9e-16 Angstrom
    in the positions and by 0.0 in the cell; the largest change of a cell component over the 10 steps is 1.4e-2 Angstrom; the
    enthalpies go from (2.443, 8.311, 2.311) to (0.778, 3.165, 0.648) eV."""
    boxes, _, calc = water(device)
    (aten_a, _, _), (aten_b, _, _) = torchsim_run(device, boxes, calc, "aten"), torchsim_run(device, boxes, calc, "aten")
    hip, start, end = torchsim_run(device, boxes, calc, "hip")
    assert hip._hip and not aten_a._hip and calc.compute_stress
    scatter_x = float((aten_a.positions - aten_b.positions).abs().max())
    scatter_c = float((aten_a.cell - aten_b.cell).abs().max())
    xmax, cmax = float(hip.positions.abs().max()), float(hip.reference_cell.abs().max())
    x_atol, d_atol = analytic_bound(81, 24, xmax)
    tol_x = 10.0 * scatter_x if scatter_x > 0.0 else x_atol
    tol_c = 10.0 * scatter_c if scatter_c > 0.0 else 3.0 * cmax * d_atol
    diff_x = float((hip.positions - aten_a.positions).abs().max())
    diff_c = float((hip.cell - aten_a.cell).abs().max())
    moved = float((hip.cell - hip.reference_cell).abs().max())
    print(f"scatter of two ATen runs: x {scatter_x:.3e} A, cell {scatter_c:.3e} A; kernels against ATen: x {diff_x:.3e} A "
          f"(tolerance {tol_x:.3e}), cell {diff_c:.3e} A (tolerance {tol_c:.3e}); largest change of a cell component {moved:.3e} A; "
          f"enthalpy {start.tolist()} -> {end.tolist()} eV")
    assert moved > 0.0
    assert diff_x <= tol_x and diff_c <= tol_c
    assert torch.equal(hip.dt, aten_a.dt) and torch.equal(hip.nsteps, aten_a.nsteps)
    assert bool((end <= start).all()), "the enthalpy of a system ended above where it started"


def test_cell_relaxation_around_a_graphed_step(device):
    """The 24-atom box around a ``GraphedStep`` with energy, forces and stress for 10 steps: the cell the step used is
    ``drv.cell`` (device-to-device, ``set_cell_from_device``), no step fell back to the eager path, and positions and cell agree
    with the torch-sim route of the same box at the rule of the test above.

    Measured on an MI355X: the two ATen torch-sim runs agree bit for bit, so the analytic bounds apply (1.8e-12 Angstrom for
    the positions, 9.1e-13 for the cell); the two routes differ by 0.0 in both."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.integrations.graphed_step import GraphedStep

    boxes, model, calc = water(device)
    box = boxes[0]
    (ts_a, _, _), (ts_b, _, _) = torchsim_run(device, [box], calc, "aten"), torchsim_run(device, [box], calc, "aten")
    ts, _, _ = torchsim_run(device, [box], calc, "hip")
    t = lambda a, dtype: torch.tensor(np.asarray(a), dtype=dtype, device=device)  # noqa: E731
    step = GraphedStep(model, t(box["types"], torch.long), t(box["cell"], torch.float64), True, 4.5,
                       outputs=(K.TOTAL_ENERGY_KEY, K.FORCE_KEY, K.STRESS_KEY))
    drv = CellFIRE(step, t(box["x"], torch.float64), t(box["cell"], torch.float64), scalar_pressure=PRESSURE)
    drv._set_target(TIGHT)
    for _ in range(10):
        drv.step()
    assert drv._hip and drv.nsteps.tolist() == [10] and step.num_eager_fallbacks == 0
    assert torch.equal(step._cell[0], drv.cell[0]) and torch.equal(step._nl.cell64, drv.cell[0])
    assert not torch.equal(drv.cell, drv.reference_cell)
    scatter_x = float((ts_a.positions - ts_b.positions).abs().max())
    scatter_c = float((ts_a.cell - ts_b.cell).abs().max())
    xmax, cmax = float(drv.positions.abs().max()), float(drv.reference_cell.abs().max())
    x_atol, d_atol = analytic_bound(24, 24, xmax)
    tol_x = 10.0 * scatter_x if scatter_x > 0.0 else x_atol
    tol_c = 10.0 * scatter_c if scatter_c > 0.0 else 3.0 * cmax * d_atol
    diff_x = float((drv.positions - ts.positions).abs().max())
    diff_c = float((drv.cell - ts.cell).abs().max())
    print(f"scatter of two ATen torch-sim runs: x {scatter_x:.3e} A, cell {scatter_c:.3e} A; GraphedStep route against torch-sim "
          f"route: x {diff_x:.3e} A (tolerance {tol_x:.3e}), cell {diff_c:.3e} A (tolerance {tol_c:.3e})")
    assert diff_x <= tol_x and diff_c <= tol_c
