"""The FIRE kernels (csrc/relax.hip: nqa_fire_reduce + nqa_fire_decide + nqa_fire_move) under the driver of
nequip_amd/integrations/relax.py, against the float64 restatement of tests/fire_restatement.py at the bounds its docstring
derives, and bit for bit against themselves.

Sizes: with C = nqa_fire_chunk_atoms() atoms per chunk, 1, C - 1, C, C + 1 and 64 C + 1 atoms are a fraction of one chunk, one
atom short of a chunk, a full chunk, the first atom of a second chunk, and 65 chunks, i.e. more rows of partial sums than the 64
lanes of the decide wavefront take one each.  Forces come from one analytic function evaluated in torch on the device
(restatement included, so that a float32 force is the same number on both sides): only the optimizer is under test."""
import copy
import functools

import numpy as np
import pytest
import torch

import fire_restatement as R
from nequip_amd.integrations import FIRE

pytestmark = pytest.mark.gpu

C = 256
SIZES = (1, C - 1, C, C + 1, 64 * C + 1)
DTYPES = {"f32": torch.float32, "f64": torch.float64}
TIGHT = 1e-8  # a target no case here reaches in 25 steps


def test_chunk_constant(device):
    from nequip_amd import _lib

    assert _lib.load().nqa_fire_chunk_atoms() == C


def minimum_system():
    k, x0, _ = R.wells(4, seed=99)
    return k, x0, x0.copy()


def concatenated(parts):
    k, x0, x = (np.concatenate([p[i] for p in parts]) for i in range(3))
    sidx = np.repeat(np.arange(len(parts)), [len(p[0]) for p in parts])
    return k, x0, x, sidx


def driver(device, parts, fdtype, backend="hip", fmax=TIGHT, **params):
    k, x0, x, sidx = concatenated(parts)
    drv = FIRE(R.torch_force_step(k, x0, device, fdtype), torch.from_numpy(x).to(device),
               system_idx=torch.from_numpy(sidx).to(device) if len(parts) > 1 else None, backend=backend, **params)
    drv._set_target(fmax)
    return drv


def restatements(device, parts, fdtype, fmax=TIGHT):
    return [R.Restated(R.restated_force(k, x0, device, fdtype), x, fmax_target=fmax) for k, x0, x in parts]


@functools.lru_cache(maxsize=None)
def reference(device, n, fname):
    """The restatement of the single system of ``n`` atoms after 1 and after 25 steps (computed once, never modified)."""
    (ref,) = restatements(device, [R.wells(n, seed=n)], DTYPES[fname])
    ref.run(1)
    one = copy.copy(ref)
    ref.run(24)
    return one, ref


def state_of(drv):
    """Every buffer of the driver, cloned."""
    return {"positions": drv.positions.clone(), "velocities": drv.velocities.clone(), "record": drv._rec.view(torch.int64).clone(),
            "partials": drv._partials.clone()}


def same_bits(a, b):
    sa, sb = state_of(a), state_of(b)
    return all(torch.equal(sa[name], sb[name]) for name in sa)


# ---- against the restatement -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
@pytest.mark.parametrize("n", SIZES)
def test_single_system_matches_the_restatement(device, n, fname):
    one, last = reference(device, n, fname)
    drv = driver(device, [R.wells(n, seed=n)], DTYPES[fname])
    assert drv._hip and drv.forces.dtype == DTYPES[fname] and drv._n_chunks == (n + C - 1) // C
    drv.step()
    R.assert_close(drv, [one], f"N={n} {fname} after 1 step")
    for _ in range(24):
        drv.step()
    R.assert_close(drv, [last], f"N={n} {fname} after 25 steps")
    assert last.nsteps == 25 and min(last.margins.values()) >= R.MARGIN


@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_a_batch_is_bit_for_bit_its_systems_alone(device, fname):
    """Sizes (1, C + 1, 300) and a fourth system that starts at its minimum.  Catches a chunk that straddles two systems, a merge
    over the wrong range of chunks and a converged system being moved."""
    parts = [R.wells(n, seed=n) for n in (1, C + 1, 300)] + [minimum_system()]
    batch = driver(device, parts, DTYPES[fname])
    assert batch.num_systems == 4 and batch._n_chunks == 1 + 2 + 2 + 1
    for _ in range(25):
        batch.step()
    assert batch.nsteps.tolist() == [25, 25, 25, 0] and batch.converged.tolist() == [False, False, False, True]
    off = 0
    for s, part in enumerate(parts):
        n = len(part[0])
        alone = driver(device, [part], DTYPES[fname])
        for _ in range(25):
            alone.step()
        for name in ("positions", "velocities"):
            assert torch.equal(getattr(alone, name), getattr(batch, name)[off:off + n]), f"{name} of system {s}"
        for name in ("dt", "a", "nsteps", "fmax", "converged", "_npos"):
            assert torch.equal(getattr(alone, name)[0], getattr(batch, name)[s]), f"{name} of system {s}"
        off += n
    x_min = torch.from_numpy(parts[3][2]).to(device)
    assert torch.equal(batch.positions[off - 4:], x_min) and not batch.velocities[off - 4:].any()
    R.assert_close(batch, [r for r in _run(restatements(device, parts, DTYPES[fname]), 25)], f"batch {fname} after 25 steps")


def _run(refs, n):
    for ref in refs:
        ref.run(n)
    return refs


def test_seventy_small_systems_match_the_restatement(device):
    """More systems than a wavefront has lanes, one to five atoms each."""
    parts = [R.wells(1 + s % 5, seed=1000 + s) for s in range(70)]
    drv = driver(device, parts, torch.float64)
    assert drv.num_systems == 70 and drv._n_chunks == 70
    refs = restatements(device, parts, torch.float64)
    drv.step()
    R.assert_close(drv, _run(refs, 1), "70 systems after 1 step")
    for _ in range(24):
        drv.step()
    R.assert_close(drv, _run(refs, 24), "70 systems after 25 steps")
    assert drv.nsteps.tolist() == [25] * 70


def test_convergence_in_the_steps_of_the_restatement(device):
    parts = [R.wells(n, seed=n) for n in (7, 40)] + [minimum_system()]
    drv = driver(device, parts, torch.float64)
    refs = restatements(device, parts, torch.float64)
    want = [ref.relax(1e-3) for ref in refs]
    assert drv.run(fmax=1e-3, steps=2000, check_every=5) is True
    assert drv.nsteps.tolist() == want and want[2] == 0 and bool(drv.converged.all()) and float(drv.fmax.max()) < 1e-3
    R.assert_close(drv, refs, f"converged after {want} steps")


# ---- against themselves ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_two_runs_give_the_same_bits_and_reading_changes_nothing(device, fname):
    parts = [R.wells(n, seed=n) for n in (64 * C + 1, 300)] + [minimum_system()]
    a, b, c = (driver(device, parts, DTYPES[fname]) for _ in range(3))
    for _ in range(25):
        a.step()
        b.step()
        c.step()
        c.fmax.cpu(), c.converged.cpu(), c.velocities.cpu(), c.nsteps.cpu(), c.potential_energy.cpu()
    assert same_bits(a, b), "two runs of the same inputs differ"
    assert same_bits(a, c), "reading fmax / converged / velocities at every step changed the run"


def test_state_dict_round_trip_continues_bit_for_bit(device):
    parts = [R.wells(n, seed=n) for n in (C + 1, 40)] + [minimum_system()]
    whole = driver(device, parts, torch.float32, fmax=1e-3)
    for _ in range(30):
        whole.step()
    first = driver(device, parts, torch.float32, fmax=1e-3)
    for _ in range(13):
        first.step()
    state = first.state_dict()
    second = driver(device, parts, torch.float32, fmax=0.7, dt=0.03, maxstep=0.01, nmin=1)
    for _ in range(4):
        second.step()
    second.load_state_dict(state)
    for _ in range(17):
        second.step()
    assert same_bits(second, whole)


def captured(drv, force):
    """The three launches and the analytic force at the new positions in one graph; the forces live in a static buffer.
    The caller keeps ``force`` alive as long as it replays: the graph reads the wells its closure holds."""
    static_forces = drv.forces.clone()
    drv._forces = static_forces
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        drv._launch()
        static_forces.copy_(force(drv.positions)["forces"])
    return graph, static_forces


def test_captured_steps_are_eager_steps(device):
    parts = [R.wells(n, seed=n) for n in (64 * C + 1, 300, 1)] + [minimum_system()]
    k, x0, _, _ = concatenated(parts)
    twin = driver(device, parts, torch.float64)
    for _ in range(25):  # (first, so that the kernels are loaded before anything is captured)
        twin.step()
    drv = driver(device, parts, torch.float64)
    before = state_of(drv)
    force = R.torch_force_step(k, x0, device, torch.float64)
    graph, static_forces = captured(drv, force)
    after = state_of(drv)
    assert all(torch.equal(before[name], after[name]) for name in before)  # (capturing ran nothing)
    for _ in range(25):
        graph.replay()
    torch.cuda.synchronize()
    assert drv.nsteps.tolist() == [25, 25, 25, 0]
    assert same_bits(drv, twin) and torch.equal(static_forces, twin.forces)


def test_replays_after_convergence_change_nothing(device):
    parts = [R.wells(n, seed=n) for n in (40, 7, 1)] + [minimum_system()]
    k, x0, _, _ = concatenated(parts)
    refs = restatements(device, parts, torch.float64)
    want = [ref.relax(1e-3) for ref in refs]
    warm = driver(device, parts, torch.float64, fmax=1e-3)
    warm.step()
    drv = driver(device, parts, torch.float64, fmax=1e-3)
    force = R.torch_force_step(k, x0, device, torch.float64)
    graph, static_forces = captured(drv, force)
    for _ in range(max(want) + 1):
        graph.replay()
    torch.cuda.synchronize()
    assert bool(drv.converged.all()) and drv.nsteps.tolist() == want
    R.assert_close(drv, refs, f"converged after {want} replayed steps")
    before, forces_before = state_of(drv), static_forces.clone()
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()
    after = state_of(drv)
    assert all(torch.equal(before[name], after[name]) for name in before) and torch.equal(forces_before, static_forces)


def test_entry_refusals_launch_nothing(device):
    from nequip_amd import _lib as L

    lib = L.load()
    drv = driver(device, [R.wells(5, seed=5), R.wells(3, seed=3)], torch.float64)
    before = state_of(drv)
    stream = L.stream_ptr(device)
    f, v, x, ch, pa, cb, rec = (L.ptr(t) for t in (drv.forces, drv._vel, drv._pos, drv._chunks, drv._partials, drv._chunk_begin,
                                                  drv._rec))
    null = L.ptr(None)
    refused = lambda rc, word: rc != 0 and word in lib.nqa_last_error()  # noqa: E731
    assert refused(lib.nqa_fire_reduce(L.NQA_F64, null, v, null, ch, 2, pa, stream), b"forces")
    assert refused(lib.nqa_fire_reduce(L.NQA_F64, f, null, null, ch, 2, pa, stream), b"velocities")
    assert refused(lib.nqa_fire_reduce(L.NQA_F64, f, v, null, null, 2, pa, stream), b"chunks")
    assert refused(lib.nqa_fire_reduce(L.NQA_F64, f, v, null, ch, 2, null, stream), b"partials")
    assert refused(lib.nqa_fire_reduce(L.NQA_F64, f, v, null, ch, 0, pa, stream), b"n_chunks")
    assert refused(lib.nqa_fire_reduce(7, f, v, null, ch, 2, pa, stream), b"float32 or float64")
    assert refused(lib.nqa_fire_decide(null, cb, rec, 2, stream), b"partials")
    assert refused(lib.nqa_fire_decide(pa, null, rec, 2, stream), b"chunk_begin")
    assert refused(lib.nqa_fire_decide(pa, cb, null, 2, stream), b"systems")
    assert refused(lib.nqa_fire_decide(pa, cb, rec, 0, stream), b"n_systems")
    assert refused(lib.nqa_fire_decide(pa, cb, rec, -3, stream), b"n_systems")
    assert refused(lib.nqa_fire_move(L.NQA_F64, null, x, v, null, ch, 2, rec, stream), b"forces")
    assert refused(lib.nqa_fire_move(L.NQA_F64, f, null, v, null, ch, 2, rec, stream), b"positions")
    assert refused(lib.nqa_fire_move(L.NQA_F64, f, x, null, null, ch, 2, rec, stream), b"velocities")
    assert refused(lib.nqa_fire_move(L.NQA_F64, f, x, v, null, null, 2, rec, stream), b"chunks")
    assert refused(lib.nqa_fire_move(L.NQA_F64, f, x, v, null, ch, 2, null, stream), b"systems")
    assert refused(lib.nqa_fire_move(L.NQA_F64, f, x, v, null, ch, 0, rec, stream), b"n_chunks")
    assert refused(lib.nqa_fire_move(-1, f, x, v, null, ch, 2, rec, stream), b"float32 or float64")
    torch.cuda.synchronize()
    after = state_of(drv)
    assert all(torch.equal(before[name], after[name]) for name in before)  # (nothing ran)


def test_fixed_atoms_on_the_kernel_path(device):
    n = C + 5
    k, x0, x = R.wells(n, seed=n)
    fixed = np.zeros(n, dtype=bool)
    fixed[[0, 100, C - 1, C, n - 1]] = True
    x[100] = x0[100] + np.array([3.0, 0.0, 0.0])  # the largest force of the system, on a fixed atom
    drv = FIRE(R.torch_force_step(k, x0, device), torch.from_numpy(x).to(device), fixed=torch.from_numpy(fixed).to(device))
    drv._set_target(TIGHT)
    ref = R.Restated(R.restated_force(k, x0, device), x, fixed=fixed, fmax_target=TIGHT)
    for _ in range(25):
        drv.step()
    ref.run(25)
    R.assert_close(drv, [ref], "five fixed atoms after 25 steps")
    assert np.array_equal(drv.positions.cpu().numpy()[fixed], x[fixed]) and not drv.velocities.cpu().numpy()[fixed].any()


# ---- with a model ----------------------------------------------------------------------------------------------------------------
def test_batched_relaxation_of_water_boxes_through_the_torchsim_calculator(device):
    """Three perturbed periodic water boxes (24, 81 and 24 atoms), 10 steps through ``FIRE.from_torchsim`` with the model of
    tests/test_torchsim.py: the kernels against the ATen form around the same calculator.  The model's forces are not
    reproducible to the bit (atomic accumulation), so the tolerance is measured, not fixed: the largest position difference
    between two ATen runs is the force path's own scatter, and the kernels may differ from the ATen form by ten times that, or,
    if it is exactly zero, by the bound of the analytic case.

    Measured on an MI355X: the two ATen runs agree bit for bit (scatter 0.0: at this size the force path happens to be
    reproducible), so the analytic bound applies, 5.1e-13 Angstrom; the kernels differ from the ATen form by 0.0 Angstrom; the
    largest displacement of an atom over the 10 steps is 0.29 Angstrom."""
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn

    z_of = {"H": 1, "O": 8}
    rng = np.random.default_rng(7)
    pos, numbers, cells, sidx = [], [], [], []
    for s, (seed, n_side) in enumerate(((0, 2), (1, 3), (2, 2))):
        p, types, cell, names = syn.water_box(n_side, seed=seed)
        pos.append(p + 0.05 * rng.normal(size=p.shape))
        numbers += [z_of[names[t]] for t in types]
        cells.append(cell)
        sidx += [s] * len(p)
    model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=2, l_max=1, parity=False,
                           num_features=8, radial_mlp_width=64, radial_mlp_depth=1, avg_num_neighbors=20.0).to(device).eval()
    calc = NequIPTorchSimCalc(model, device=device)
    t = lambda a, dtype: torch.tensor(np.asarray(a), dtype=dtype, device=device)  # noqa: E731
    args = (t(np.concatenate(pos), torch.float64), t(np.stack(cells), torch.float64), True, t(numbers, torch.long), t(sidx, torch.long))

    def relaxed(backend):
        drv = FIRE.from_torchsim(calc, *args, backend=backend)
        drv._set_target(TIGHT)
        for _ in range(10):
            drv.step()
        assert drv.nsteps.tolist() == [10, 10, 10] and torch.isfinite(drv.positions).all()
        assert drv.potential_energy.shape == (3,)
        return drv

    aten_a, aten_b, hip = relaxed("aten"), relaxed("aten"), relaxed("hip")
    assert hip._hip and not aten_a._hip
    scatter = float((aten_a.positions - aten_b.positions).abs().max())
    n_max = 81
    analytic = R.AMP * 10 * R.EPS * (3 * n_max * 0.2 + float(hip.positions.abs().max()))
    tolerance = 10.0 * scatter if scatter > 0.0 else analytic
    difference = float((hip.positions - aten_a.positions).abs().max())
    moved = float((hip.positions - args[0]).abs().max())
    print(f"scatter of two ATen runs {scatter:.3e} A, kernels against ATen {difference:.3e} A, tolerance {tolerance:.3e} A; "
          f"largest displacement in 10 steps {moved:.3e} A")
    assert moved > 0.0
    assert difference <= tolerance
    assert torch.equal(hip.dt, aten_a.dt) and torch.equal(hip.nsteps, aten_a.nsteps)
