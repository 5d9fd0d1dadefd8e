"""The batched Langevin kernels (csrc/md_batched.hip) under BatchedLangevin and BatchedLangevinNPT
(nequip_amd/integrations/md_batched.py).  The main check needs no tolerance: system ``s`` of a batch has, bit for bit, the
positions, stored and completed velocities, kinetic energy and (NPT) cell, mu, pressure and volume that the single-system kernels
(Langevin / LangevinNPT, pinned to their float64 restatements by tests/test_langevin_gpu.py and tests/test_langevin_npt_gpu.py)
give for it alone with the same seed and the same forces, at every step.

Sizes (tests/batched_md_cases.py): 1, 85, 86, 1, 171 and 5462 atoms in one batch are a fraction of a chunk, one component short of
a chunk, a second chunk that begins inside an atom, three chunks and 65 chunks (the bath lanes add runs of two rows); 70 systems
of 1 to 3 atoms are more systems than a wavefront has lanes, every chunk nearly empty.  Forces (and stresses) are analytic and
element-wise, so that a system alone and in a batch is handed the same bits: only the integrator is under test."""
import numpy as np
import pytest
import torch

import batched_md_cases as B
import langevin_restatement as LR
import npt_restatement as NR
from nequip_amd.integrations import BatchedLangevin, BatchedLangevinNPT
from nequip_amd.integrations import md as M

pytestmark = pytest.mark.gpu

DTYPES = B.DTYPES


def snapshot(drv):
    """What a batch holds after a step, read once: positions, stored and completed velocities, kinetic energies, step counts and,
    under NPT, cells, mu, pressures and volumes."""
    snap = dict(x=drv.positions.clone(), stored=drv._vel.clone(), v=drv.velocities.clone(), k=drv.kinetic_energy.clone(),
                temperature=drv.temperature.clone(), nsteps=drv.nsteps.clone())
    if drv._hip:
        snap["bath_k"] = drv._rec[:, M._EKIN].clone()
    if isinstance(drv, BatchedLangevinNPT):
        snap.update(cell=drv.cell.clone(), mu=drv.scaling, pressure=drv.pressure, volume=drv.volume)
        if drv._hip:
            snap.update(npt_k=drv._npt[:, M._NPT_EKIN].clone(), npt_volume=drv._npt[:, M._NPT_VOLUME].clone())
    return snap


def same_snapshots(a, b):
    return all(torch.equal(a[name], b[name]) for name in a)


def assert_system_is_the_single_run(snap, s, lo, hi, one, what):
    assert torch.equal(snap["x"][lo:hi], one.positions), f"{what}: positions"
    assert torch.equal(snap["stored"][lo:hi], one._vel), f"{what}: stored velocities"
    assert torch.equal(snap["v"][lo:hi], one.velocities), f"{what}: completed velocities"
    assert float(snap["k"][s]) == one.kinetic_energy, f"{what}: kinetic energy"
    assert float(snap["temperature"][s]) == one.temperature, f"{what}: temperature"
    assert float(snap["bath_k"][s]) == float(one._rec[M._EKIN]), f"{what}: the kinetic energy of the bath launch"
    assert int(snap["nsteps"][s]) == one.nsteps, f"{what}: step count"
    if "cell" in snap:
        assert torch.equal(snap["cell"][s:s + 1], one.cell), f"{what}: cell"
        assert float(snap["mu"][s]) == float(one._npt[M._NPT_MU]), f"{what}: mu"
        assert float(snap["pressure"][s]) == one.pressure, f"{what}: pressure"
        assert float(snap["volume"][s]) == one.volume, f"{what}: volume"
        assert float(snap["npt_k"][s]) == float(one._npt[M._NPT_EKIN]) and float(snap["npt_volume"][s]) == float(
            one._npt[M._NPT_VOLUME]), f"{what}: the record of the barostat"


# 1, 2 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
@pytest.mark.parametrize("ensemble", ("nvt", "npt"))
def test_every_system_of_a_batch_takes_the_steps_it_takes_alone_bit_for_bit(device, ensemble, fname):
    systems, dtype = B.batch(B.COUNTS), DTYPES[fname]
    make, alone_of = (B.batched_nvt, B.single_nvt) if ensemble == "nvt" else (B.batched_npt, B.single_npt)
    drv = make(systems, device, dtype)
    alone = [alone_of(q, device, dtype) for q in systems]
    assert drv._hip and all(one._hip for one in alone) and drv.forces.dtype == dtype
    assert drv._n_chunks == 1 + 1 + 2 + 1 + 3 + 65 and drv._chunk_begin.tolist() == [0, 1, 2, 4, 5, 8, 73]
    b = B.offsets(systems)
    cell0 = drv.cell.clone() if ensemble == "npt" else None
    for step in range(11):  # (step 0: the state of the constructor)
        if step:
            drv.step()
        snap = snapshot(drv)
        for s, one in enumerate(alone):
            if step:
                one.step()
            assert_system_is_the_single_run(snap, s, int(b[s]), int(b[s + 1]), one,
                                            f"{ensemble} {fname}, system {s} ({systems[s]['n']} atoms), step {step}")
    assert drv.nsteps.tolist() == [10] * len(systems) and drv.potential_energy.shape == (len(systems),)
    if ensemble == "npt":
        assert all(not torch.equal(drv.cell[s], cell0[s]) for s in range(len(systems)))  # (every barostat acted)


# 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_zero_compressibility_gives_the_bits_of_the_nvt_batch(device):
    systems = B.batch(B.COUNTS)
    kept = systems[2]["compressibility"]
    npt = B.batched_npt(systems, device, torch.float32, compressibility=[0.0, 0.0, kept, 0.0, 0.0, 0.0])
    cells = npt.cell.clone()
    inner = npt.force_step
    x = torch.from_numpy(np.concatenate([q["part"]["x"] for q in systems])).to(device)
    nvt = BatchedLangevin(lambda pos: inner(pos, cells), npt.masses, npt.timestep, npt.target_temperature, npt.friction, x,
                          npt.system_idx, B._cat(systems, "v", device), seed=npt.seeds)
    assert npt._hip and nvt._hip
    npt.run(10), nvt.run(10)
    a, c = snapshot(npt), snapshot(nvt)
    b = B.offsets(systems)
    for s in (0, 1, 3, 4, 5):
        lo, hi = int(b[s]), int(b[s + 1])
        assert all(torch.equal(a[name][lo:hi], c[name][lo:hi]) for name in ("x", "stored", "v")), f"system {s}"
        assert all(torch.equal(a[name][s], c[name][s]) for name in ("k", "bath_k", "nsteps")), f"system {s}"
        assert torch.equal(a["cell"][s], cells[s]) and float(a["mu"][s]) == 1.0
    lo, hi = int(b[2]), int(b[3])
    assert not torch.equal(a["cell"][2], cells[2]) and not torch.equal(a["x"][lo:hi], c["x"][lo:hi])


# 4 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", sorted(DTYPES))
def test_seventy_tiny_systems_match_the_restatement(device, fname):
    counts = tuple(1 + s % 3 for s in range(70))
    systems, dtype = B.batch(counts, salt=1), DTYPES[fname]
    drv = B.batched_nvt(systems, device, dtype)
    assert drv._hip and drv.num_systems == 70 and drv._n_chunks == 70
    refs = [B.restated_nvt(q, device, dtype) for q in systems]
    drv.run(5)
    for s, ref in enumerate(refs):
        ref.run(5)
        LR.assert_close(B.View(drv, s), ref, f"system {s} of 70 ({systems[s]['n']} atoms) {fname}", systems[s]["temperature"])
    npt = B.batched_npt(systems, device, dtype)
    refs = [B.restated_npt(q, device, dtype) for q in systems]
    npt.run(5)
    for s, ref in enumerate(refs):
        ref.run(5)
        NR.assert_close(B.View(npt, s), ref, f"NPT, system {s} of 70 ({systems[s]['n']} atoms) {fname}", systems[s]["temperature"],
                        systems[s]["part"])


# 5 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ("nvt", "npt"))
def test_the_place_in_the_batch_leaves_a_trajectory_unchanged(device, ensemble):
    """The 171-atom system behind a first system of 1 atom and behind one of 86 atoms (its first component at global index 3 and
    258: in another lane, and in the second case preceded by two chunks): the noise is drawn for the local index, so the two
    trajectories are the same bits."""
    systems = B.batch(B.COUNTS)
    make = B.batched_nvt if ensemble == "nvt" else B.batched_npt
    a, b = make((systems[0], systems[4]), device), make((systems[2], systems[4]), device)
    a.run(10), b.run(10)
    sa, sb = snapshot(a), snapshot(b)
    for name in ("x", "stored", "v"):
        assert torch.equal(sa[name][1:], sb[name][86:]), name
    for name in set(sa) - {"x", "stored", "v"}:
        assert torch.equal(sa[name][1], sb[name][1]), name
    assert not torch.equal(sa["x"][:1], sb["x"][:1])


# 6 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ("nvt", "npt"))
def test_two_runs_give_the_same_bits_and_reading_changes_nothing(device, ensemble):
    systems = B.batch(B.COUNTS)
    make = B.batched_nvt if ensemble == "nvt" else B.batched_npt
    a, b, c = (make(systems, device, torch.float32) for _ in range(3))
    a.run(10)
    b.run(10)
    for _ in range(10):
        c.step()
        c.velocities, c.kinetic_energy, c.temperature, c.potential_energy, c.nsteps
    assert same_snapshots(snapshot(a), snapshot(b)), "two runs of the same inputs differ"
    assert same_snapshots(snapshot(a), snapshot(c)), "reading velocities / kinetic_energy / temperature at every step changed the run"
    other = make(systems, device, torch.float32, seed=[q["seed"] + 1 for q in systems])
    other.run(10)
    assert not torch.equal(other.positions, a.positions)  # (the seeds matter)


# 7 ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ("nvt", "npt"))
def test_state_dict_round_trip_continues_bit_for_bit(device, ensemble):
    systems = B.batch(B.COUNTS)
    make = B.batched_nvt if ensemble == "nvt" else B.batched_npt
    whole = make(systems, device, torch.float32)
    whole.run(12)
    first = make(systems, device, torch.float32)
    first.run(5)
    state = first.state_dict()
    assert state["nsteps"].tolist() == [5] * 6 and state["seeds"] == [q["seed"] for q in systems]
    second = make(systems, device, torch.float32, seed=5)
    second.run(3)
    second.set_temperature(1.0), second.set_friction(0.0), second.set_timestep(2.0 * B.DT)
    if ensemble == "npt":
        second.set_pressure(3.0 * B.P0), second.set_barostat(2.0 * B.COMPRESSIBILITY, 3.0 * B.TAUP)
    second.load_state_dict(state)
    second.run(7)
    assert second.nsteps.tolist() == [12] * 6 and same_snapshots(snapshot(second), snapshot(whole))


# 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_setters_in_mid_run_act_on_the_named_systems_only(device):
    systems = B.batch(B.COUNTS)
    drv, twin = B.batched_npt(systems, device), B.batched_npt(systems, device)
    alone = B.single_npt(systems[2], device)
    drv.run(3), twin.run(3), alone.run(3)
    temperature, friction, dt = drv.target_temperature, drv.friction, drv.timestep
    pressure, compressibility, taup = drv.target_pressure, drv.compressibility, drv.taup
    temperature[2], friction[2], dt[2], pressure[2], compressibility[2], taup[2] = 900.0, 5.0 * friction[2], 0.5 * dt[2], 0.05, 0.3, 2 * taup[2]
    drv.set_temperature(temperature), drv.set_friction(friction), drv.set_timestep(dt)
    drv.set_pressure(pressure), drv.set_barostat(compressibility, taup)
    alone.set_temperature(900.0), alone.set_friction(friction[2]), alone.set_timestep(dt[2])
    alone.set_pressure(0.05), alone.set_barostat(0.3, taup[2])
    drv.run(4), twin.run(4), alone.run(4)
    a, c = snapshot(drv), snapshot(twin)
    b = B.offsets(systems)
    for s in (0, 1, 3, 4, 5):
        lo, hi = int(b[s]), int(b[s + 1])
        assert all(torch.equal(a[name][lo:hi], c[name][lo:hi]) for name in ("x", "stored", "v")), f"system {s} was touched"
        assert all(torch.equal(a[name][s], c[name][s]) for name in set(a) - {"x", "stored", "v"}), f"system {s} was touched"
    assert not torch.equal(a["x"][int(b[2]):int(b[3])], c["x"][int(b[2]):int(b[3])])
    assert_system_is_the_single_run(a, 2, int(b[2]), int(b[3]), alone, "the system whose parameters were set")


# 9 ---------------------------------------------------------------------------------------------------------------------------------
def test_kernel_path_and_aten_path_agree(device):
    systems = B.batch((1, 85, 86, 171))
    hip, aten = B.batched_nvt(systems, device, torch.float32), B.batched_nvt(systems, device, torch.float32, backend="aten")
    assert hip._hip and not aten._hip and aten.positions.is_cuda
    hip.run(25), aten.run(25)
    t_max = max(q["temperature"] for q in systems)
    np.testing.assert_allclose(hip.positions.cpu().numpy(), aten.positions.cpu().numpy(), rtol=LR.RTOL, atol=LR.X_ATOL)
    np.testing.assert_allclose(hip.velocities.cpu().numpy(), aten.velocities.cpu().numpy(), rtol=LR.RTOL, atol=LR.v_atol(t_max))
    np.testing.assert_allclose(hip.kinetic_energy.cpu().numpy(), aten.kinetic_energy.cpu().numpy(), rtol=LR.RTOL)
    assert torch.equal(hip.nsteps, aten.nsteps) and hip.nsteps.tolist() == [25] * 4

    hip, aten = B.batched_npt(systems, device, torch.float32), B.batched_npt(systems, device, torch.float32, backend="aten")
    assert hip._hip and not aten._hip and aten.cell.is_cuda
    refs = [B.restated_npt(q, device, torch.float32) for q in systems]
    hip.run(25), aten.run(25)
    for s, (q, ref) in enumerate(zip(systems, refs)):
        ref.run(25)
        NR.assert_close(B.View(aten, s), ref, f"ATen path on the device, system {s}", q["temperature"], q["part"])
        bound = NR.bounds(ref, 25, q["temperature"], q["part"])
        h, a = B.View(hip, s), B.View(aten, s)
        np.testing.assert_allclose(h.positions.cpu().numpy(), a.positions.cpu().numpy(), rtol=NR.RTOL, atol=bound["x_atol"])
        np.testing.assert_allclose(h.velocities.cpu().numpy(), a.velocities.cpu().numpy(), rtol=NR.RTOL, atol=bound["v_atol"])
        np.testing.assert_allclose(h.cell.cpu().numpy(), a.cell.cpu().numpy(), rtol=bound["cell_rtol"], atol=0)
        np.testing.assert_allclose(h.kinetic_energy, a.kinetic_energy, rtol=NR.RTOL)
        np.testing.assert_allclose(h.pressure, a.pressure, rtol=0, atol=bound["p_atol"])
    assert torch.equal(hip.nsteps, aten.nsteps)


# 10 --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ensemble", ("nvt", "npt"))
def test_a_captured_step_draws_fresh_noise_per_system_at_every_replay(device, ensemble):
    """The step's launches captured once (one stream: a linear chain), forces (and stress) in static buffers that an eager call
    refreshes between replays: three replays are three eager steps of a twin, bit for bit.  The step counts, the cells and mu
    live in device memory, so nothing of them is frozen into the graph."""
    systems = B.batch(B.COUNTS)
    make = B.batched_nvt if ensemble == "nvt" else B.batched_npt
    twin = make(systems, device)
    twin.run(3)  # (first, so that the kernels are loaded before anything is captured)
    drv = make(systems, device)
    static_forces = drv.forces.clone()
    drv._forces = static_forces
    if ensemble == "npt":
        static_stress = drv.stress.clone()
        drv._stress = static_stress
    x0 = drv.positions.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        drv._launch(finish_only=False)
    assert drv.nsteps.tolist() == [0] * 6 and torch.equal(drv.positions, x0)  # (capturing ran nothing)
    seen = []
    for _ in range(3):
        graph.replay()
        out = drv.force_step(drv.positions) if ensemble == "nvt" else drv.force_step(drv.positions, drv.cell)
        static_forces.copy_(out["forces"])
        if ensemble == "npt":
            static_stress.copy_(out["stress"])
        seen.append(drv._vel.clone())
    torch.cuda.synchronize()
    assert drv.nsteps.tolist() == [3] * 6 and not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    assert same_snapshots(snapshot(drv), snapshot(twin))


# 11 --------------------------------------------------------------------------------------------------------------------------------
def test_entry_refusals_launch_nothing_and_name_the_argument(device):
    from nequip_amd import _lib as L

    lib = L.load()
    drv = B.batched_npt(B.batch((3, 86, 4)), device)
    stream, null = L.stream_ptr(device), L.ptr(None)
    buffers = (drv._pos, drv._vel, drv._vel_out, drv.cell, drv._rec, drv._par, drv._npt, drv._partials, drv._partials_observed)
    before = [t.clone() for t in buffers]
    f, m, x, v, vo, ch, rec, par, pa, cb, npt, sig, cell = (L.ptr(t) for t in (
        drv.forces, drv._m, drv._pos, drv._vel, drv._vel_out, drv._chunks, drv._rec, drv._par, drv._partials, drv._chunk_begin,
        drv._npt, drv.stress, drv.cell))
    F64, nc, S = L.NQA_F64, drv._n_chunks, drv.num_systems

    def refused(rc, word):
        message = lib.nqa_last_error()
        assert rc != 0 and word in message, (rc, word, message)

    step = lambda **kw: lib.nqa_md_batched_langevin_step(*[kw.get(name, value) for name, value in (  # noqa: E731
        ("dtype", F64), ("forces", f), ("masses", m), ("positions", x), ("velocities", v), ("vel_out", vo), ("chunks", ch),
        ("num_chunks", nc), ("states", rec), ("params", par), ("partials", pa), ("mode", 0), ("stream", stream))])
    for name in ("forces", "masses", "positions", "velocities", "chunks", "states", "params", "partials"):
        refused(step(**{name: null}), name.encode())
    refused(step(vel_out=null, mode=1), b"vel_out")
    refused(step(num_chunks=0), b"num_chunks")
    refused(step(num_chunks=-1), b"num_chunks")
    refused(step(dtype=7), b"force_dtype")
    refused(step(mode=2), b"mode")
    refused(step(mode=4), b"mode")

    bath = lambda **kw: lib.nqa_md_batched_bath(*[kw.get(name, value) for name, value in (  # noqa: E731
        ("partials", pa), ("chunk_begin", cb), ("states", rec), ("num_systems", S), ("mode", 0), ("stream", stream))])
    for name in ("partials", "chunk_begin", "states"):
        refused(bath(**{name: null}), name.encode())
    refused(bath(num_systems=0), b"num_systems")
    refused(bath(mode=2), b"mode")

    npt_bath = lambda **kw: lib.nqa_md_batched_npt_bath(*[kw.get(name, value) for name, value in (  # noqa: E731
        ("partials", pa), ("chunk_begin", cb), ("states", rec), ("params", par), ("npt", npt), ("dtype", F64), ("stress", sig),
        ("cell", cell), ("num_systems", S), ("stream", stream))])
    for name in ("partials", "chunk_begin", "states", "params", "npt", "stress", "cell"):
        refused(npt_bath(**{name: null}), name.encode())
    refused(npt_bath(num_systems=0), b"num_systems")
    refused(npt_bath(num_systems=-5), b"num_systems")
    refused(npt_bath(dtype=7), b"stress_dtype")

    scale = lambda **kw: lib.nqa_md_batched_npt_scale(*[kw.get(name, value) for name, value in (  # noqa: E731
        ("positions", x), ("velocities", v), ("chunks", ch), ("num_chunks", nc), ("npt", npt), ("stream", stream))])
    for name in ("positions", "velocities", "chunks", "npt"):
        refused(scale(**{name: null}), name.encode())
    refused(scale(num_chunks=0), b"num_chunks")
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, buffers))  # (nothing ran)
    assert drv.nsteps.tolist() == [0, 0, 0]


# 12 --------------------------------------------------------------------------------------------------------------------------------
def test_a_cell_without_volume_fails_its_own_system_only(device):
    """A value check inside the kernel: ``V = 0`` leaves ``mu = 1`` and sets the flag of that system; nothing faults."""
    systems = B.batch((3, 86, 4))
    drv, twin = B.batched_npt(systems, device), B.batched_npt(systems, device)
    state = drv.state_dict()
    state["cell"][1, 2] = 0.0  # a lattice vector of zeros: every term of the determinant is exactly 0
    drv.load_state_dict(state)
    assert drv.failed.tolist() == [False] * 3
    drv.step(), twin.step()
    assert drv.failed.tolist() == [False, True, False] and float(drv.scaling[1]) == 1.0
    assert float(drv._npt[1, M._NPT_VOLUME]) == 0.0
    b = B.offsets(systems)
    for s in (0, 2):
        lo, hi = int(b[s]), int(b[s + 1])
        assert torch.equal(drv.cell[s], twin.cell[s]) and torch.equal(drv.positions[lo:hi], twin.positions[lo:hi])
        assert torch.equal(drv._vel[lo:hi], twin._vel[lo:hi]) and torch.equal(drv.scaling[s], twin.scaling[s])
    drv.step()
    assert drv.failed.tolist() == [False, True, False]  # (the flag stays)
    for read in (lambda: drv.nsteps, lambda: drv.pressure, lambda: drv.volume):
        with pytest.raises(RuntimeError, match=r"barostat of system\(s\) \[1\]"):
            read()
    assert twin.nsteps.tolist() == [1, 1, 1]


# 13 --------------------------------------------------------------------------------------------------------------------------------
def test_lockstep_with_the_real_model_through_the_torchsim_calculator(device):
    """Eight perturbed periodic water boxes (24 and 81 atoms, the boxes of the torch-sim test of tests/test_fire_gpu.py) through
    ``NequIPTorchSimCalc`` and ``from_torchsim``: five NVT and five NPT steps of the kernels against the ATen form, which is
    handed, at every step, the forces (and stresses) the kernel route just obtained (the model's forces are not reproducible to
    the bit): the integrator alone is compared, at the tolerances of the single-system lockstep tests.  The targets of the
    barostats lie 2 eV/A^3 above or below any pressure the model gives, so that ``a |p0 - P|`` exceeds the largest value the
    noise term can take (``sqrt(-2 log u1) <= 8.6``) and every volume must move the way its pressure error says."""
    from nequip_amd.integrations.md import maxwell_boltzmann_velocities, units
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn

    z_of, mass_of = {"H": 1, "O": 8}, {"H": 1.008, "O": 15.999}
    rng = np.random.default_rng(7)
    pos, numbers, masses, cells, sidx = [], [], [], [], []
    for s, n_side in enumerate((2, 3, 2, 3, 3, 2, 3, 2)):
        p, types, cell, names = syn.water_box(n_side, seed=s)
        pos.append(p + 0.05 * rng.normal(size=p.shape))
        numbers += [z_of[names[t]] for t in types]
        masses += [mass_of[names[t]] for t in types]
        cells.append(cell)
        sidx += [s] * len(p)
    S = 8
    model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=2, l_max=1, parity=False,
                           num_features=8, radial_mlp_width=64, radial_mlp_depth=1, avg_num_neighbors=20.0).to(device).eval()
    calc = NequIPTorchSimCalc(model, device=device)
    t = lambda a, dtype: torch.tensor(np.asarray(a), dtype=dtype, device=device)  # noqa: E731
    x, cell, z, idx, m = (t(np.concatenate(pos), torch.float64), t(np.stack(cells), torch.float64), t(numbers, torch.long),
                          t(sidx, torch.long), t(masses, torch.float64))
    vel = maxwell_boltzmann_velocities(m.cpu(), 300.0, generator=torch.Generator().manual_seed(1)).to(device)
    temperature = [250.0 + 25.0 * s for s in range(S)]
    friction = [B.FRICTION * (1 + s % 3) for s in range(S)]
    t_max = max(temperature)

    def compare(drv, aten, what):
        a, h = snapshot(aten), snapshot(drv)
        ex, ev = float((h["x"] - a["x"]).abs().max()), float((h["v"] - a["v"]).abs().max())
        print(f"{what}: x off by {ex:.3e}, v by {ev:.3e}")
        np.testing.assert_allclose(h["x"].cpu().numpy(), a["x"].cpu().numpy(), rtol=LR.RTOL, atol=LR.X_ATOL, err_msg=what)
        np.testing.assert_allclose(h["v"].cpu().numpy(), a["v"].cpu().numpy(), rtol=LR.RTOL, atol=LR.v_atol(t_max), err_msg=what)
        np.testing.assert_allclose(h["k"].cpu().numpy(), a["k"].cpu().numpy(), rtol=LR.RTOL, err_msg=what)
        return a, h

    # NVT
    drv = BatchedLangevin.from_torchsim(calc, x, cell, True, z, idx, m, B.DT, temperature, friction, velocities=vel, seed=LR.SEED)
    given = lambda positions: {"forces": drv.forces.clone(), "total_energy": drv.potential_energy}  # noqa: E731
    aten = BatchedLangevin(given, m, B.DT, temperature, friction, x, idx, vel, seed=LR.SEED, backend="aten")
    assert drv._hip and not aten._hip and drv.forces.is_cuda
    for k in range(5):
        drv.step(), aten.step()
        compare(drv, aten, f"NVT, step {k + 1}")
    assert drv.nsteps.tolist() == [5] * S and drv.potential_energy.shape == (S,)
    assert bool(torch.isfinite(drv.potential_energy).all()) and bool(torch.isfinite(drv.positions).all())

    # NPT
    target = [2.0 if s % 2 else -2.0 for s in range(S)]
    args = (B.DT, temperature, friction, target, B.COMPRESSIBILITY, B.TAUP)
    npt = BatchedLangevinNPT.from_torchsim(calc, x, cell, True, z, idx, m, *args, velocities=vel, seed=LR.SEED)
    assert calc.compute_stress and npt.stress.shape == (S, 3, 3)
    given = lambda positions, cells: {"forces": npt.forces.clone(), "stress": npt.stress.clone(),  # noqa: E731
                                      "total_energy": npt.potential_energy}
    aten = BatchedLangevinNPT(given, m, *args, x, cell, idx, vel, seed=LR.SEED, backend="aten")
    a_bar = B.COMPRESSIBILITY * B.DT / B.TAUP
    for k in range(5):
        volume = npt.volume.clone()
        npt.step(), aten.step()
        what = f"NPT, step {k + 1}"
        a, h = compare(npt, aten, what)
        np.testing.assert_allclose(h["cell"].cpu().numpy(), a["cell"].cpu().numpy(), rtol=LR.RTOL, atol=LR.X_ATOL, err_msg=what)
        np.testing.assert_allclose(h["pressure"].cpu().numpy(), a["pressure"].cpu().numpy(), rtol=LR.RTOL, atol=1e-12, err_msg=what)
        error = torch.tensor(target, dtype=torch.float64, device=device) - h["pressure"]
        noise_max = 8.6 * torch.sqrt(2.0 * units.kB * t_max * a_bar / volume)
        print(f"{what}: P {h['pressure'].tolist()}, volumes {h['volume'].tolist()}")
        assert bool((a_bar * error.abs() > noise_max).all()), "the targets do not dominate the noise: the check below says nothing"
        assert torch.equal(torch.sign(h["volume"] - volume), -torch.sign(error)), f"{what}: a volume moved against its pressure error"
    assert npt.nsteps.tolist() == [5] * S and bool(torch.isfinite(npt.potential_energy).all())
    assert bool(torch.isfinite(npt.positions).all()) and not bool(npt.failed.any())
