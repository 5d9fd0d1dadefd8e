"""The cases of ``tests/geometry_cases.py`` against the reference's ATen formulation, on the CPU: the int64 restatements equal
float64 ATen bit for bit in any edge order -- so the grid inputs stay exact without the kernels under test -- and the derived
bound of the random cases holds for a float64 evaluation and rejects a float32 one."""
import numpy as np
import pytest
import torch

import geometry_cases as gc


def aten(case):
    """vec (CPU branch of ``with_edge_vectors_``), its position / cell gradients (``torch.autograd.grad``), the per-frame
    virial sum (``index_add_``), in float64."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.nn.utils import with_edge_vectors_

    pos = case.pos.clone().requires_grad_(True)
    data = {K.POSITIONS_KEY: pos, K.EDGE_INDEX_KEY: case.edge_index}
    cell = None
    if case.cell is not None:
        cell = case.cell.clone().requires_grad_(True)
        data[K.CELL_KEY], data[K.EDGE_CELL_SHIFT_KEY] = cell, case.shift
        if case.batch is not None:
            data[K.BATCH_KEY] = case.batch
    vec = with_edge_vectors_(data, with_lengths=False)[K.EDGE_VECTORS_KEY]
    out = {"vec": vec.detach()}
    grads = torch.autograd.grad(vec, [pos] + ([cell] if cell is not None else []), case.g, allow_unused=True)
    out["g_pos"] = grads[0] if grads[0] is not None else torch.zeros_like(case.pos)
    if cell is not None:
        out["g_cell"] = grads[1].reshape(-1, 3, 3)
    outer = (out["vec"][:, :, None] * case.g[:, None, :]).reshape(-1, 9)
    frame = case.frame_of_atom[case.edge_index[0]]
    m = torch.zeros((case.num_frames, 9), dtype=torch.float64).index_add_(0, frame, outer).view(-1, 3, 3)
    out["sym"] = 0.5 * (m + m.transpose(1, 2))
    out["rows_vec"] = torch.zeros((case.num_nodes, 9), dtype=torch.float64).index_add_(0, case.edge_index[0], outer)
    return out


@pytest.mark.parametrize("name", gc.GRID_CASES)
def test_restatement_equals_aten_bitwise_in_any_edge_order(name):
    case = gc.make_case(name)
    ref = gc.grid_reference(case)
    assert ref["peak"] < 2 ** 52, f"{name}: a restatement needs {ref['peak'].bit_length()} bits"
    perm = torch.randperm(case.num_edges, generator=torch.Generator().manual_seed(5))
    for label, c, vec_ref in (("given", case, ref["vec"]), ("permuted", case.permuted(perm), ref["vec"][perm])):
        got = aten(c)
        assert torch.equal(got["vec"], vec_ref), f"{name} {label}: vec"
        assert torch.equal(got["g_pos"], ref["g_pos"]), f"{name} {label}: g_pos"
        assert torch.equal(got["rows_vec"], ref["rows_vec"]), f"{name} {label}: rows_vec"
        assert torch.equal(got["sym"], ref["sym"]), f"{name} {label}: sym"
        if case.cell is not None:
            assert torch.equal(got["g_cell"], ref["g_cell"]), f"{name} {label}: g_cell"
            assert torch.isfinite(ref["stress"]).all()
    # the permuted case restates to the same integers
    ref_p = gc.grid_reference(case.permuted(perm))
    for key in ("g_pos", "rows_shift", "rows_vec", "g_cell", "sym"):
        assert torch.equal(ref_p[key], ref[key]), key


def test_cases_have_the_shapes_they_are_named_for():
    c = gc.make_case("degrees")
    N = c.num_nodes
    assert N == 7 and N % 4 != 0
    assert torch.bincount(c.edge_index[0], minlength=N).tolist() == list(gc.DEGREES)
    as_nbr = torch.bincount(c.edge_index[1], minlength=N).tolist()
    assert sorted(as_nbr) == sorted(gc.DEGREES) and as_nbr != list(gc.DEGREES)
    loops = c.edge_index[0] == c.edge_index[1]
    assert int(loops.sum()) > 0 and bool((c.shift_i[loops] != 0).any(1).all())
    full = torch.cat([c.edge_index.t(), c.shift_i], 1)
    assert len(torch.unique(full, dim=0)) < c.num_edges  # exact duplicates
    assert (torch.diff(c.edge_index[0]) < 0).any()  # unsorted

    c = gc.make_case("frames_interleaved")
    assert c.num_frames == 4 and c.cell.shape == (4, 3, 3) and int((c.batch == 2).sum()) == 0
    assert (torch.diff(c.batch) < 0).any()
    dets = gc.det_int(c.cell_i)
    assert int(dets[1]) < 0 and int(dets[0]) > 0 and int((c.cell_i[3] == 0).sum()) == 0
    frame_dst, frame_src = c.batch[c.edge_index[0]], c.batch[c.edge_index[1]]
    assert (frame_dst != frame_src).any()  # the frame of an edge is its centre's: some neighbours live elsewhere
    assert int(torch.bincount(c.edge_index[0]).max()) < 64  # (the lane loop's second trip is `degrees`' business)

    for n in (1023, 1024, 1025):
        c = gc.make_case(f"one_frame_large_{n}")
        assert c.num_nodes == n and c.batch is None and c.cell.shape == (3, 3) and int(c.edge_index[0].max()) == n - 1
    for e in (255, 256, 257):
        c = gc.make_case(f"block_edges_{e}")
        assert c.num_edges == e and c.num_nodes == 33
    assert gc.make_case("block_edges_256").cell is None
    assert gc.make_case("one_atom_e5").num_edges == 5 and gc.make_case("one_atom_e0").num_edges == 0
    assert gc.make_case("no_edges").num_nodes == 9

    c = gc.make_case("symmetric_box")  # every edge has its reverse with the opposite shift
    fwd = {tuple(r) for r in torch.cat([c.edge_index.t(), c.shift_i], 1).tolist()}
    rev = {(j, i, -a, -b, -d) for (i, j, a, b, d) in fwd}
    assert fwd == rev and len(fwd) == c.num_edges and c.num_edges % 2 == 0


def test_host_csr_is_the_stable_grouping():
    key = torch.tensor([3, 0, 3, 1, 0, 3])
    other = torch.tensor([5, 4, 3, 2, 1, 0])
    rowptr, eid, oth = gc.host_csr(key, other, 5)
    assert rowptr.tolist() == [0, 2, 3, 3, 6, 6] and eid.tolist() == [1, 4, 3, 0, 2, 5] and oth.tolist() == [4, 1, 2, 5, 3, 0]
    assert rowptr.dtype == torch.int32


@pytest.mark.parametrize("name", gc.RANDOM_CASES)
def test_derived_bound_holds_for_float64_and_rejects_float32(name):
    case = gc.random_case(name)
    got = aten(case)
    v = gc.ld_vec(case)
    gc.check_bound(got["vec"], v.ref, v.bound, "vec")
    g_pos, rows = gc.ld_adjoint(case, got["vec"])
    gc.check_bound(got["g_pos"], g_pos.ref, g_pos.bound, "g_pos")
    gc.check_bound(got["rows_vec"], rows.ref, rows.bound, "rows_vec")
    _, rows_s = gc.ld_adjoint(case, case.shift)
    g_cell = gc.ld_frame_reduce(rows_s, case.batch, case.num_frames)
    gc.check_bound(got["g_cell"], g_cell.ref.reshape(-1, 3, 3), g_cell.bound.reshape(-1, 3, 3), "g_cell")
    sym = gc.ld_sym(gc.ld_frame_reduce(rows, case.batch, case.num_frames))
    gc.check_bound(got["sym"], sym.ref, sym.bound, "sym")
    vol = torch.linalg.det(case.cell.reshape(-1, 3, 3)).abs().view(-1, 1, 1)
    s_ref, s_bound = gc.ld_stress(sym, case.cell)
    gc.check_bound(got["sym"] / vol, s_ref, s_bound, "stress")
    # a result that went through float32 anywhere is far outside
    with pytest.raises(AssertionError):
        gc.check_bound(got["vec"].float().double(), v.ref, v.bound, "vec")
    with pytest.raises(AssertionError):
        gc.check_bound(got["g_pos"].float().double(), g_pos.ref, g_pos.bound, "g_pos")
    with pytest.raises(AssertionError):
        gc.check_bound(got["sym"].float().double(), sym.ref, sym.bound, "sym")
    # the forward has five addends per element: seven units of the magnitude sum, no more
    assert np.all(v.terms == 5) and np.all(v.bound <= 7 * gc.U * v.mag * (1 + 1e-15))
