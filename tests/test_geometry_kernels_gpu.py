"""The geometry kernels, launch by launch, against the restatements of ``tests/geometry_cases.py``: ``nqa_csr_build``,
``nqa_csr_from_pairs``, ``nqa_edge_vectors_fwd / bwd``, ``nqa_virial_finalize``, ``nqa_frame_sum`` and the assembled tails
(``force_virial``, the autograd of the edge vectors in both forms, to second order).

On the grid cases every comparison is ``torch.equal`` (the kernels only subtract, multiply by small factors and add, so on
dyadic inputs a correct kernel is exact in any summation order); the stress, one division, is held to 4 ulp.  The random
cases are held to the derived bound ``(terms + 2) * 2^-53 * sum|term|``.  Nothing here reads the reference tree."""
import ctypes
import functools

import pytest
import torch

import geometry_cases as gc

pytestmark = pytest.mark.gpu

CELL_CASES = tuple(n for n in gc.GRID_CASES if n != "block_edges_256")
TAIL_CASES = ("degrees", "frames_interleaved", "symmetric_box")


@functools.lru_cache(maxsize=None)
def grid(name):
    case = gc.make_case(name)
    return case, gc.grid_reference(case)


@functools.lru_cache(maxsize=None)
def rand(name):
    return gc.random_case(name)


def _to(t, device):
    return None if t is None else t.to(device).contiguous()


def _call(name, *args):
    from nequip_amd import _lib

    _lib.check(getattr(_lib.load(), name)(*args), name)


def _p(t):
    from nequip_amd import _lib

    return _lib.ptr(t)


def _stream(device):
    from nequip_amd import _lib

    return _lib.stream_ptr(device)


def _nan(shape, device):
    return torch.full(shape, float("nan"), dtype=torch.float64, device=device)


def _host_lists(case, device):
    dst, src = case.edge_index
    by_dst = tuple(t.to(device) for t in gc.host_csr(dst, src, case.num_nodes))
    by_src = tuple(t.to(device) for t in gc.host_csr(src, dst, case.num_nodes))
    return by_dst, by_src


def _fwd_abi(case, device):
    dst, src = _to(case.edge_index[0], device), _to(case.edge_index[1], device)
    pos, cell = _to(case.pos, device), _to(case.cell, device)
    shift = _to(case.shift, device) if cell is not None else None
    batch = _to(case.batch, device) if cell is not None else None
    vec = _nan((case.num_edges, 3), device)
    _call("nqa_edge_vectors_fwd", _p(pos), _p(dst), _p(src), _p(shift), _p(cell), _p(batch), case.num_edges, _p(vec),
          _stream(device))
    return vec.cpu()


def _bwd_abi(case, device, by_dst, by_src, left, sign, g=None):
    """(g_pos, rows or None) of one ``nqa_edge_vectors_bwd`` launch; outputs start as NaN: every element must be written."""
    N = case.num_nodes
    g_d, left_d = _to(case.g if g is None else g, device), _to(left, device)
    g_pos = _nan((N, 3), device)
    rows = _nan((N, 9), device) if left is not None else None
    _call("nqa_edge_vectors_bwd", _p(g_d), _p(left_d), _p(by_dst[0]), _p(by_dst[1]), _p(by_src[0]), _p(by_src[1]), N,
          ctypes.c_double(sign), _p(g_pos), _p(rows), _stream(device))
    return g_pos.cpu(), (None if rows is None else rows.cpu())


def _finalize_abi(rows, batch, cell, num_frames, device, want_stress=True):
    rows_d, batch_d, cell_d = _to(rows, device), _to(batch, device), _to(cell, device)
    virial = _nan((num_frames, 3, 3), device)
    stress = _nan((num_frames, 3, 3), device) if (want_stress and cell is not None) else None
    _call("nqa_virial_finalize", _p(rows_d), _p(batch_d), _p(cell_d if stress is not None else None), rows.shape[0],
          num_frames, _p(virial), _p(stress), _stream(device))
    return virial.cpu(), (None if stress is None else stress.cpu())


def _assert_stress(got, ref):
    assert torch.isfinite(got).all()
    torch.testing.assert_close(got, ref, rtol=gc.STRESS_RTOL, atol=0)


# ---- (a) nqa_csr_build -------------------------------------------------------------------------------------------------


def _check_csr(device, key, other, N):
    from nequip_amd.nn._topology import EdgeTopology

    E = key.numel()
    topo = EdgeTopology(key.to(device), other.to(device), N)
    for got, (k, o) in ((topo.by_dst, (key, other)), (topo.by_src, (other, key))):
        rowptr, eid, oth = gc.host_csr(k, o, N)
        assert got[0].dtype == torch.int32 and got[0].shape == (N + 1,)
        assert torch.equal(got[0].cpu(), rowptr)
        assert torch.equal(got[1][:E].cpu(), eid)
        assert torch.equal(got[2][:E].cpu(), oth)


@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 65535, 65536, 65537])
def test_csr_build_key_width(device, N):
    """The radix sort only looks at ``end_bit_for(N)`` key bits: N = 2^k and 2^k +- 1, keys up to N - 1, E = 1000."""
    gen = torch.Generator().manual_seed(N)
    E = 1000
    key, other = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    key[::97], other[5::89] = N - 1, N - 1
    key[1::101] = 0
    _check_csr(device, key, other, N)


@pytest.mark.parametrize("shape", ["isolated_ends", "one_node", "E0", "E1", "E255", "E256", "E257"])
def test_csr_build_rows_and_order(device, shape):
    """``rowptr`` is the count prefix, the order inside a row is the original edge order, on unsorted, repeated, directed
    lists: isolated nodes at 0 and N - 1, every edge on one node, edge counts around the block size."""
    gen = torch.Generator().manual_seed(11)
    if shape == "isolated_ends":
        N, E = 40, 600
        key, other = torch.randint(1, N - 1, (E,), generator=gen), torch.randint(1, N - 1, (E,), generator=gen)
        key[100:110], other[100:110] = key[0], other[0]  # repeated edges
    elif shape == "one_node":
        N, E = 5, 700
        key, other = torch.full((E,), 3), torch.randint(0, N, (E,), generator=gen)
    else:
        N, E = 10, int(shape[1:])
        key, other = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    _check_csr(device, key, other, N)


@pytest.mark.parametrize("side,value", [("key", -1), ("key", "N"), ("other", -1), ("other", "N")])
def test_csr_build_reports_an_index_out_of_range(device, side, value):
    from nequip_amd.nn._topology import EdgeTopology

    N, E = 12, 300
    gen = torch.Generator().manual_seed(2)
    key, other = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    good = EdgeTopology(key.to(device), other.to(device), N)
    good.check_indices = True
    good.by_dst  # a list in range passes the check
    (key if side == "key" else other)[123] = N if value == "N" else value
    topo = EdgeTopology(key.to(device), other.to(device), N)
    topo.check_indices = True  # on the instance: the class default stays off
    with pytest.raises(RuntimeError, match="out of range"):
        topo.by_dst
    assert EdgeTopology.check_indices is False


@pytest.mark.parametrize("hand_over", ["rowptr_dst", "csr_dst"])
def test_csr_identity_hand_overs_equal_the_sort(device, hand_over):
    from nequip_amd.nn._topology import EdgeTopology

    N, E = 50, 900
    gen = torch.Generator().manual_seed(4)
    dst = torch.sort(torch.randint(1, N - 1, (E,), generator=gen)).values  # grouped by destination
    src = torch.randint(0, N, (E,), generator=gen)
    rowptr, eid, oth = (t.to(device) for t in gc.host_csr(dst, src, N))
    dst_d, src_d = dst.to(device), src.to(device)
    sorted_topo = EdgeTopology(dst_d, src_d, N)
    if hand_over == "rowptr_dst":
        topo = EdgeTopology(dst_d, src_d, N, rowptr_dst=rowptr)
    else:
        topo = EdgeTopology(dst_d, src_d, N, csr_dst=(rowptr, eid, oth))
    assert topo._dst_is_identity and not sorted_topo._dst_is_identity
    for a, b in zip(topo.by_dst + topo.by_src, sorted_topo.by_dst + sorted_topo.by_src):
        assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)


# ---- (b) nqa_csr_from_pairs --------------------------------------------------------------------------------------------


def _paired_topology(case, device, monkeypatch):
    from nequip_amd.nn._topology import EdgeTopology

    monkeypatch.delenv("NQA_NO_PAIRED", raising=False)
    ei = case.edge_index.to(device)
    topo = EdgeTopology(ei[0].contiguous(), ei[1].contiguous(), case.num_nodes)
    assert topo.pairing(case.shift.to(device)) is not None
    return topo


def test_csr_from_pairs_lists_the_same_edges_as_the_sort(device, monkeypatch):
    from nequip_amd.nn._topology import EdgeTopology

    case, _ = grid("symmetric_box")
    N, E = case.num_nodes, case.num_edges
    topo = _paired_topology(case, device, monkeypatch)
    rp_d, _, _ = topo.by_dst
    rp_s, eid_s, _ = topo.by_src
    assert rp_s is rp_d  # the pairing shares the row pointer: nqa_csr_from_pairs built the list
    monkeypatch.setenv("NQA_NO_PAIRED", "1")
    ei = case.edge_index.to(device)
    plain = EdgeTopology(ei[0].contiguous(), ei[1].contiguous(), N)
    assert plain.pairing(case.shift.to(device)) is None
    rp_p, eid_p, _ = plain.by_src
    assert torch.equal(rp_s.cpu(), rp_p.cpu())
    rp = rp_s.cpu().to(torch.int64)
    row_of_slot = torch.repeat_interleave(torch.arange(N), rp[1:] - rp[:-1])
    got, want = eid_s[:E].cpu().to(torch.int64), eid_p[:E].cpu().to(torch.int64)
    assert torch.equal(case.edge_index[1][got], row_of_slot)  # every listed edge's src is the row's atom
    assert torch.equal(torch.sort(row_of_slot * E + got).values, torch.sort(row_of_slot * E + want).values)  # same sets
    assert torch.equal(torch.sort(got).values, torch.arange(E))


# ---- (c) nqa_edge_vectors_fwd ------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", gc.GRID_CASES)
def test_edge_vectors_fwd_bitwise(device, name):
    from nequip_amd.nn.utils import _EdgeVectorsFn

    case, ref = grid(name)
    has_cell = case.cell is not None
    vec = _EdgeVectorsFn.apply(_to(case.pos, device), _to(case.cell, device), _to(case.edge_index, device),
                               _to(case.shift, device) if has_cell else None, _to(case.batch, device) if has_cell else None)
    assert vec.dtype == torch.float64 and torch.equal(vec.cpu(), ref["vec"])
    assert torch.equal(_fwd_abi(case, device), ref["vec"])


# ---- (d) nqa_edge_vectors_bwd ------------------------------------------------------------------------------------------


def _check_bwd_bitwise(case, ref, device, by_dst, by_src):
    lefts = {"none": (None, None), "shift": (case.shift, ref["rows_shift"]), "vec": (ref["vec"], ref["rows_vec"])}
    for sign in (1.0, -1.0):
        for label, (left, rows_ref) in lefts.items():
            g_pos, rows = _bwd_abi(case, device, by_dst, by_src, left, sign)
            assert torch.equal(g_pos, sign * ref["g_pos"]), f"g_pos, sign {sign}, left {label}"
            if left is not None:
                assert torch.equal(rows, rows_ref), f"rows, sign {sign}, left {label}"
    centre_deg = torch.bincount(case.edge_index[0], minlength=case.num_nodes)
    assert not ref["rows_vec"][centre_deg == 0].any()  # atoms without edges as centre: exact zero rows


@pytest.mark.parametrize("name", gc.GRID_CASES)
def test_edge_vectors_bwd_bitwise(device, name):
    """Both signs; ``g_cell_per_node`` NULL and given; left factor = shift (autograd) and = edge vectors (inference)."""
    case, ref = grid(name)
    by_dst, by_src = _host_lists(case, device)
    _check_bwd_bitwise(case, ref, device, by_dst, by_src)


def test_edge_vectors_bwd_bitwise_on_device_built_lists(device, monkeypatch):
    """The same through the lists the device builds: the sort (frames_interleaved) and the pairing (symmetric_box)."""
    from nequip_amd.nn._topology import EdgeTopology

    case, ref = grid("frames_interleaved")
    ei = case.edge_index.to(device)
    topo = EdgeTopology(ei[0].contiguous(), ei[1].contiguous(), case.num_nodes)
    _check_bwd_bitwise(case, ref, device, topo.by_dst, topo.by_src)
    case, ref = grid("symmetric_box")
    topo = _paired_topology(case, device, monkeypatch)
    assert topo.by_src[0] is topo.by_dst[0]
    _check_bwd_bitwise(case, ref, device, topo.by_dst, topo.by_src)


# ---- (e) nqa_virial_finalize -------------------------------------------------------------------------------------------


@pytest.mark.parametrize("name", gc.GRID_CASES)
def test_virial_finalize_bitwise(device, name):
    case, ref = grid(name)
    B = case.num_frames
    batch = case.batch if B > 1 else None  # (num_frames = 1 runs with batch = None)
    cell = None if case.cell is None else case.cell.reshape(-1, 3, 3)
    virial, stress = _finalize_abi(ref["rows_vec"], batch, cell, B, device)
    assert torch.equal(virial, -ref["sym"]) and torch.equal(virial, ref["virial"])
    assert torch.equal(virial, virial.transpose(1, 2))
    if cell is None:
        assert stress is None
    else:
        _assert_stress(stress, ref["stress"])
        virial2, none = _finalize_abi(ref["rows_vec"], batch, cell, B, device, want_stress=False)  # stress = NULL
        assert none is None and torch.equal(virial2, virial)
        mirror = cell.clone()
        mirror[:, 0] = -mirror[:, 0]  # the mirror image of every cell: the other handedness, the same volume
        _, stress_m = _finalize_abi(ref["rows_vec"], batch, mirror, B, device)
        assert torch.equal(stress_m, stress)
    if name == "frames_interleaved":
        assert not virial[2].any() and not stress[2].any() and torch.isfinite(stress[2]).all()  # the empty frame
        assert int(gc.det_int(case.cell_i)[1]) < 0  # the left-handed frame: stress = sym / |det|, as for its mirror image
        assert torch.equal(torch.sign(stress[1]), torch.sign(ref["sym"][1]))


# ---- (f) nqa_frame_sum -------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("N", [0, 1, 255, 256, 257])
@pytest.mark.parametrize("K", [1, 3, 15, 16])
def test_frame_sum_bitwise(device, N, K):
    from nequip_amd.nn.utils import frame_sum

    gen = torch.Generator().manual_seed(100 * N + K)
    B = 3
    rows_i = torch.randint(-gc.G_MAX, gc.G_MAX + 1, (N, K), generator=gen, dtype=torch.int64)
    batch = torch.tensor([2, 0])[torch.randint(0, 2, (N,), generator=gen)]  # unsorted; frame 1 stays empty
    rows = gc.exact(rows_i, gc.G_BITS)
    out = frame_sum(rows.to(device), batch.to(device), B)
    assert out.shape == (B, K) and torch.equal(out.cpu(), gc.exact(gc.frame_sum_int(rows_i, batch, B), gc.G_BITS))
    one = _nan((1, K), device)  # B = 1 with batch = None, through the C ABI
    rows_d = rows.to(device)
    _call("nqa_frame_sum", _p(rows_d), _p(None), N, K, 1, _p(one), _stream(device))
    assert torch.equal(one.cpu(), gc.exact(rows_i.sum(0, keepdim=True), gc.G_BITS))


# ---- (g) the assembled tails -------------------------------------------------------------------------------------------


def _forms():
    from nequip_amd.nn.utils import _EdgeVectorsFn

    return {"function": _EdgeVectorsFn.apply, "dispatcher": torch.ops.nequip_amd.edge_vectors}


def _inputs(case, device):
    pos = _to(case.pos, device).requires_grad_(True)
    cell = _to(case.cell, device)
    if cell is not None:
        cell.requires_grad_(True)
    has_cell = cell is not None
    return pos, cell, _to(case.edge_index, device), (_to(case.shift, device) if has_cell else None), \
        (_to(case.batch, device) if has_cell else None)


@pytest.mark.parametrize("name", TAIL_CASES)
def test_force_virial_bitwise(device, name, monkeypatch):
    from nequip_amd.nn._topology import topology_cache

    case, ref = grid(name)
    N, B = case.num_nodes, case.num_frames
    ei = _to(case.edge_index, device)
    if name == "symmetric_box":  # the tail then walks the by-source lists of the pairing
        monkeypatch.delenv("NQA_NO_PAIRED", raising=False)
        assert topology_cache.get(ei[0], ei[1], N).pairing(_to(case.shift, device)) is not None
    g, vec = _to(case.g, device), _to(ref["vec"], device)
    cell = _to(case.cell.reshape(-1, 3, 3), device)
    forces, virial, stress = torch.ops.nequip_amd.force_virial(g, vec, ei, _to(case.batch, device), cell, N, B)
    assert torch.equal(forces.cpu(), -ref["g_pos"])
    assert torch.equal(virial.cpu(), ref["virial"])
    _assert_stress(stress.cpu(), ref["stress"])
    if B == 1:
        forces, virial, stress = torch.ops.nequip_amd.force_virial(g, vec, ei, None, None, N, 1)
        assert stress.shape == (0,) and torch.equal(forces.cpu(), -ref["g_pos"]) and torch.equal(virial.cpu(), ref["virial"])


@pytest.mark.parametrize("form", ["function", "dispatcher"])
@pytest.mark.parametrize("name", gc.GRID_CASES)
def test_edge_vector_gradients_bitwise(device, name, form):
    """``grad(edge_vec, [pos, cell], g)``: [B, 3, 3] cells reduce through ``nqa_frame_sum``, [3, 3] and [1, 3, 3] through an
    ATen sum (exact on the grid)."""
    case, ref = grid(name)
    pos, cell, ei, shift, batch = _inputs(case, device)
    vec = _forms()[form](pos, cell, ei, shift, batch)
    assert torch.equal(vec.detach().cpu(), ref["vec"])
    grads = torch.autograd.grad(vec, [pos] + ([cell] if cell is not None else []), _to(case.g, device))
    assert torch.equal(grads[0].cpu(), ref["g_pos"])
    if cell is not None:
        assert grads[1].shape == case.cell.shape and torch.equal(grads[1].cpu().reshape(-1, 3, 3), ref["g_cell"])


# ---- (h) second order --------------------------------------------------------------------------------------------------


@pytest.mark.parametrize("pattern", ["pos", "cell", "both"])
@pytest.mark.parametrize("form", ["function", "dispatcher"])
@pytest.mark.parametrize("name", TAIL_CASES + ("one_atom_e5",))
def test_second_order_is_the_forward_map_of_the_cotangents(device, name, form, pattern):
    """d(g_pos, g_cell)/d g_vec contracted with (c_pos, c_cell) = the edge vectors of (c_pos, c_cell): the map is linear.
    Cell only -- a stress-only loss -- gives ``shift @ c_cell[frame]``."""
    case, ref = grid(name)
    gen = torch.Generator().manual_seed(9)
    c_pos_i = torch.randint(-gc.POS_MAX, gc.POS_MAX + 1, case.pos.shape, generator=gen, dtype=torch.int64)
    c_cell_i = torch.randint(-gc.CELL_MAX, gc.CELL_MAX + 1, case.cell.shape, generator=gen, dtype=torch.int64)
    want = gc.exact(gc.vec_int(gc.Case(
        "cotangents", case.pos, case.edge_index, case.shift, case.cell, case.batch, case.g,
        pos_i=c_pos_i if pattern != "cell" else torch.zeros_like(c_pos_i), shift_i=case.shift_i,
        cell_i=c_cell_i if pattern != "pos" else None)), gc.VEC_BITS)

    pos, cell, ei, shift, batch = _inputs(case, device)
    g_vec = _to(case.g, device).requires_grad_(True)
    vec = _forms()[form](pos, cell, ei, shift, batch)
    g_pos, g_cell = torch.autograd.grad(vec, [pos, cell], g_vec, create_graph=True)
    assert torch.equal(g_pos.detach().cpu(), ref["g_pos"])
    assert torch.equal(g_cell.detach().cpu().reshape(-1, 3, 3), ref["g_cell"])
    c_pos, c_cell = _to(gc.exact(c_pos_i, gc.POS_BITS), device), _to(gc.exact(c_cell_i, gc.CELL_BITS), device)
    outs, cots = {"pos": ([g_pos], [c_pos]), "cell": ([g_cell], [c_cell]), "both": ([g_pos, g_cell], [c_pos, c_cell])}[pattern]
    (got,) = torch.autograd.grad(outs, g_vec, cots)
    assert torch.equal(got.cpu(), want)


# ---- (i) random inputs at the derived bound ----------------------------------------------------------------------------


@pytest.mark.parametrize("name", gc.RANDOM_CASES)
def test_random_inputs_forward_and_adjoint_kernels(device, name):
    from nequip_amd.nn.utils import _EdgeVectorsFn

    case = rand(name)
    v = gc.ld_vec(case)
    vec = _EdgeVectorsFn.apply(_to(case.pos, device), _to(case.cell, device), _to(case.edge_index, device),
                               _to(case.shift, device), _to(case.batch, device)).cpu()
    gc.check_bound(vec, v.ref, v.bound, "vec")
    gc.check_bound(_fwd_abi(case, device), v.ref, v.bound, "vec (C ABI)")
    by_dst, by_src = _host_lists(case, device)
    for label, left in (("shift", case.shift), ("vec", vec)):  # (the left factor is an input: the kernel's own vectors)
        g_pos_ref, rows_ref = gc.ld_adjoint(case, left)
        for sign in (1.0, -1.0):
            g_pos, rows = _bwd_abi(case, device, by_dst, by_src, left, sign)
            gc.check_bound(sign * g_pos, g_pos_ref.ref, g_pos_ref.bound, f"g_pos, sign {sign}")
            gc.check_bound(rows, rows_ref.ref, rows_ref.bound, f"rows, left {label}")


@pytest.mark.parametrize("name", gc.RANDOM_CASES)
def test_random_inputs_virial_finalize(device, name):
    case = rand(name)
    B, N = case.num_frames, case.num_nodes
    rows = torch.randn((N, 9), dtype=torch.float64, generator=torch.Generator().manual_seed(6))
    batch = case.batch if B > 1 else None
    cell = case.cell.reshape(-1, 3, 3)
    sym = gc.ld_sym(gc.ld_frame_reduce(gc.ld_given_rows(rows), batch, B))
    virial, stress = _finalize_abi(rows, batch, cell, B, device)
    gc.check_bound(-virial, sym.ref, sym.bound, "virial")
    s_ref, s_bound = gc.ld_stress(sym, cell)
    gc.check_bound(stress, s_ref, s_bound, "stress")


@pytest.mark.parametrize("name", gc.RANDOM_CASES)
def test_random_inputs_assembled_tails(device, name):
    case = rand(name)
    N, B = case.num_nodes, case.num_frames
    pos, cell, ei, shift, batch = _inputs(case, device)
    for form, fwd in _forms().items():
        vec = fwd(pos, cell, ei, shift, batch)
        g_pos, g_cell = torch.autograd.grad(vec, [pos, cell], _to(case.g, device))
        g_pos_ref, rows_s = gc.ld_adjoint(case, case.shift)
        gc.check_bound(g_pos.cpu(), g_pos_ref.ref, g_pos_ref.bound, f"{form}: g_pos")
        g_cell_ref = gc.ld_frame_reduce(rows_s, case.batch, B)
        gc.check_bound(g_cell.cpu().reshape(B, 9), g_cell_ref.ref, g_cell_ref.bound, f"{form}: g_cell")
    vec = vec.detach()
    g_pos_ref, rows_v = gc.ld_adjoint(case, vec.cpu())
    sym = gc.ld_sym(gc.ld_frame_reduce(rows_v, case.batch, B))
    forces, virial, stress = torch.ops.nequip_amd.force_virial(_to(case.g, device), vec, ei, batch,
                                                               cell.detach().reshape(-1, 3, 3), N, B)
    gc.check_bound(-forces.cpu(), g_pos_ref.ref, g_pos_ref.bound, "forces")
    gc.check_bound(-virial.cpu(), sym.ref, sym.bound, "virial")
    s_ref, s_bound = gc.ld_stress(sym, case.cell)
    gc.check_bound(stress.cpu(), s_ref, s_bound, "stress")
