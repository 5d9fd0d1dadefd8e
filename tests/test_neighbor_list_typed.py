"""Typed device neighbour list (``nqa_neighbor_list_*_typed``: per-edge-type cutoffs) through ``nequip_amd.data._nl``.

1. against a brute-force numpy enumeration over lattice images filtered with ``r < r_max and r <= rc[t_i][t_j]``: identical
   ``(i, j, S)`` sets on orthorhombic / triclinic / thin / partially periodic / cell-less frames, 1, 2 and 5 types, symmetric and
   asymmetric tables, and a table whose every entry is below ``r_max``;
2. bitwise (order, ``edge_cell_shift``, ``rowptr``) against "untyped list, then mask", single frame and batched; batched ==
   concatenation of the typed single-frame lists over frames of different periodicity;
3. a table filled with ``r_max`` gives bitwise the untyped list;
4. the capacity-padded form: real edges == the symmetrised-table list, every other slot a self image longer than ``r_max``,
   ``rowptr_padded[N] == capacity``, the does-not-fit status;
5. an out-of-range type raises ``ValueError`` (no fault); a table entry above ``r_max`` raises before any launch.

Precondition asserted on every input: no candidate distance lies within 1e-9 A of ``r_max`` or of a table entry (float rounding
at a boundary is not what is tested); a frame that fails it fails the test.
"""

import itertools

import numpy as np
import pytest
import torch

GAP = 1e-9


def _candidates(pos, cell, pbc, r_reach):
    """All (i, j, S, r) with r < r_reach, i == j and S == 0 excluded (float64)."""
    pos = np.asarray(pos, dtype=np.float64)
    n = len(pos)
    if cell is None:
        cell, pbc = np.eye(3), (False,) * 3
    cell = np.asarray(cell, dtype=np.float64)
    inv = np.linalg.inv(cell)
    heights = 1.0 / np.linalg.norm(inv, axis=0)
    frac = pos @ inv
    spread = np.ceil(frac.max(0) - frac.min(0)).astype(int) + 1 if n else np.zeros(3, int)
    rng = [range(-(int(np.ceil(r_reach / heights[d])) + spread[d]), int(np.ceil(r_reach / heights[d])) + spread[d] + 1)
           if pbc[d] else range(0, 1) for d in range(3)]
    out = []
    for S in itertools.product(*rng):
        d = pos[None, :, :] + (np.array(S, dtype=np.float64) @ cell)[None, None, :] - pos[:, None, :]
        r = np.sqrt((d * d).sum(-1))
        ii, jj = np.nonzero(r < r_reach)
        for i, j in zip(ii, jj):
            if i == j and S == (0, 0, 0):
                continue
            out.append((int(i), int(j), tuple(int(s) for s in S), float(r[i, j])))
    return out


def _enumerate(pos, types, cell, pbc, r_max, table):
    """The typed edge set, after asserting the precondition on the distances."""
    cands = _candidates(pos, cell, pbc, r_max + 1e-6)
    bounds = np.unique(np.concatenate([[r_max], np.asarray(table, dtype=np.float64).reshape(-1)]))
    if cands:
        r = np.array([c[3] for c in cands])
        gap = np.abs(r[:, None] - bounds[None, :]).min()
        assert gap > GAP, f"a candidate distance lies within {gap:.2e} A of a cutoff: choose another seed"
    table = np.asarray(table, dtype=np.float64)
    return {(i, j) + S for i, j, S, r in cands if r < r_max and r <= table[types[i], types[j]]}


def _as_set(edge_index, shift):
    ei = edge_index.cpu().numpy()
    sh = shift.cpu().numpy()
    assert np.array_equal(sh, np.round(sh))
    return {(int(a), int(b), int(s[0]), int(s[1]), int(s[2])) for a, b, s in zip(ei[0], ei[1], sh)}


def _table(T, kind, r_max, rng):
    if kind == "rmax":
        return np.full((T, T), r_max)
    if kind == "below":  # every entry below r_max
        t = rng.uniform(0.45, 0.85, size=(T, T)) * r_max
        return np.maximum(t, t.T)
    t = rng.uniform(0.5, 1.0, size=(T, T)) * r_max
    t[rng.integers(T), rng.integers(T)] = r_max
    if kind == "sym":
        t = np.maximum(t, t.T)
    else:
        assert kind == "asym"
        if T > 1 and np.array_equal(t, t.T):
            t[0, 1] *= 0.9
    return t


def _frame(kind, seed):
    """(pos, cell, pbc) of a random frame; atoms also outside the cell."""
    rng = np.random.default_rng(seed)
    if kind == "ortho":
        cell, pbc, n = np.diag([7.0, 8.0, 6.5]), (True, True, True), 60
    elif kind == "triclinic":
        cell, pbc, n = np.array([[7.0, 0.0, 0.0], [2.0, 6.5, 0.0], [1.0, -1.5, 7.5]]), (True, True, True), 60
    elif kind == "thin":  # thinner than the cutoff along two directions: several images of one atom
        cell, pbc, n = np.array([[2.2, 0.0, 0.0], [0.3, 2.6, 0.0], [0.0, 0.4, 9.0]]), (True, True, True), 12
    elif kind == "mixed":
        cell, pbc, n = np.array([[6.0, 0.0, 0.0], [1.0, 7.0, 0.0], [0.0, 0.0, 8.0]]), (True, False, True), 50
    else:
        assert kind == "nocell"
        return rng.uniform(0.0, 7.0, size=(40, 3)), None, (False, False, False)
    pos = rng.uniform(-0.3, 1.3, size=(n, 3)) @ cell
    return pos, cell, pbc


def _single(device, pos, types, cell, pbc, r_max, table):
    from nequip_amd.data._nl import _compute_neighborlist_single_frame

    kw = {}
    if table is not None:
        kw = dict(atom_types=torch.as_tensor(types, device=device), per_edge_type_cutoff=torch.as_tensor(table))
    return _compute_neighborlist_single_frame(
        torch.as_tensor(pos, dtype=torch.float64, device=device), r_max,
        cell=None if cell is None else torch.as_tensor(cell, dtype=torch.float64, device=device), pbc=tuple(pbc),
        return_rowptr=True, **kw)


def _mask_of(device, ei, sh, pos, types, cell, table):
    """The typed rule on an existing list, in float64 on the host (the distances are far from every boundary)."""
    ei_h, sh_h = ei.cpu().numpy(), sh.cpu().numpy()
    vec = pos[ei_h[1]] - pos[ei_h[0]] + (sh_h @ cell if cell is not None else 0.0)
    r = np.sqrt((vec * vec).sum(-1))
    return torch.as_tensor(r <= np.asarray(table)[types[ei_h[0]], types[ei_h[1]]], device=device)


def _rowptr_of(centres, n):
    return torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(centres.cpu(), minlength=n).cumsum(0)]).to(torch.int32)


CASES = [(frame, T, kind) for frame in ("ortho", "triclinic", "thin", "mixed", "nocell")
         for T, kind in ((1, "below"), (2, "sym"), (2, "asym"), (5, "sym"), (5, "asym"), (5, "below"))]


@pytest.mark.gpu
@pytest.mark.parametrize("frame,T,kind", CASES)
def test_typed_list_matches_enumeration_and_masked_full_list(device, frame, T, kind):
    """Checks 1 and 2 (single frame): the set equals the enumerator's; the arrays equal the masked untyped list bitwise."""
    r_max = 3.0
    seed = 1000 + 17 * CASES.index((frame, T, kind))
    pos, cell, pbc = _frame(frame, seed)
    rng = np.random.default_rng(seed + 1)
    types = rng.integers(T, size=len(pos))
    table = _table(T, kind, r_max, rng)
    want = _enumerate(pos, types, cell, pbc, r_max, table)
    ei, sh, rp = _single(device, pos, types, cell, pbc, r_max, table)
    assert ei.dtype == torch.int64 and rp.dtype == torch.int32
    assert _as_set(ei, sh) == want
    assert ei.shape[1] == len(want)
    full_ei, full_sh, _ = _single(device, pos, types, cell, pbc, r_max, None)
    assert ei.shape[1] < full_ei.shape[1]
    mask = _mask_of(device, full_ei, full_sh, pos, types, cell, table)
    assert torch.equal(ei, full_ei[:, mask]) and torch.equal(sh, full_sh[mask])
    assert torch.equal(rp.cpu(), _rowptr_of(ei[0], len(pos)))
    if kind == "sym" or T == 1:  # a symmetric table keeps the list symmetric
        assert {(j, i, -a, -b, -c) for i, j, a, b, c in want} == want


@pytest.mark.gpu
def test_water_box_counts(device):
    """The figures of the issue: water_box(n_side=8), r_max 4.5, 60 736 edges; 24 276 with the symmetric water table,
    28 226 with the asymmetric variant."""
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=8)
    assert list(names) == ["H", "O"]
    full, _, _ = _single(device, pos, types, cell, (True,) * 3, 4.5, None)
    assert full.shape[1] == 60736
    for table, count in (([[3.0, 3.5], [3.5, 4.5]], 24276), ([[3.0, 4.0], [3.5, 4.5]], 28226)):
        ei, sh, rp = _single(device, pos, types, cell, (True,) * 3, 4.5, np.array(table))
        assert ei.shape[1] == count and int(rp[-1]) == count


@pytest.mark.gpu
@pytest.mark.parametrize("frame", ["triclinic", "mixed", "nocell"])
def test_table_of_rmax_gives_the_untyped_list_bitwise(device, frame):
    """Check 3."""
    pos, cell, pbc = _frame(frame, 77)
    types = np.random.default_rng(5).integers(3, size=len(pos))
    _enumerate(pos, types, cell, pbc, 3.0, np.full((3, 3), 3.0))  # (the precondition)
    a = _single(device, pos, types, cell, pbc, 3.0, np.full((3, 3), 3.0))
    b = _single(device, pos, types, cell, pbc, 3.0, None)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _batch(device, kinds, T, seed):
    from nequip_amd.data import AtomicDataDict as K

    rng = np.random.default_rng(seed)
    frames = []
    for f, kind in enumerate(kinds):
        pos, cell, pbc = _frame(kind, seed + 31 * f)
        frames.append((pos, rng.integers(T, size=len(pos)), cell, pbc))
    data = {
        K.POSITIONS_KEY: torch.as_tensor(np.concatenate([f[0] for f in frames]), dtype=torch.float64, device=device),
        K.ATOM_TYPE_KEY: torch.as_tensor(np.concatenate([f[1] for f in frames]), device=device),
        K.BATCH_KEY: torch.repeat_interleave(torch.arange(len(frames)), torch.tensor([len(f[0]) for f in frames])).to(device),
        K.NUM_NODES_KEY: torch.tensor([len(f[0]) for f in frames], device=device),
        K.CELL_KEY: torch.as_tensor(np.stack([np.zeros((3, 3)) if f[2] is None else f[2] for f in frames]),
                                    dtype=torch.float64, device=device),
        K.PBC_KEY: torch.tensor([list(f[3]) for f in frames], device=device),
    }
    return frames, data


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sym", "asym"])
def test_batched_typed_list(device, kind, monkeypatch):
    """Check 2 (batched): == the masked untyped batched list == the concatenation of the typed single-frame lists, over
    frames of different periodicity; the topology hint is the pruned row pointer; NQA_NL_PER_FRAME=1 gives the same."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data._nl import compute_neighborlist_

    T, r_max = 3, 3.0
    frames, data = _batch(device, ["ortho", "nocell", "thin", "mixed", "triclinic"], T, 4242)
    table = _table(T, kind, r_max, np.random.default_rng(9))
    monkeypatch.delenv("NQA_NL_PER_FRAME", raising=False)
    from nequip_amd.nn._topology import topology_cache

    typed = compute_neighborlist_(dict(data), r_max, per_edge_type_cutoff=torch.as_tensor(table))
    ei, sh = typed[K.EDGE_INDEX_KEY], typed[K.EDGE_CELL_SHIFT_KEY]
    # the topology hint: this very edge_index, with the row pointer of the PRUNED list
    hint = topology_cache._hint
    assert hint[0]() is ei
    assert torch.equal(hint[3].cpu(), _rowptr_of(ei[0], data[K.POSITIONS_KEY].shape[0]))
    assert topology_cache._rowptr_hint(ei, ei[0], data[K.POSITIONS_KEY].shape[0]) is hint[3]
    full = compute_neighborlist_(dict(data), r_max)
    # concatenation of the single-frame typed lists (and, per frame, the enumerator)
    parts_ei, parts_sh, off, masks = [], [], 0, []
    for pos, types, cell, pbc in frames:
        want = _enumerate(pos, types, cell, pbc, r_max, table)
        e1, s1, _ = _single(device, pos, types, cell, pbc, r_max, table)
        assert _as_set(e1, s1) == want
        parts_ei.append(e1 + off)
        parts_sh.append(s1)
        off += len(pos)
    assert torch.equal(ei, torch.cat(parts_ei, dim=1)) and torch.equal(sh, torch.cat(parts_sh))
    # the masked untyped batched list
    fe, fs = full[K.EDGE_INDEX_KEY], full[K.EDGE_CELL_SHIFT_KEY]
    pos_all = np.concatenate([f[0] for f in frames])
    types_all = np.concatenate([f[1] for f in frames])
    fe_h, fs_h = fe.cpu().numpy(), fs.cpu().numpy()
    frame_of = np.repeat(np.arange(len(frames)), [len(f[0]) for f in frames])[fe_h[0]]
    cells = np.stack([np.zeros((3, 3)) if f[2] is None else f[2] for f in frames])
    vec = pos_all[fe_h[1]] - pos_all[fe_h[0]] + np.einsum("ni,nij->nj", fs_h, cells[frame_of])
    mask = torch.as_tensor(np.sqrt((vec * vec).sum(-1)) <= table[types_all[fe_h[0]], types_all[fe_h[1]]], device=device)
    assert ei.shape[1] < fe.shape[1]
    assert torch.equal(ei, fe[:, mask]) and torch.equal(sh, fs[mask])
    assert bool((ei[0][1:] >= ei[0][:-1]).all())
    monkeypatch.setenv("NQA_NL_PER_FRAME", "1")
    loop = compute_neighborlist_(dict(data), r_max, per_edge_type_cutoff=torch.as_tensor(table))
    assert torch.equal(loop[K.EDGE_INDEX_KEY], ei) and torch.equal(loop[K.EDGE_CELL_SHIFT_KEY], sh)


@pytest.mark.gpu
@pytest.mark.parametrize("batched", [False, True])
def test_neighbor_list_transform_builds_the_typed_device_list(device, batched):
    """``NeighborListTransform.forward`` == ``compute_neighborlist_`` with the same table (dict + type names, and a ready
    tensor), == the untyped list without a table; its hint is the pruned row pointer too."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data._nl import compute_neighborlist_
    from nequip_amd.data.transforms import NeighborListTransform
    from nequip_amd.nn._topology import topology_cache

    r_max, names = 3.0, ["A", "B"]
    pt = {"A": {"A": 2.0, "B": 2.6}, "B": {"A": 2.4}}
    table = np.array([[2.0, 2.6], [2.4, 3.0]])
    frames, data = _batch(device, ["triclinic", "mixed"] if batched else ["triclinic"], 2, 99)
    for f in frames:
        _enumerate(f[0], f[1], f[2], f[3], r_max, table)  # (the precondition)
    if not batched:
        data = {k: data[k] for k in (K.POSITIONS_KEY, K.ATOM_TYPE_KEY, K.CELL_KEY, K.PBC_KEY)}
    want = compute_neighborlist_(dict(data), r_max, per_edge_type_cutoff=torch.as_tensor(table))
    for t in (NeighborListTransform(r_max, per_edge_type_cutoff=pt, type_names=names),
              NeighborListTransform(r_max, per_edge_type_cutoff=torch.as_tensor(table))):
        out = t(dict(data))
        assert torch.equal(out[K.EDGE_INDEX_KEY], want[K.EDGE_INDEX_KEY])
        assert torch.equal(out[K.EDGE_CELL_SHIFT_KEY], want[K.EDGE_CELL_SHIFT_KEY])
        assert topology_cache._hint[0]() is out[K.EDGE_INDEX_KEY]
        assert torch.equal(topology_cache._hint[3].cpu(), _rowptr_of(out[K.EDGE_INDEX_KEY][0], data[K.POSITIONS_KEY].shape[0]))
    if not batched:
        assert _as_set(out[K.EDGE_INDEX_KEY], out[K.EDGE_CELL_SHIFT_KEY]) == _enumerate(*frames[0], r_max, table)
    plain, full = NeighborListTransform(r_max)(dict(data)), compute_neighborlist_(dict(data), r_max)
    assert torch.equal(plain[K.EDGE_INDEX_KEY], full[K.EDGE_INDEX_KEY])
    assert want[K.EDGE_INDEX_KEY].shape[1] < full[K.EDGE_INDEX_KEY].shape[1]
    no_types = {k: v for k, v in data.items() if k != K.ATOM_TYPE_KEY}
    with pytest.raises(KeyError, match="atom_types"):
        NeighborListTransform(r_max, per_edge_type_cutoff=pt, type_names=names)(no_types)


@pytest.mark.gpu
def test_batched_rowptr_is_the_pruned_csr(device):
    from nequip_amd.data._nl import _compute_neighborlist_batched

    frames, data = _batch(device, ["triclinic", "mixed"], 2, 99)
    table = np.array([[2.0, 2.6], [2.4, 3.0]])
    for f in frames:
        _enumerate(f[0], f[1], f[2], f[3], 3.0, table)
    ptr = torch.tensor([0, len(frames[0][0]), len(frames[0][0]) + len(frames[1][0])], device=device)
    ei, sh, rp = _compute_neighborlist_batched(data["pos"], 3.0, ptr, cell=data["cell"], pbc=data["pbc"],
                                               atom_types=data["atom_types"], per_edge_type_cutoff=torch.as_tensor(table))
    assert torch.equal(rp.cpu(), _rowptr_of(ei[0], data["pos"].shape[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["sym", "asym"])
def test_padded_typed_list(device, kind):
    """Check 4."""
    from nequip_amd.data._nl import PaddedNeighborList

    r_max, T = 3.0, 3
    pos, cell, pbc = _frame("triclinic", 314)
    rng = np.random.default_rng(15)
    types = rng.integers(T, size=len(pos))
    table = _table(T, kind, r_max, rng)
    sym = np.maximum(table, table.T)
    want = _enumerate(pos, types, cell, pbc, r_max, sym)
    _enumerate(pos, types, cell, pbc, r_max, table)  # (the precondition for the table as given)
    E = len(want)
    assert E % 2 == 0
    cap = E + 46
    cell_t = torch.as_tensor(cell, dtype=torch.float64, device=device)
    pos_t = torch.as_tensor(pos, dtype=torch.float64, device=device)
    nl = PaddedNeighborList(len(pos), r_max, cell_t, pbc, cap, shift_dtype=torch.float64,
                            atom_types=torch.as_tensor(types, device=device), per_edge_type_cutoff=torch.as_tensor(table))
    ei, sh, rp = nl.build(pos_t)
    fits, e_real = nl.status()
    assert fits and e_real == E and ei.shape[1] == cap == nl.edge_capacity and int(rp[-1]) == cap
    assert bool((ei[0][1:] >= ei[0][:-1]).all()) and torch.equal(rp.cpu(), _rowptr_of(ei[0], len(pos)))
    ei_h, sh_h = ei.cpu().numpy(), sh.cpu().numpy()
    vec = pos[ei_h[1]] - pos[ei_h[0]] + sh_h @ cell
    r = np.sqrt((vec * vec).sum(-1))
    pad = (ei_h[0] == ei_h[1]) & (r > r_max)
    assert int(pad.sum()) == cap - E
    real = ~pad
    assert _as_set(ei[:, torch.as_tensor(real)], sh[torch.as_tensor(real)]) == want
    # does not fit: padding only, status says so
    small = PaddedNeighborList(len(pos), r_max, cell_t, pbc, E - 10, shift_dtype=torch.float64,
                               atom_types=torch.as_tensor(types, device=device), per_edge_type_cutoff=torch.as_tensor(table))
    ei2, sh2, rp2 = small.build(pos_t)
    fits2, e2 = small.status()
    assert not fits2 and e2 == E and int(rp2[-1]) == E - 10
    assert torch.equal(ei2[0], ei2[1])


@pytest.mark.gpu
def test_bad_types_and_bad_tables_raise(device):
    """Check 5."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data._nl import PaddedNeighborList, compute_neighborlist_

    pos, cell, pbc = _frame("ortho", 3)
    types = np.random.default_rng(0).integers(2, size=len(pos))
    table = np.array([[2.0, 2.5], [2.5, 3.0]])
    bad_types = types.copy()
    bad_types[7] = 2
    neg_types = types.copy()
    neg_types[11] = -1
    for t in (bad_types, neg_types):
        with pytest.raises(ValueError, match="type index"):
            _single(device, pos, t, cell, pbc, 3.0, table)
        frames, data = _batch(device, ["ortho", "mixed"], 2, 8)
        data[K.ATOM_TYPE_KEY] = data[K.ATOM_TYPE_KEY].clone()
        data[K.ATOM_TYPE_KEY][5] = int(t[7]) if t is bad_types else -1
        with pytest.raises(ValueError, match="type index"):
            compute_neighborlist_(data, 3.0, per_edge_type_cutoff=torch.as_tensor(table))
        with pytest.raises(ValueError, match="type index"):
            PaddedNeighborList(len(pos), 3.0, torch.as_tensor(cell, device=device), pbc, 100,
                               atom_types=torch.as_tensor(t, device=device), per_edge_type_cutoff=torch.as_tensor(table))
    # the device is still healthy and the good input still works
    ei, sh, _ = _single(device, pos, types, cell, pbc, 3.0, table)
    assert _as_set(ei, sh) == _enumerate(pos, types, cell, pbc, 3.0, table)
    # host-side refusals, before any launch (CPU positions would be refused later: the table check comes first)
    cpu_pos = torch.as_tensor(pos)
    for bad in (np.array([[2.0, 3.5], [2.5, 3.0]]), np.array([[2.0, 0.0], [2.5, 3.0]]), np.array([[2.0, -1.0], [2.5, 3.0]])):
        with pytest.raises(ValueError, match="per-edge-type cutoffs"):
            compute_neighborlist_({K.POSITIONS_KEY: cpu_pos, K.ATOM_TYPE_KEY: torch.as_tensor(types)}, 3.0,
                                  per_edge_type_cutoff=torch.as_tensor(bad))
    with pytest.raises(KeyError, match="atom_types"):
        compute_neighborlist_({K.POSITIONS_KEY: torch.as_tensor(pos, device=device)}, 3.0,
                              per_edge_type_cutoff=torch.as_tensor(table))


def test_typed_symbols_are_exported_and_declared():
    """CPU: the typed entry points are declared in the header, bound in ``_lib`` and exported by the built library."""
    import os

    from nequip_amd import _lib

    names = ("nqa_neighbor_list_typed_workspace_bytes", "nqa_neighbor_list_count_typed", "nqa_neighbor_list_fill_typed",
             "nqa_neighbor_list_fill_padded_typed", "nqa_neighbor_list_batched_typed_workspace_bytes",
             "nqa_neighbor_list_batched_count_typed", "nqa_neighbor_list_batched_fill_typed")
    root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    header = open(os.path.join(root, "include", "nequip_amd.h")).read()
    for name in names:
        assert name in _lib.SIGNATURES, name
        assert f" {name}(" in header, name
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
    # the untyped workspace is what it was; the typed one extends it
    assert lib.nqa_neighbor_list_typed_workspace_bytes(100, 3) > lib.nqa_neighbor_list_workspace_bytes(100)
    assert lib.nqa_neighbor_list_batched_typed_workspace_bytes(100, 4, 3) > lib.nqa_neighbor_list_batched_workspace_bytes(100, 4)
    assert lib.nqa_neighbor_list_typed_workspace_bytes(100, 0) == -1


# (vgpr, sgpr, vgpr_spill, sgpr_spill, lds, scratch) of the untyped kernels as they were before the typed walk was added:
# the typed test is a template parameter of the shared walk, and the untyped instantiations must not have changed
UNTYPED_RESOURCES = {
    "nl_plan_kernel": (54, 46, 0, 0, 49304, 0), "nl_bin_kernel": (22, 31, 0, 0, 0, 0), "nl_scan_kernel": (28, 24, 0, 0, 128, 0),
    "nl_place_kernel": (7, 18, 0, 0, 0, 0), "nl_order_kernel": (19, 38, 0, 0, 0, 0), "nl_count_kernel": (22, 82, 0, 0, 0, 0),
    "nl_fill_kernel": (32, 94, 0, 0, 0, 0), "nl_pad_rowptr_kernel": (6, 40, 0, 0, 0, 0),
    "nl_fill_padded_kernel": (31, 106, 0, 2, 0, 0), "nl_batched_plan_kernel": (77, 78, 0, 0, 12456, 0),
    "nl_batched_bin_kernel": (40, 28, 0, 0, 0, 0), "nl_batched_count_kernel": (22, 84, 0, 0, 0, 0),
    "nl_batched_fill_kernel": (32, 94, 0, 0, 0, 0),
}


def test_untyped_kernels_kept_their_resources_and_typed_ones_do_not_spill_vgprs():
    import glob
    import os
    import sys

    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scripts"))
    import kernel_resources as kr

    objs = glob.glob(os.path.join(kr.BUILD, "neighbor_list.o"))
    if not objs or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("build objects / ROCm LLVM tools not present (run python -m nequip_amd.csrc.build)")
    ks = {n.split("(")[0].split("::")[-1]: r for n, r in kr.kernels_of(objs[0]).items()}
    keys = ("vgpr", "sgpr", "vgpr_spill", "sgpr_spill", "lds", "scratch")
    for name, want in UNTYPED_RESOURCES.items():
        assert tuple(ks[name][k] for k in keys) == want, (name, ks[name])
    typed = {n: r for n, r in ks.items() if n.startswith("nl_typed_")}
    assert sorted(typed) == ["nl_typed_count_kernel", "nl_typed_fill_kernel", "nl_typed_fill_padded_kernel", "nl_typed_prep_kernel"]
    for name, r in typed.items():
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert kr.waves_per_simd(r["vgpr"]) >= 4, (name, r)
