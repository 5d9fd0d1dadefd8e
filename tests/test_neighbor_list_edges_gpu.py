"""The device neighbour list (``nequip_amd/csrc/neighbor_list.hip``) on the cases of ``tests/neighbor_list_cases.py``: bins and
z-runs of more than 64 and 128 atoms, the 1024 cap and a long coarsening, thin, skewed and left-handed cells, atoms on cell and
bin faces, pairs at exactly r_max, coincident atoms -- in every form of the list (single frame, batched, typed, capacity
padded) against the float64 enumeration, and the consumers of such lists (``nqa_edge_pairs``, ``nqa_pair_owner_lists``) on
their crowded rows.

Forms and the cases they leave out (a form leaves a case out only where it cannot represent it):

* single frame, pairing: every case;
* batched: every case, but one batch per cutoff -- a batched call has ONE r_max for all its frames, and the cases' cutoffs are
  part of their properties -- in table order, with empty frames in front, in the middle and behind;
* typed: the cases the typed runs were specified for (``TYPED_NAMES``);
* padded: ``PADDED_NAMES``; ``blob_no_cell`` could not be added: the padding edges are lattice images, the form needs a cell.

Nothing here reads the reference tree."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import neighbor_list_cases as nc
from test_graphed_step import _pad_reference

pytestmark = pytest.mark.gpu

HEADER_NB, HEADER_REACH = 192, 204  # byte offsets in NLHeader: cell[9], inv[9], lo[3], width[3] (24 doubles), nb[3], reach[3]


def _tensors(case, device):
    pos = torch.tensor(case.pos, dtype=torch.float64, device=device).reshape(-1, 3)
    cell = None if case.cell is None else torch.tensor(case.cell, dtype=torch.float64, device=device)
    return pos, cell


@functools.lru_cache(maxsize=None)
def _run(name, typed, device):
    """One count + fill through ``_nl_count`` / ``_nl_fill`` with a workspace of our own:
    ``(edge_index, shift, rowptr, nb, reach)``; the first three stay on the device and are never written again."""
    from nequip_amd import _lib
    from nequip_amd.data import _nl

    case = nc.typed_case(name) if typed else nc.make_case(name)
    lib = _lib.load()
    N = case.num_atoms
    pos, cell = _tensors(case, device)
    pbc32 = torch.tensor([int(b) for b in case.pbc], dtype=torch.int32, device=device)
    T = nc.NUM_TYPES if typed else 0
    types = torch.tensor(case.types, dtype=torch.int64, device=device) if typed else None
    table = torch.tensor(case.table, dtype=torch.float64, device=device) if typed else None
    ws_bytes = _nl._nl_workspace_bytes(lib, N, T=T)
    ws = torch.zeros(ws_bytes, dtype=torch.uint8, device=device)
    aux = torch.full((N + 2,), -7, dtype=torch.int32, device=device)
    rowptr, status = aux[:N + 1], aux[N + 1:]
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    with torch.cuda.device(device):
        _nl._nl_count(lib, pos, cell, pbc32, case.r_max, N, ws, ws_bytes, rowptr, stream, types=types, table=table,
                      status=status if typed else None)
        E = int(rowptr[N].item())
        assert 0 <= E < 10 ** 6
        assert int(status.item()) == (0 if typed else -7)
        edge_index = torch.full((2, E), -1, dtype=torch.int64, device=device)
        shift = torch.full((E, 3), float("nan"), dtype=torch.float64, device=device)
        _nl._nl_fill(lib, ws, rowptr, N, E, edge_index, shift, stream, types=types, T=T)
    head = ws[:256].cpu().numpy().tobytes()
    nb = tuple(np.frombuffer(head, dtype=np.int32, count=3, offset=HEADER_NB).tolist())
    reach = tuple(np.frombuffer(head, dtype=np.int32, count=3, offset=HEADER_REACH).tolist())
    return edge_index, shift, rowptr.clone(), nb, reach


def _rows(edge_index, shift):
    """The list as int64 rows ``(i, j, Sx, Sy, Sz)`` in the order it came in; shifts have to be integer valued."""
    ei, sh = edge_index.cpu().numpy(), shift.cpu().numpy()
    assert np.array_equal(sh, np.round(sh)), "shifts must be integer valued"
    return np.concatenate([ei.T, sh.astype(np.int64)], 1).reshape(-1, 5)


def _assert_list(case, rows, rowptr, want):
    """``rows`` (in list order) is the list ``want`` (sorted reference rows) of ``case``, grouped by centre in ascending order."""
    N = case.num_atoms
    assert len(np.unique(rows, axis=0)) == len(rows), "duplicate edges"
    got = nc.sort_rows(rows)
    assert got.shape == want.shape, f"{len(got)} edges, the enumeration has {len(want)}"
    assert np.array_equal(got, want)
    assert np.all(np.diff(rows[:, 0]) >= 0), "centres must come in ascending order"
    assert np.array_equal(rowptr, np.concatenate([[0], np.cumsum(np.bincount(rows[:, 0], minlength=N))]))
    v = nc.edge_vectors(case, rows)
    assert np.all(np.sqrt((v * v).sum(1)) < case.r_max)


@pytest.mark.parametrize("name", nc.NAMES)
def test_single_frame_equals_the_enumeration(device, name):
    from nequip_amd.data._nl import _compute_neighborlist_single_frame

    case = nc.make_case(name)
    ei, sh, rowptr, nb, reach = _run(name, False, device)
    grid = nc.expected_grid(case, case.num_atoms + 8)
    deg = np.diff(rowptr.cpu().numpy())
    print(f"\n{name:<20} single  E {ei.shape[1]:>6}  degree <= {deg.max():>3}  nb {nb}  reach {reach}")
    assert nb == grid.nb and reach == grid.reach, "expected_grid no longer restates nl_size_grid"
    _assert_list(case, _rows(ei, sh), rowptr.cpu().numpy(), nc.enumerate_edges(case))
    pos, cell = _tensors(case, device)
    ei2, sh2, rowptr2 = _compute_neighborlist_single_frame(pos, case.r_max, cell=cell, pbc=case.pbc, return_rowptr=True)
    assert torch.equal(ei2, ei) and torch.equal(sh2, sh) and torch.equal(rowptr2, rowptr)


def _empty(periodic):
    return nc.Case("empty", np.zeros((0, 3)), np.eye(3) * 5.0 if periodic else None, (periodic,) * 3, 1.0)


def _batches():
    """One batch per cutoff, cases in table order, an empty frame in front, one in the middle, one (periodic) behind."""
    out = []
    for r_max in sorted({nc.make_case(n).r_max for n in nc.NAMES}):
        frames = [nc.make_case(n) for n in nc.NAMES if nc.make_case(n).r_max == r_max]
        mid = (len(frames) + 1) // 2
        out.append((r_max, [_empty(False)] + frames[:mid] + [_empty(False)] + frames[mid:] + [_empty(True)]))
    return out


def test_batches_hold_every_case():
    assert sorted(f.name for _, frames in _batches() for f in frames if f.num_atoms) == sorted(nc.NAMES)


@pytest.mark.parametrize("index", range(len(_batches())))
def test_batched_is_the_concatenation_of_the_single_frame_lists(device, index):
    from nequip_amd.data._nl import _compute_neighborlist_batched

    r_max, frames = _batches()[index]
    n = [f.num_atoms for f in frames]
    pos = torch.tensor(np.concatenate([f.pos.reshape(-1, 3) for f in frames]), dtype=torch.float64, device=device)
    cell = torch.tensor(np.stack([np.zeros((3, 3)) if f.cell is None else f.cell for f in frames]), dtype=torch.float64,
                        device=device)
    pbc = torch.tensor([f.pbc for f in frames], dtype=torch.bool, device=device)
    frame_ptr = torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int64, device=device)
    ei, sh, rowptr = _compute_neighborlist_batched(pos, r_max, frame_ptr, cell=cell, pbc=pbc)
    eis, shs, rps, off, eoff = [], [], [], 0, 0
    for f in frames:
        if f.num_atoms:
            e1, s1, r1, _, _ = _run(f.name, False, device)
            eis.append(e1 + off)
            shs.append(s1)
            rps.append(r1[:-1] + eoff)
            eoff += e1.shape[1]
            off += f.num_atoms
    rps.append(torch.tensor([eoff], dtype=torch.int32, device=device))
    print(f"\nbatch r_max {r_max}: {[f.name for f in frames]}  E {ei.shape[1]}")
    assert ei.dtype == torch.int64 and sh.dtype == torch.float64 and rowptr.dtype == torch.int32
    assert torch.equal(ei, torch.cat(eis, 1)) and torch.equal(sh, torch.cat(shs, 0)) and torch.equal(rowptr, torch.cat(rps))
    # ... and therefore the enumeration, frame by frame (checked on the batched arrays themselves)
    rows, rp, off = _rows(ei, sh), rowptr.cpu().numpy(), 0
    for f in frames:
        if f.num_atoms:
            mine = rows[rp[off]:rp[off + f.num_atoms]] - np.array([off, off, 0, 0, 0])
            _assert_list(f, mine, rp[off:off + f.num_atoms + 1] - rp[off], nc.enumerate_edges(f))
            off += f.num_atoms


@pytest.mark.parametrize("name", nc.TYPED_NAMES)
def test_typed_equals_the_filtered_enumeration_and_the_masked_untyped_list(device, name):
    """T = 3 with one type no atom has, an asymmetric table with the entries r_max, 0.6 r_max and 0.0 (``nc.typed_case``; the
    margin of the typed case, checked on the CPU, covers the table's cutoffs).  The entry 0.0 is below what ``CutoffTable``
    admits, which is why the table goes to the kernel directly."""
    case = nc.typed_case(name)
    ei, sh, rowptr, nb, reach = _run(name, True, device)
    ei_u, sh_u, _, nb_u, reach_u = _run(name, False, device)
    print(f"\n{name:<20} typed   E {ei.shape[1]:>6}  degree <= {np.diff(rowptr.cpu().numpy()).max():>3}  nb {nb}  reach {reach}")
    assert nb == nb_u and reach == reach_u  # the grid is the r_max grid
    want = nc.typed_edges(case)
    assert 0 < len(want) < len(nc.enumerate_edges(case))
    rows = _rows(ei, sh)
    assert len(np.unique(rows, axis=0)) == len(rows)
    assert np.array_equal(nc.sort_rows(rows), want)
    keep = torch.tensor(nc.typed_keep(case, _rows(ei_u, sh_u)), device=device)
    assert torch.equal(ei, ei_u[:, keep]) and torch.equal(sh, sh_u[keep])
    N = case.num_atoms
    assert np.array_equal(rowptr.cpu().numpy(), np.concatenate([[0], np.cumsum(np.bincount(rows[:, 0], minlength=N))]))


@pytest.mark.parametrize("fit", ["E+2", "E+2N+6", "too_small"])
@pytest.mark.parametrize("name", nc.PADDED_NAMES)
def test_padded_is_the_plain_list_plus_the_padding_rule(device, name, fit):
    from nequip_amd.data._nl import PaddedNeighborList

    case = nc.make_case(name)
    ei, sh, _, _, _ = _run(name, False, device)
    N, E = case.num_atoms, ei.shape[1]
    assert E % 2 == 0 and np.array_equal(nc.sort_rows(_rows(ei, sh)), nc.enumerate_edges(case))
    capacity = {"E+2": E + 2, "E+2N+6": E + 2 * N + 6, "too_small": E - 2}[fit]
    pos, cell = _tensors(case, device)
    nl = PaddedNeighborList(N, case.r_max, cell, case.pbc, capacity, shift_dtype=torch.float64)
    pei, psh, prp = nl.build(pos)
    fits, e_real = nl.status()
    pei, psh, prp = pei.cpu().numpy(), psh.cpu().numpy(), prp.cpu().numpy()
    print(f"\n{name:<20} padded  capacity {capacity:>6}  fits {fits}  E {e_real}")
    assert e_real == E and pei.shape == (2, capacity) and psh.shape == (capacity, 3)
    if fit == "too_small":
        assert not fits
        assert prp[0] == 0 and prp[-1] == capacity and np.all(np.diff(prp) >= 0)
        assert np.array_equal(pei[0], pei[1]) and np.array_equal(pei[0], np.repeat(np.arange(N), np.diff(prp)))  # in range
        assert np.all(np.linalg.norm(psh @ case.cell, axis=1) > case.r_max)
        return
    assert fits
    wi, ws, wr = _pad_reference(ei.cpu().numpy(), sh.cpu().numpy(), case.cell, case.pbc, case.r_max, N, capacity)
    assert np.array_equal(pei, wi) and np.array_equal(psh, ws) and np.array_equal(prp, wr)
    lengths = np.linalg.norm(case.pos[wi[1]] - case.pos[wi[0]] + ws @ case.cell, axis=1)
    assert int((lengths < case.r_max).sum()) == E


@functools.lru_cache(maxsize=None)
def _pairing(name, device):
    from nequip_amd.nn._topology import EdgeTopology

    case = nc.make_case(name)
    ei, sh, rowptr, _, _ = _run(name, False, device)
    topo = EdgeTopology(ei[0].contiguous(), ei[1].contiguous(), case.num_atoms, rowptr_dst=rowptr)  # (as the list hands it over)
    return topo, topo.pairing(sh if case.cell is not None else None)


@pytest.fixture
def paired_path(monkeypatch):
    import os

    if os.environ.get("NQA_FORCE_GENERIC", "") not in ("", "0"):
        pytest.skip("NQA_FORCE_GENERIC is read once per process by the library: no specialised kernels, no pairing")
    monkeypatch.delenv("NQA_NO_PAIRED", raising=False)


@pytest.mark.parametrize("name", nc.NAMES)
def test_lists_pair_up_as_a_reverse_edge_matching(device, name, paired_path):
    """Both directions of a pair see the same squared length (the comment in ``nl_walk``): every list here, crowded rows and
    r == 0 edges included, has to pair up (the assertions of ``test_pairing_is_a_reverse_edge_matching``)."""
    ei, sh, _, _, _ = _run(name, False, device)
    topo, pr = _pairing(name, device)
    assert pr is not None, "the list does not pair up"
    E = ei.shape[1]
    P = E // 2
    rows, rep = pr.rows.cpu().numpy(), pr.rep_edge.cpu().numpy()
    dst, src, shn = ei[0].cpu().numpy(), ei[1].cpu().numpy(), sh.cpu().numpy()
    assert sorted(rows.tolist()) == list(range(2 * P))
    other = np.empty(P, dtype=np.int64)
    other[rows[rows >= P] - P] = np.nonzero(rows >= P)[0]
    assert np.array_equal(rows[rep], np.arange(P))
    assert np.array_equal(dst[rep], src[other]) and np.array_equal(src[rep], dst[other])
    assert np.array_equal(shn[rep], -shn[other])
    eid_d = topo.by_dst[1][:E].cpu().numpy()
    assert np.array_equal(pr.slots_dst.cpu().numpy(), rows[eid_d])
    eid_s = topo.by_src[1][:E].cpu().numpy()
    assert np.array_equal(pr.slots_src.cpu().numpy(), rows[eid_s])


@pytest.mark.parametrize("name", nc.NAMES)
def test_owner_lists_of_these_lists_match_the_host_statement(device, name, paired_path):
    """The assertions of ``test_owner_lists_from_the_csr_match_the_host_statement_of_the_rule`` on rows of up to 200 entries."""
    from nequip_amd.nn._topology import build_owner_csr

    case = nc.make_case(name)
    ei, _, _, _, _ = _run(name, False, device)
    topo, pr = _pairing(name, device)
    assert pr is not None, "the list does not pair up"
    N, P = case.num_atoms, pr.num_pairs
    got = [t.cpu().long() for t in pr.owner_csr]
    ref = [t.cpu().long() for t in build_owner_csr(topo._dst, topo._src, pr.rows, P, N)]
    orow, oth, prow, ein, eout, trow, tslot = got
    assert torch.equal(orow, ref[0]) and torch.equal(trow, ref[5])
    dst, src = ei[0].cpu(), ei[1].cpu()
    rows = pr.rows.cpu().long()
    assert sorted(prow[:P].tolist()) == list(range(P)) and sorted(tslot[:P].tolist()) == list(range(P))
    owner = torch.repeat_interleave(torch.arange(N), orow[1:] - orow[:-1])
    assert torch.equal(dst[ein[:P]], owner) and torch.equal(src[ein[:P]], oth[:P])
    assert torch.equal(dst[eout[:P]], oth[:P]) and torch.equal(src[eout[:P]], owner)
    assert torch.equal(rows[ein[:P]] % P, prow[:P]) and torch.equal(rows[eout[:P]] % P, prow[:P])
    assert not torch.equal(rows[ein[:P]], rows[eout[:P]])
    other_of_slot = torch.repeat_interleave(torch.arange(N), trow[1:] - trow[:-1])
    assert torch.equal(oth[:P][tslot[:P]], other_of_slot)

    def triples(lst):
        o = torch.repeat_interleave(torch.arange(N), lst[0][1:] - lst[0][:-1])
        return sorted(zip(o.tolist(), lst[2][:P].tolist(), lst[3][:P].tolist(), lst[4][:P].tolist()))

    assert triples(got) == triples(ref)


def test_some_list_has_a_row_of_more_than_128_entries(device):
    """The partner scan reads 48 entries of a CSR row per trip, the owner kernels 64 per ballot: rows beyond 128 entries take both
    to their third trip."""
    longest = {n: int(np.diff(_run(n, False, device)[2].cpu().numpy()).max()) for n in nc.NAMES}
    assert sum(v > 128 for v in longest.values()) >= 1, longest
