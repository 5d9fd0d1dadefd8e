"""Cases and restatements of the geometry kernels (``csrc/edge_vectors.hip``, ``csrc/csr.hip``, ``nqa_csr_from_pairs``),
shared by ``tests/test_geometry_cases.py`` (CPU: the restatements against the ATen formulation) and
``tests/test_geometry_kernels_gpu.py`` (GPU launches).  A plain module: no fixtures, no pytest import, no GPU.

Convention (``include/nequip_amd.h``): ``edge_index[0]`` = centre atom (dst), ``edge_index[1]`` = neighbour (src),
``vec_e = pos[src] - pos[dst] + shift_e @ cell[frame(dst)]``.

**Grid cases.**  Every value is an int64 array times a fixed power of two: positions on a 2^-8 grid in [-16, 16], gradients on
a 2^-8 grid in [-4, 4], integer shifts in [-2, 2], cells on a 2^-4 grid in [-16, 16].  The kernels only subtract, multiply
and add float64, so on these inputs every intermediate is exactly representable: the result does not depend on the summation
order or on FMA contraction, and a correct kernel reproduces the int64 restatement below bit for bit (``bit_budget`` checks
that no restatement leaves 2^52).  The only rounded quantity is ``stress = sym / |det cell|``: one division of two exact
operands, compared at ``STRESS_RTOL``.

**Random cases.**  ``randn`` values on the topology of a grid case, compared with a ``numpy.longdouble`` accumulation at the
derived bound ``|err| <= (terms + 2) * 2^-53 * sum|term|`` (``check_bound``): a float64 sum of ``terms`` addends, each the
rounded product of inputs, errs by at most ``((1 + u)^terms - 1) * sum|term|`` in any order, u = 2^-53; the two spare units
cover the final scale, the second-order part of ``(1 + u)^terms`` (terms <= 40 000: terms^2 u^2 / 2 < 1e-7 u) and the
reference's own longdouble error (terms * 2^-64 * sum|term| <= 0.02 u * sum|term|).
"""

import dataclasses
import os
import sys
from typing import Optional

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

POS_BITS, G_BITS, CELL_BITS = 8, 8, 4  # value = integer * 2^-bits
POS_MAX, G_MAX, SHIFT_MAX, CELL_MAX = 16 << POS_BITS, 4 << G_BITS, 2, 16 << CELL_BITS
VEC_BITS = POS_BITS  # edge vectors: pos difference + (shift @ cell) << (POS_BITS - CELL_BITS)
ROWS_SHIFT_BITS = G_BITS  # per-atom rows with left = shift:   shift_a * g_b
ROWS_VEC_BITS = VEC_BITS + G_BITS  # per-atom rows with left = edge_vec: vec_a * g_b
DET_BITS = 3 * CELL_BITS
STRESS_RTOL = 4 * 2.0 ** -52
U = 2.0 ** -53

DEGREES = (0, 1, 63, 64, 65, 129, 200)  # edges per atom as centre; as neighbour: the reverse
GRID_CASES = ("degrees", "one_atom_e0", "one_atom_e5", "no_edges", "block_edges_255", "block_edges_256", "block_edges_257",
              "frames_interleaved", "one_frame_large_1023", "one_frame_large_1024", "one_frame_large_1025", "symmetric_box")
RANDOM_CASES = ("degrees", "frames_interleaved")


@dataclasses.dataclass
class Case:
    """One input set.  Grid cases carry the integers (``*_i``); ``pos / shift / cell / g`` are always float64."""

    name: str
    pos: torch.Tensor  # [N, 3]
    edge_index: torch.Tensor  # [2, E] int64
    shift: torch.Tensor  # [E, 3]
    cell: Optional[torch.Tensor]  # None, [3, 3], [1, 3, 3] or [B, 3, 3]
    batch: Optional[torch.Tensor]  # None or [N] int64
    g: torch.Tensor  # [E, 3]
    pos_i: Optional[torch.Tensor] = None
    shift_i: Optional[torch.Tensor] = None
    cell_i: Optional[torch.Tensor] = None
    g_i: Optional[torch.Tensor] = None

    @property
    def num_nodes(self) -> int:
        return int(self.pos.shape[0])

    @property
    def num_edges(self) -> int:
        return int(self.edge_index.shape[1])

    @property
    def num_frames(self) -> int:
        return 1 if self.cell is None else int(self.cell.reshape(-1, 3, 3).shape[0])

    @property
    def frame_of_atom(self) -> torch.Tensor:
        return self.batch if self.batch is not None else torch.zeros(self.num_nodes, dtype=torch.int64)

    def permuted(self, perm: torch.Tensor) -> "Case":
        """The same graph with its edges listed in another order."""
        pick = lambda t: None if t is None else t[perm].contiguous()  # noqa: E731
        return dataclasses.replace(self, edge_index=self.edge_index[:, perm].contiguous(), shift=pick(self.shift),
                                   g=pick(self.g), shift_i=pick(self.shift_i), g_i=pick(self.g_i))


def exact(x_i: torch.Tensor, bits: int) -> torch.Tensor:
    """int64 * 2^-bits as float64 (exact below 2^53)."""
    assert x_i.dtype == torch.int64
    assert x_i.numel() == 0 or int(x_i.abs().max()) < 2 ** 53
    return x_i.to(torch.float64) * (2.0 ** -bits)


def _grid_case(name, pos_i, edge_index, shift_i, cell_i, batch, g_i) -> Case:
    return Case(name, exact(pos_i, POS_BITS), edge_index.contiguous(), exact(shift_i, 0),
                None if cell_i is None else exact(cell_i, CELL_BITS), batch, exact(g_i, G_BITS),
                pos_i=pos_i, shift_i=shift_i, cell_i=cell_i, g_i=g_i)


def _rint(gen, lim, shape):
    return torch.randint(-lim, lim + 1, shape, generator=gen, dtype=torch.int64)


def det_int(cell_i: torch.Tensor) -> torch.Tensor:
    """Determinants of [..., 3, 3] int64 cells (scale 2^-DET_BITS)."""
    c = cell_i.reshape(-1, 9)
    return (c[:, 0] * (c[:, 4] * c[:, 8] - c[:, 5] * c[:, 7]) - c[:, 1] * (c[:, 3] * c[:, 8] - c[:, 5] * c[:, 6])
            + c[:, 2] * (c[:, 3] * c[:, 7] - c[:, 4] * c[:, 6]))


def _cell(gen, handed: int = 0, triclinic: bool = False) -> torch.Tensor:
    """A random [3, 3] grid cell with a volume of at least 1 (handed: +1 / -1 fixes the sign of the determinant)."""
    while True:
        c = _rint(gen, CELL_MAX, (3, 3))
        d = int(det_int(c)[0])
        if abs(d) < 2 ** DET_BITS or (handed and (d > 0) != (handed > 0)) or (triclinic and int((c == 0).sum()) > 0):
            continue
        return c


def _random_edges(gen, N: int, E: int):
    return torch.randint(0, N, (2, E), generator=gen, dtype=torch.int64)


def _degrees_topology(gen):
    """N = 7 directed list: as-centre counts DEGREES, as-neighbour counts reversed, self-loops with a shift, duplicates."""
    n = len(DEGREES)
    dst = torch.repeat_interleave(torch.arange(n), torch.tensor(DEGREES))
    src = torch.repeat_interleave(torch.arange(n), torch.tensor(DEGREES[::-1]))
    E = int(dst.numel())
    src = src[torch.randperm(E, generator=gen)]
    shift = _rint(gen, SHIFT_MAX, (E, 3))
    loops = (dst == src) & (shift == 0).all(1)
    shift[loops, 0] = 1  # an atom sees its own IMAGE: a self-loop has a non-zero shift
    # exact duplicates: the first two edges of the 200-edge row that share a neighbour get the same shift
    row = torch.nonzero(dst == n - 1).flatten()
    seen = {}
    for e in row.tolist():
        j = int(src[e])
        if j in seen:
            shift[e] = shift[seen[j]]
            break
        seen[j] = e
    perm = torch.randperm(E, generator=gen)  # an unsorted list
    return torch.stack([dst[perm], src[perm]]), shift[perm].contiguous()


def make_case(name: str, seed: int = 0) -> Case:
    """The named grid case (GRID_CASES)."""
    gen = torch.Generator().manual_seed(1000 + seed)
    cell_i, batch = None, None
    if name == "degrees":
        edge_index, shift_i = _degrees_topology(gen)
        N = len(DEGREES)
        cell_i = _cell(gen, triclinic=True)  # [3, 3]
    elif name in ("one_atom_e0", "one_atom_e5"):
        N, E = 1, (0 if name.endswith("e0") else 5)
        edge_index = torch.zeros((2, E), dtype=torch.int64)
        shift_i = _rint(gen, SHIFT_MAX, (E, 3))
        shift_i[(shift_i == 0).all(1), 2] = -1
        cell_i = _cell(gen).view(1, 3, 3)
        batch = torch.zeros(1, dtype=torch.int64)
    elif name == "no_edges":
        N = 9
        edge_index = torch.zeros((2, 0), dtype=torch.int64)
        shift_i = torch.zeros((0, 3), dtype=torch.int64)
        cell_i = _cell(gen).view(1, 3, 3)
    elif name.startswith("block_edges_"):
        N, E = 33, int(name.rsplit("_", 1)[1])
        edge_index = _random_edges(gen, N, E)
        shift_i = _rint(gen, SHIFT_MAX, (E, 3))
        if E == 255:
            cell_i = _cell(gen)  # [3, 3]
        elif E == 257:
            cell_i, batch = _cell(gen).view(1, 3, 3), torch.zeros(N, dtype=torch.int64)
        # (E == 256: no cell, an open system; the forward ignores the shifts, the adjoint still takes them as left factor)
    elif name == "frames_interleaved":
        N, E, B = 2100, 20000, 4
        batch = torch.tensor([0, 1, 3])[torch.randint(0, 3, (N,), generator=gen)]  # frame 2 stays empty
        for f in (0, 1, 3):  # every frame owns atoms on both sides of 1024 and of 2048
            own = torch.nonzero(batch == f).flatten()
            assert int(own.min()) < 1024 and int(((own > 1024) & (own < 2048)).sum()) > 0 and int(own.max()) > 2048
        edge_index = _random_edges(gen, N, E)  # (directed, across frames too: the frame of an edge is its CENTRE's)
        shift_i = _rint(gen, SHIFT_MAX, (E, 3))
        cell_i = torch.stack([_cell(gen, handed=+1), _cell(gen, handed=-1), _cell(gen), _cell(gen, handed=+1, triclinic=True)])
    elif name.startswith("one_frame_large_"):
        N, E = int(name.rsplit("_", 1)[1]), 4000
        edge_index = _random_edges(gen, N, E)
        edge_index[0, :3] = N - 1  # the last atom is a centre
        shift_i = _rint(gen, SHIFT_MAX, (E, 3))
        cell_i = _cell(gen)
    elif name == "symmetric_box":
        from nequip_amd.utils import synthetic as syn

        pos, types, cell, _ = syn.water_box(n_side=2, seed=seed)
        data = syn.make_data(pos, types, 4.5, cell)
        edge_index = data["edge_index"]
        shift_i = data["edge_cell_shift"].round().to(torch.int64)
        assert int(shift_i.abs().max()) <= SHIFT_MAX
        pos_i = (data["pos"] * 2 ** POS_BITS).round().to(torch.int64)
        cell_i = (data["cell"] * 2 ** CELL_BITS).round().to(torch.int64).view(1, 3, 3)
        g_i = _rint(gen, G_MAX, (edge_index.shape[1], 3))
        return _grid_case(name, pos_i, edge_index, shift_i, cell_i, None, g_i)
    else:
        raise KeyError(name)
    pos_i = _rint(gen, POS_MAX, (N, 3))
    g_i = _rint(gen, G_MAX, (edge_index.shape[1], 3))
    return _grid_case(name, pos_i, edge_index, shift_i, cell_i, batch, g_i)


def random_case(name: str, seed: int = 0) -> Case:
    """``randn`` values (positions, shifts, cells, gradients) on the topology of a grid case: nothing is exactly
    representable in fewer than 53 bits.  The cells are 8 * identity + randn: volumes far from zero."""
    base = make_case(name, seed)
    gen = torch.Generator().manual_seed(2000 + seed)
    rn = lambda shape: torch.randn(shape, generator=gen, dtype=torch.float64)  # noqa: E731
    cell = None if base.cell is None else 8.0 * torch.eye(3, dtype=torch.float64).expand(base.cell.shape) + rn(base.cell.shape)
    if cell is not None and base.num_frames > 1:
        cell[1, 0] = -cell[1, 0]  # keep the left-handed frame
    return Case(base.name + "_randn", 4.0 * rn(base.pos.shape), base.edge_index, rn(base.shift.shape), cell, base.batch,
                rn(base.g.shape))


# ---- integer restatements (int64 throughout; `exact` is the only conversion) -------------------------------------------


def vec_int(case: Case) -> torch.Tensor:
    """Edge vectors [E, 3] at scale 2^-VEC_BITS."""
    dst, src = case.edge_index
    v = case.pos_i[src] - case.pos_i[dst]
    if case.cell_i is not None:
        c = case.cell_i.reshape(-1, 3, 3)[case.frame_of_atom[dst]]  # [E, 3, 3]
        v = v + (case.shift_i[:, :, None] * c).sum(1) * 2 ** (POS_BITS - CELL_BITS)
    return v


def adjoint_int(case: Case, left_i: Optional[torch.Tensor]):
    """``g_pos[n] = sum_{src(e)=n} g_e - sum_{dst(e)=n} g_e`` (scale 2^-G_BITS) and, with a left factor,
    ``rows[n, 3a+b] = sum_{dst(e)=n} left_ea g_eb`` (scale of left * 2^-G_BITS)."""
    dst, src = case.edge_index
    N = case.num_nodes
    g_pos = torch.zeros((N, 3), dtype=torch.int64).index_add_(0, src, case.g_i).index_add_(0, dst, -case.g_i)
    rows = None
    if left_i is not None:
        outer = (left_i[:, :, None] * case.g_i[:, None, :]).reshape(-1, 9)
        rows = torch.zeros((N, 9), dtype=torch.int64).index_add_(0, dst, outer)
    return g_pos, rows


def frame_sum_int(rows_i: torch.Tensor, batch: Optional[torch.Tensor], num_frames: int) -> torch.Tensor:
    f = batch if batch is not None else torch.zeros(rows_i.shape[0], dtype=torch.int64)
    return torch.zeros((num_frames,) + tuple(rows_i.shape[1:]), dtype=torch.int64).index_add_(0, f, rows_i)


def sym2_int(m_i: torch.Tensor) -> torch.Tensor:
    """``m + m^T`` of [B, 9] sums as [B, 3, 3]: TWICE the symmetrised sum, i.e. ``sym`` with one more bit in the scale."""
    m = m_i.view(-1, 3, 3)
    return m + m.transpose(1, 2)


def stress_from(sym: torch.Tensor, case: Case) -> torch.Tensor:
    """float64 ``sym / |det cell|`` from the exact ``sym`` and the exact determinant: one rounding."""
    vol = exact(det_int(case.cell_i).abs(), DET_BITS)
    return sym / vol.view(-1, 1, 1)


def grid_reference(case: Case) -> dict:
    """Everything the tests compare, as exact float64 (and the largest integer met, for the bit budget)."""
    v_i = vec_int(case)
    g_pos_i, rows_s_i = adjoint_int(case, case.shift_i)
    _, rows_v_i = adjoint_int(case, v_i)
    B = case.num_frames
    g_cell_i = frame_sum_int(rows_s_i, case.batch, B)
    sym2_i = sym2_int(frame_sum_int(rows_v_i, case.batch, B))
    peak = max([int(t.abs().max()) for t in (v_i, g_pos_i, rows_s_i, rows_v_i, g_cell_i, sym2_i) if t.numel()] + [0])
    ref = {"vec": exact(v_i, VEC_BITS), "g_pos": exact(g_pos_i, G_BITS), "rows_shift": exact(rows_s_i, ROWS_SHIFT_BITS),
           "rows_vec": exact(rows_v_i, ROWS_VEC_BITS), "g_cell": exact(g_cell_i, ROWS_SHIFT_BITS).view(B, 3, 3),
           "sym": exact(sym2_i, ROWS_VEC_BITS + 1), "peak": peak}
    ref["virial"] = -ref["sym"]
    if case.cell_i is not None:
        peak = max(peak, int(det_int(case.cell_i).abs().max()))
        ref["peak"] = peak
        ref["stress"] = stress_from(ref["sym"], case)
    return ref


def sym_of_rows(rows_i: torch.Tensor, bits: int, batch: Optional[torch.Tensor], num_frames: int) -> torch.Tensor:
    """Exact float64 ``sym`` [B, 3, 3] of integer per-atom rows at scale 2^-bits."""
    return exact(sym2_int(frame_sum_int(rows_i, batch, num_frames)), bits + 1)


def host_csr(key: torch.Tensor, other: torch.Tensor, num_nodes: int):
    """What ``nqa_csr_build`` promises: the count prefix, the stable order, the other side in that order (int32)."""
    order = torch.argsort(key, stable=True)
    rowptr = torch.zeros(num_nodes + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(key, minlength=num_nodes), 0)
    return rowptr.to(torch.int32), order.to(torch.int32), other[order].to(torch.int32)


# ---- longdouble restatements and the derived bound (random cases) ------------------------------------------------------


def _ld(t) -> np.ndarray:
    return np.asarray(t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t).astype(np.longdouble)


@dataclasses.dataclass
class Bounded:
    """A longdouble reference with, per element, the number of addends and their magnitude sum."""

    ref: np.ndarray
    terms: np.ndarray
    mag: np.ndarray

    @property
    def bound(self) -> np.ndarray:
        return (self.terms.astype(np.longdouble) + 2) * np.longdouble(U) * self.mag


def _scatter(index: np.ndarray, terms: np.ndarray, n: int) -> Bounded:
    """Sum rows of ``terms`` [E, K] into ``n`` slots; every row is one addend."""
    K = terms.shape[1]
    ref, mag = np.zeros((n, K), np.longdouble), np.zeros((n, K), np.longdouble)
    np.add.at(ref, index, terms)
    np.add.at(mag, index, np.abs(terms))
    cnt = np.bincount(index, minlength=n).astype(np.int64)[:, None].repeat(K, 1)
    return Bounded(ref, cnt, mag)


def ld_vec(case: Case) -> Bounded:
    dst, src = case.edge_index.numpy()
    pos = _ld(case.pos)
    ref, mag = pos[src] - pos[dst], np.abs(pos[src]) + np.abs(pos[dst])
    terms = np.full(ref.shape, 2, np.int64)
    if case.cell is not None:
        c = _ld(case.cell).reshape(-1, 3, 3)[case.frame_of_atom.numpy()[dst]]
        prod = _ld(case.shift)[:, :, None] * c  # [E, a, b]
        ref, mag, terms = ref + prod.sum(1), mag + np.abs(prod).sum(1), terms + 3
    return Bounded(ref, terms, mag)


def ld_adjoint(case: Case, left: Optional[torch.Tensor]):
    """(g_pos for sign = +1, rows) of the adjoint."""
    dst, src = case.edge_index.numpy()
    g, N = _ld(case.g), case.num_nodes
    a, b = _scatter(src, g, N), _scatter(dst, -g, N)
    g_pos = Bounded(a.ref + b.ref, a.terms + b.terms, a.mag + b.mag)
    rows = None
    if left is not None:
        rows = _scatter(dst, (_ld(left)[:, :, None] * g[:, None, :]).reshape(-1, 9), N)
    return g_pos, rows


def ld_given_rows(rows: torch.Tensor) -> Bounded:
    """Rows handed to a kernel as inputs: one exact addend each."""
    r = _ld(rows)
    return Bounded(r, np.ones(r.shape, np.int64), np.abs(r))


def ld_frame_reduce(rows: Bounded, batch: Optional[torch.Tensor], num_frames: int) -> Bounded:
    f = batch.numpy() if batch is not None else np.zeros(rows.ref.shape[0], np.int64)
    K = rows.ref.shape[1]
    ref, mag = np.zeros((num_frames, K), np.longdouble), np.zeros((num_frames, K), np.longdouble)
    terms = np.zeros((num_frames, K), np.int64)
    np.add.at(ref, f, rows.ref)
    np.add.at(mag, f, rows.mag)
    np.add.at(terms, f, rows.terms)
    return Bounded(ref, terms, mag)


def ld_sym(m: Bounded) -> Bounded:
    t = lambda x: x.reshape(-1, 3, 3).transpose(0, 2, 1)  # noqa: E731
    r3 = lambda x: x.reshape(-1, 3, 3)  # noqa: E731
    return Bounded(0.5 * (r3(m.ref) + t(m.ref)), r3(m.terms) + t(m.terms), 0.5 * (r3(m.mag) + t(m.mag)))


def ld_stress(sym: Bounded, cell: torch.Tensor):
    """``sym / |det cell|`` and its bound.  The determinant is a float64 sum of six triple products (two roundings each, up
    to five additions): relative error ``rel_vol <= 9 u D / vol`` with D the magnitude sum of the six products; the division
    adds one rounding.  To first order ``|err| <= (sym_bound + |sym| (rel_vol + u)) / vol``; the factor ``1 + 2 rel_vol``
    covers the higher orders."""
    c = _ld(cell).reshape(-1, 9)
    trip = np.stack([c[:, 0] * c[:, 4] * c[:, 8], -c[:, 0] * c[:, 5] * c[:, 7], -c[:, 1] * c[:, 3] * c[:, 8],
                     c[:, 1] * c[:, 5] * c[:, 6], c[:, 2] * c[:, 3] * c[:, 7], -c[:, 2] * c[:, 4] * c[:, 6]], 1)
    vol = np.abs(trip.sum(1))[:, None, None]
    rel_vol = (9 * np.longdouble(U) * np.abs(trip).sum(1))[:, None, None] / vol
    ref = sym.ref / vol
    bound = (sym.bound + np.abs(sym.ref) * (rel_vol + np.longdouble(U))) / vol * (1 + 2 * rel_vol)
    return ref, bound


def check_bound(got, ref: np.ndarray, bound: np.ndarray, what: str) -> float:
    """Assert ``|got - ref| <= bound`` element by element; returns the largest ``err / bound`` (0 where both vanish)."""
    assert np.finfo(np.longdouble).eps <= 2.0 ** -63, "numpy.longdouble is not an extended type on this machine"
    got = _ld(got).reshape(ref.shape)
    assert np.all(np.isfinite(got)), f"{what}: non-finite values"
    err = np.abs(got - ref)
    bad = err > bound
    worst = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)), initial=0.0))
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} elements beyond the derived bound, worst err / bound = "
                           f"{worst:.3g} at {np.unravel_index(int(np.argmax(err - bound)), err.shape)}")
    return worst
