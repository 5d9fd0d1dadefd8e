"""Cases and reference of the device neighbour list (``nequip_amd/csrc/neighbor_list.hip``) at crowded bins, thin cells and
faces, shared by ``tests/test_neighbor_list_cases.py`` (CPU: the properties of the cases and of the reference itself) and
``tests/test_neighbor_list_edges_gpu.py`` (GPU launches).  A plain module: no fixtures, no pytest import, no GPU, and no code
shared with ``nequip_amd``.

Convention (``nequip_amd/data/_nl.py``): the edge ``(i, j, S)`` exists iff ``|pos_j + S @ cell - pos_i| < r_max`` (strict),
``i == j`` with ``S == 0`` excluded; a typed list keeps it iff also ``r <= table[type_i][type_j]``.

**Reference.**  ``enumerate_edges`` walks the lattice images in plain float64 Cartesian arithmetic.  The kernel forms the same
vector through wrapped fractional coordinates, so the two may disagree on a pair whose length is within rounding of a cutoff:
``margin`` (``numpy.longdouble``) is the smallest relative distance of any pair length to any cutoff of the case and has to be
``>= MARGIN_MIN = 1e-9``.  The kernel's error is largest for ``clipped_1024`` (|pos| <= 5000 A): about 10 ulp * 5000 A ~ 1e-11 A,
3e-12 relative to r_max, so 1e-9 leaves more than two orders of room.  ``exact_grid`` is the exception on purpose: its values
are dyadic (0.5 A lattice, 8 A cube, r_max 2), every quantity of the kernel and of the reference is exact, and pairs at exactly
r_max have to be absent.

**Grid.**  ``expected_grid`` restates ``nl_size_grid`` and ``nl_bin_atom``; the GPU test compares ``nb`` and ``reach`` with the
header the kernel wrote, so a drift of the restatement shows.

Figures of the cases (``pytest -s tests/test_neighbor_list_cases.py`` prints this table; E and degrees from the reference, the
grid for a bin budget of N + 8, ``run`` = most candidates in one z-run of one image, ``bin`` = most atoms in one bin)::

    case                   N       E   degree   margin     nb          reach     halvings  bin   run
    crowded_single_bin   150   16752   95..125  4.2e-05  (1, 1, 1)    (1, 1, 1)      0     150   150
    dense_640            640   36458   41..80   4.9e-05  (3, 3, 3)    (1, 1, 1)      0      32    84
    blob_no_cell         200   39574  176..199  4.9e-05  (1, 1, 1)    (0, 0, 0)      0     200   200
    slab_crowded         120   10442   73..99   1.5e-05  (2, 2, 1)    (1, 1, 0)      0      35    35
    cluster_on_corner    130   10330   25..118  7.7e-06  (5, 5, 5)    (1, 1, 1)      3      21    21
    clipped_1024           7       6    0..1    3.8e-01  (2, 2, 2)    (1, 1, 1)     27       2     2
    thin_x                80   10264  104..156  5.3e-05  (1, 2, 2)    (3, 1, 1)      0      25    41
    skewed                60   10720  162..200  4.8e-05  (1, 1, 1)    (2, 2, 2)      0      60    60
    left_handed           50    1336   15..35   8.1e-04  (1, 1, 2)    (1, 1, 1)      0      25    50
    one_atom_images        1      60   60..60   2.6e-03  (1, 1, 1)    (3, 3, 3)      0       1     1
    coincident            42     616    7..21   8.0e-04  (2, 2, 2)    (1, 1, 1)      0      10    13
    exact_grid           300    5374    9..29   0.0e+00  (4, 4, 4)    (1, 1, 1)      0       9    24
    minus_epsilon        150   16734   95..126  4.2e-05  (1, 1, 1)    (1, 1, 1)      0     150   150
"""

import dataclasses
import functools
import itertools
from typing import Optional, Tuple

import numpy as np

MARGIN_MIN = 1e-9
NEAR = 1e-3  # pairs within this relative distance of a cutoff are measured again in longdouble


@dataclasses.dataclass(frozen=True, eq=False)
class Case:
    """One frame.  ``types`` / ``table`` ([N] int64, [T, T] float64, rows = centre type) only on typed cases, whose geometry
    (and cached enumeration) is that of ``base``."""

    name: str
    pos: np.ndarray  # [N, 3] float64
    cell: Optional[np.ndarray]  # [3, 3] float64 (rows = lattice vectors) or None
    pbc: Tuple[bool, bool, bool]
    r_max: float
    types: Optional[np.ndarray] = None
    table: Optional[np.ndarray] = None
    base: Optional["Case"] = None

    @property
    def num_atoms(self) -> int:
        return int(self.pos.shape[0])


# ---- the reference ------------------------------------------------------------------------------------------------------------


def _images(case: Case):
    """``(S, translation)`` of every lattice image that can hold a partner: the range per periodic direction comes from the
    cell heights plus the spread of the fractional coordinates; an image whose bounding sphere cannot touch the frame's own
    (centre distance > 2 R + r_max, R = the largest distance of an atom from the centroid) is rejected whole."""
    if case.cell is None or case.num_atoms == 0:
        return [((0, 0, 0), np.zeros(3))]
    cell, pos = case.cell, case.pos
    inv = np.linalg.inv(cell)
    heights = 1.0 / np.linalg.norm(inv, axis=0)
    frac = pos @ inv
    spread = np.ceil(frac.max(0) - frac.min(0)).astype(int) + 1
    ranges = []
    for d in range(3):
        k = int(np.ceil(case.r_max / heights[d])) + int(spread[d])
        ranges.append(range(-k, k + 1) if case.pbc[d] else range(0, 1))
    radius = float(np.linalg.norm(pos - pos.mean(0), axis=1).max())
    reach = (2.0 * radius + case.r_max) * (1.0 + 1e-9)
    out = []
    for S in itertools.product(*ranges):
        t = np.array(S, dtype=np.float64) @ cell
        if float(np.linalg.norm(t)) <= reach:
            out.append((S, t))
    return out


def _enumerate(case: Case, dtype) -> np.ndarray:
    pos = case.pos.astype(dtype)
    r2max = dtype(case.r_max) * dtype(case.r_max)
    rows = []
    for S, t in _images(case):
        d = (pos[None, :, :] + t.astype(dtype)[None, None, :]) - pos[:, None, :]
        r2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
        hit = r2 < r2max
        if S == (0, 0, 0):
            np.fill_diagonal(hit, False)
        ii, jj = np.nonzero(hit)
        if len(ii):
            rows.append(np.concatenate([np.stack([ii, jj], 1), np.broadcast_to(np.array(S), (len(ii), 3))], 1))
    if not rows:
        return np.zeros((0, 5), dtype=np.int64)
    e = np.concatenate(rows).astype(np.int64)
    return e[np.lexsort((e[:, 4], e[:, 3], e[:, 2], e[:, 1], e[:, 0]))]


@functools.lru_cache(maxsize=None)
def _enumerate_cached(case: Case) -> np.ndarray:
    e = _enumerate(case, np.float64)
    e.setflags(write=False)
    return e


def enumerate_edges(case: Case) -> np.ndarray:
    """Every ``(i, j, Sx, Sy, Sz)`` of the UNTYPED list of ``case``: int64 ``[E, 5]``, lexsorted, read-only, cached per case."""
    return _enumerate_cached(case.base or case)


def enumerate_edges_float32(case: Case) -> np.ndarray:
    """The same enumeration with positions, translations and the comparison in float32 (what a comparison has to tell apart)."""
    return _enumerate(case.base or case, np.float32)


def edge_vectors(case: Case, edges: np.ndarray) -> np.ndarray:
    """``pos_j + S @ cell - pos_i`` of ``edges`` in float64."""
    t = edges[:, 2:].astype(np.float64) @ case.cell if case.cell is not None else 0.0
    return (case.pos[edges[:, 1]] + t) - case.pos[edges[:, 0]]


def typed_keep(case: Case, edges: np.ndarray) -> np.ndarray:
    """Mask of ``edges`` that the typed list keeps: ``r <= table[type_i][type_j]`` (compared as squares, as the cutoff is)."""
    v = edge_vectors(case, edges)
    rc = case.table[case.types[edges[:, 0]], case.types[edges[:, 1]]]
    return (v * v).sum(1) <= rc * rc


def typed_edges(case: Case) -> np.ndarray:
    e = enumerate_edges(case)
    return e[typed_keep(case, e)]


def sort_rows(rows: np.ndarray) -> np.ndarray:
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 5)
    return rows[np.lexsort((rows[:, 4], rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))]


def margin(case: Case) -> float:
    """``min | |r| - rc | / rc`` over all candidate pairs (every image the enumeration looks at) and every cutoff of the case:
    r_max and, for a typed case, every positive table entry (whatever the types of the pair).  A table entry of 0 keeps exactly
    the pairs with r == 0; against it the pairs ITS type pair selects are measured as ``|r| / r_max``, and none of them may
    coincide.  Pairs within ``NEAR`` of a cutoff in float64 are measured in ``numpy.longdouble``."""
    ld = np.longdouble
    cutoffs = [case.r_max]
    zero_pairs = None
    if case.table is not None:
        cutoffs += [float(c) for c in np.unique(case.table) if c > 0.0]
        zero_pairs = case.table[case.types[:, None], case.types[None, :]] == 0.0
    pos, pos_ld = case.pos, case.pos.astype(ld)
    cell_ld = case.cell.astype(ld) if case.cell is not None else None
    best = np.inf
    for S, t in _images(case):
        d = (pos[None, :, :] + t[None, None, :]) - pos[:, None, :]
        r = np.sqrt((d * d).sum(-1))
        if S == (0, 0, 0):
            np.fill_diagonal(r, np.inf)
        if zero_pairs is not None and zero_pairs.any():
            best = min(best, float(r[zero_pairs].min()) / case.r_max)
        for rc in cutoffs:
            rel = np.abs(r - rc) / rc
            near = rel < NEAR
            if near.any():
                ii, jj = np.nonzero(near)
                t_ld = np.array(S, dtype=ld) @ cell_ld if cell_ld is not None else ld(0)
                v = (pos_ld[jj] + t_ld) - pos_ld[ii]
                r_ld = np.sqrt((v * v).sum(-1))
                best = min(best, float((np.abs(r_ld - ld(rc)) / ld(rc)).min()))
            else:
                best = min(best, float(rel.min()))
    return best


# ---- the kernel's grid, restated ----------------------------------------------------------------------------------------------


def _inv3(c: np.ndarray) -> np.ndarray:
    """``inv3`` of the kernel: the cofactor formula, one rounding per operation in its order."""
    c = c.reshape(9)
    det = c[0] * (c[4] * c[8] - c[5] * c[7]) - c[1] * (c[3] * c[8] - c[5] * c[6]) + c[2] * (c[3] * c[7] - c[4] * c[6])
    r = 1.0 / det
    return np.array([(c[4] * c[8] - c[5] * c[7]) * r, (c[2] * c[7] - c[1] * c[8]) * r, (c[1] * c[5] - c[2] * c[4]) * r,
                     (c[5] * c[6] - c[3] * c[8]) * r, (c[0] * c[8] - c[2] * c[6]) * r, (c[2] * c[3] - c[0] * c[5]) * r,
                     (c[3] * c[7] - c[4] * c[6]) * r, (c[1] * c[6] - c[0] * c[7]) * r, (c[0] * c[4] - c[1] * c[3]) * r])


def wrapped_fractional(case: Case):
    """``(s, o)`` as ``nl_bin_atom`` forms them: ``s = pos @ inv`` summed left to right, periodic directions wrapped by
    ``floor`` with the ``s >= 1.0`` re-wrap, ``o`` the integer part removed; also the raw ``s - floor(s)`` before the re-wrap."""
    c = (case.cell if case.cell is not None else np.eye(3)).astype(np.float64)
    inv = _inv3(c).reshape(3, 3)
    p = case.pos
    s = (p[:, 0:1] * inv[0][None, :] + p[:, 1:2] * inv[1][None, :]) + p[:, 2:3] * inv[2][None, :]
    raw = s.copy()
    o = np.zeros(s.shape, dtype=np.int64)
    for d in range(3):
        if case.pbc[d]:
            fl = np.floor(s[:, d])
            o[:, d] = fl.astype(np.int64)
            s[:, d] = s[:, d] - fl
            raw[:, d] = s[:, d]
            again = s[:, d] >= 1.0
            s[again, d] -= 1.0
            o[again, d] += 1
    return s, o, raw


@dataclasses.dataclass(frozen=True)
class Grid:
    nb: Tuple[int, int, int]
    reach: Tuple[int, int, int]
    halvings: int  # coarsening steps (after the 1024 cap)
    capped: bool  # some direction asked for more than 1024 bins
    max_bin: int  # most atoms in one bin
    max_run: int  # most candidates in one z-run of one image, over all atoms' walks


def expected_grid(case: Case, bin_capacity: int) -> Grid:
    """A restatement of ``nl_size_grid`` (bins per direction = ``floor(extent * height / r_max)`` in [1, 1024], the largest
    direction halved until the grid fits ``bin_capacity``, ``reach = ceil(r_max / bin thickness)``, clipped to ``nb - 1``
    without periodicity), of the binning of ``nl_bin_atom`` and of the z-runs of ``nl_walk``.  IT HAS TO CHANGE TOGETHER WITH THE
    KERNEL'S RULE: the GPU test compares ``nb`` and ``reach`` with the header the kernel wrote."""
    c = (case.cell if case.cell is not None else np.eye(3)).astype(np.float64)
    inv = _inv3(c).reshape(3, 3)
    s, _, _ = wrapped_fractional(case)
    N = case.num_atoms
    p = case.pos
    s_raw = (p[:, 0:1] * inv[0][None, :] + p[:, 1:2] * inv[1][None, :]) + p[:, 2:3] * inv[2][None, :]
    nb, lo, extent, height = [0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
    capped = False
    for d in range(3):
        height[d] = 1.0 / np.sqrt(inv[0, d] * inv[0, d] + inv[1, d] * inv[1, d] + inv[2, d] * inv[2, d])
        if case.pbc[d]:
            lo[d], extent[d] = 0.0, 1.0
        else:
            lo[d] = float(s_raw[:, d].min()) if N else 0.0
            extent[d] = float(s_raw[:, d].max() - s_raw[:, d].min()) if N else 0.0
            extent[d] = extent[d] * (1.0 + 1e-9) + 1e-9
        n = int(np.floor(extent[d] * height[d] / case.r_max))
        n = max(n, 1)
        if n > 1024:
            n, capped = 1024, True
        nb[d] = n
    halvings = 0
    while nb[0] * nb[1] * nb[2] > bin_capacity:
        big = 0
        if nb[1] > nb[big]:
            big = 1
        if nb[2] > nb[big]:
            big = 2
        nb[big] = (nb[big] + 1) // 2
        halvings += 1
    width, reach = [0.0] * 3, [0] * 3
    for d in range(3):
        width[d] = extent[d] / float(nb[d])
        reach[d] = int(np.ceil(case.r_max / (width[d] * height[d])))
        if not case.pbc[d]:
            reach[d] = min(reach[d], nb[d] - 1)
    count = np.zeros(nb, dtype=np.int64)
    if N:
        b = np.stack([np.clip(np.floor((s[:, d] - lo[d]) / width[d]).astype(np.int64), 0, nb[d] - 1) for d in range(3)], 1)
        np.add.at(count, (b[:, 0], b[:, 1], b[:, 2]), 1)
    ptr = np.concatenate([np.zeros(nb[:2] + [1], dtype=np.int64), np.cumsum(count, axis=2)], axis=2)  # along z, per column
    max_run = 0
    for bx, by, bz in zip(*np.nonzero(count)):
        for dx in range(-reach[0], reach[0] + 1):
            x = bx + dx
            if not case.pbc[0] and not 0 <= x < nb[0]:
                continue
            for dy in range(-reach[1], reach[1] + 1):
                y = by + dy
                if not case.pbc[1] and not 0 <= y < nb[1]:
                    continue
                z, zhi = bz - reach[2], bz + reach[2]
                if not case.pbc[2]:
                    z, zhi = max(z, 0), min(zhi, nb[2] - 1)
                while z <= zhi:
                    nz = z // nb[2] if case.pbc[2] else 0
                    zend = min((nz + 1) * nb[2] - 1, zhi)
                    col = ptr[x % nb[0], y % nb[1]]
                    max_run = max(max_run, int(col[zend - nz * nb[2] + 1] - col[z - nz * nb[2]]))
                    z = zend + 1
    return Grid(tuple(nb), tuple(reach), halvings, capped, int(count.max()) if N else 0, max_run)


# ---- the cases ----------------------------------------------------------------------------------------------------------------

NAMES = ("crowded_single_bin", "dense_640", "blob_no_cell", "slab_crowded", "cluster_on_corner", "clipped_1024", "thin_x",
         "skewed", "left_handed", "one_atom_images", "coincident", "exact_grid", "minus_epsilon")
TYPED_NAMES = ("crowded_single_bin", "dense_640", "blob_no_cell", "coincident", "thin_x")
PADDED_NAMES = ("crowded_single_bin", "coincident", "one_atom_images")
PBC3 = (True, True, True)
NUM_TYPES, ABSENT_TYPE = 3, 1  # typed cases: three types, no atom has type 1


def _cube(a: float) -> np.ndarray:
    return np.eye(3) * a


def _grid(case: Case) -> Grid:
    return expected_grid(case, case.num_atoms + 8)


def _degrees(case: Case) -> np.ndarray:
    return np.bincount(enumerate_edges(case)[:, 0], minlength=case.num_atoms)


def _crowded_positions() -> np.ndarray:
    return np.random.default_rng(11).uniform(0.0, 8.0, size=(150, 3))


def _build(name: str) -> Case:
    if name == "crowded_single_bin":
        case = Case(name, _crowded_positions(), _cube(8.0), PBC3, 4.5)
        g = _grid(case)
        assert g.nb == (1, 1, 1) and g.max_bin == 150 and g.max_run == 150, g
    elif name == "dense_640":
        case = Case(name, np.random.default_rng(12).uniform(0.0, 18.0, size=(640, 3)), _cube(18.0), PBC3, 5.0)
        g = _grid(case)
        assert g.nb == (3, 3, 3) and g.max_run > 64, g
    elif name == "blob_no_cell":
        case = Case(name, np.random.default_rng(13).uniform(-2.0, 2.0, size=(200, 3)), None, (False,) * 3, 5.0)
        g = _grid(case)
        assert g.max_bin == 200 and g.reach == (0, 0, 0), g
    elif name == "slab_crowded":
        rng = np.random.default_rng(14)
        pos = np.concatenate([rng.uniform(0.0, 9.0, size=(120, 2)), rng.uniform(13.5, 16.5, size=(120, 1))], 1)
        case = Case(name, pos, np.diag([9.0, 9.0, 30.0]), (True, True, False), 4.5)
        g = _grid(case)
        assert g.nb == (2, 2, 1) and g.reach == (1, 1, 0), g
    elif name == "cluster_on_corner":
        case = Case(name, np.random.default_rng(15).normal(0.0, 1.6, size=(130, 3)), _cube(40.0), PBC3, 4.0)
        g = _grid(case)
        assert g.halvings == 3 and g.nb == (5, 5, 5), g
        s, _, _ = wrapped_fractional(case)
        corners = {tuple(r) for r in (s > 0.5).astype(int)}
        assert len(corners) == 8, "the cluster has to reach all eight corner bins"
    elif name == "clipped_1024":
        pos = np.array([[0.5, 2500.0, 2500.0], [4999.0, 2500.0, 2500.0],          # across the x faces
                        [0.75, 0.5, 0.625], [4999.25, 4999.5, 4999.0],            # across opposite corners
                        [1234.5, 3210.25, 777.0], [1236.0, 3211.5, 778.5],        # interior
                        [3000.0, 1000.0, 4000.0]])                                # isolated
        case = Case(name, pos, _cube(5000.0), PBC3, 4.0)
        g = _grid(case)
        assert g.capped and g.halvings > 0 and g.nb[0] * g.nb[1] * g.nb[2] <= case.num_atoms + 8, g
        assert np.array_equal(_degrees(case), [1, 1, 1, 1, 1, 1, 0])
    elif name == "thin_x":
        cell = np.array([[1.7, 0.0, 0.0], [0.4, 9.0, 0.0], [0.3, -0.2, 11.0]])
        case = Case(name, np.random.default_rng(17).uniform(-0.5, 1.5, size=(80, 3)) @ cell, cell, PBC3, 4.0)
        assert _grid(case).reach == (3, 1, 1), _grid(case)
    elif name == "skewed":
        cell = np.array([[10.0, 0.0, 0.0], [9.0, 3.0, 0.0], [8.0, 2.0, 3.0]])
        case = Case(name, np.random.default_rng(18).uniform(0.0, 1.0, size=(60, 3)) @ cell, cell, PBC3, 4.0)
        g = _grid(case)
        assert g.nb == (1, 1, 1) and g.reach == (2, 2, 2), g
    elif name == "left_handed":
        cell = np.array([[7.0, 0.3, -0.4], [1.9, 6.5, 0.2], [1.1, -2.4, -8.0]])
        assert np.linalg.det(cell) < 0.0
        case = Case(name, np.random.default_rng(19).uniform(-0.7, 1.7, size=(50, 3)) @ cell, cell, PBC3, 3.5)
    elif name == "one_atom_images":
        cell = np.array([[2.5, 0.0, 0.0], [0.5, 2.4, 0.0], [0.2, 0.3, 2.6]])
        case = Case(name, np.array([[0.3, 0.2, 0.1]]), cell, PBC3, 6.0)
        e = enumerate_edges(case)
        assert _grid(case).reach == (3, 3, 3) and len(e) == 60 and not e[:, :2].any(), (_grid(case), len(e))
    elif name == "coincident":
        # positions on a 2^-30 grid, so that adding the lattice vector (0, 0, 7) is exact and the image pair has r == 0
        pos = np.round(np.random.default_rng(20).uniform(0.0, 7.0, size=(40, 3)) * 2.0 ** 30) / 2.0 ** 30
        cell = _cube(7.0)
        pos = np.concatenate([pos, pos[0:1], pos[1:2] + cell[2]])
        case = Case(name, pos, cell, PBC3, 3.0)
        e = enumerate_edges(case)
        zero = e[(edge_vectors(case, e) == 0.0).all(1)]
        want = [[0, 40, 0, 0, 0], [1, 41, 0, 0, -1], [40, 0, 0, 0, 0], [41, 1, 0, 0, 1]]
        assert np.array_equal(zero, want), zero
    elif name == "exact_grid":
        rng = np.random.default_rng(21)
        sites = rng.choice(32 ** 3, size=300, replace=False)  # distinct sites of the 0.5 A lattice in [-4, 12)^3
        pos = np.stack([sites // 1024, (sites // 32) % 32, sites % 32], 1).astype(np.float64) * 0.5 - 4.0
        case = Case(name, pos, _cube(8.0), PBC3, 2.0)
        boundary = 0
        for S, t in _images(case):
            d = (pos[None, :, :] + t) - pos[:, None, :]
            boundary += int(((d * d).sum(-1) == 4.0).sum())
        e = enumerate_edges(case)
        v = edge_vectors(case, e)
        assert boundary >= 1 and ((v * v).sum(1) < 4.0).all() and _grid(case).nb == (4, 4, 4), boundary
        assert (pos < 0).any() and (pos >= 8).any() and (pos % 8 == 0).any() and (pos % 2 == 0).any()
    elif name == "minus_epsilon":
        pos = _crowded_positions()
        pos[0, 0] = -2.0 ** -60
        pos[1, 1] = -2.0 ** -60
        pos[2, 2] = 8.0 - 2.0 ** -60  # (rounds to 8.0: exactly on the upper face)
        case = Case(name, pos, _cube(8.0), PBC3, 4.5)
        s, o, raw = wrapped_fractional(case)
        assert raw[0, 0] == 1.0 and raw[1, 1] == 1.0, "s - floor(s) of -epsilon has to round to 1.0"
        assert s[0, 0] == 0.0 and o[0, 0] == 0 and s[1, 1] == 0.0 and o[1, 1] == 0 and s[2, 2] == 0.0 and o[2, 2] == 1
    else:
        raise KeyError(name)
    case.pos.setflags(write=False)
    return case


@functools.lru_cache(maxsize=None)
def make_case(name: str) -> Case:
    return _build(name)


@functools.lru_cache(maxsize=None)
def typed_case(name: str) -> Case:
    """``make_case(name)`` with random types out of {0, 2} (no atom has ``ABSENT_TYPE``) and an asymmetric table whose entries
    are r_max, 0.6 r_max and 0.0.  The two copies of ``coincident`` are copies of an atom, type included."""
    base = make_case(name)
    rng = np.random.default_rng(100 + NAMES.index(name))
    types = rng.choice(np.array([0, 2]), size=base.num_atoms).astype(np.int64)
    if name == "coincident":
        types[40], types[41] = types[0], types[1]
    r = base.r_max
    table = np.array([[r, 0.6 * r, 0.6 * r], [0.0, r, r], [0.0, 0.6 * r, r]])
    assert not np.array_equal(table, table.T) and not (types == ABSENT_TYPE).any() and len(set(types.tolist())) == 2
    return dataclasses.replace(base, name=name + "_typed", types=types, table=table, base=base)


def kdtree_supported(case: Case) -> bool:
    """``nequip_amd.utils.synthetic.neighbor_list`` takes one periodicity flag, searches ``ceil(r_max / height)`` images on
    either side (enough only while the fractional coordinates spread over less than one cell) and keeps ``r <= r_max``."""
    if case.cell is None:
        return True
    if not all(case.pbc) or case.name == "exact_grid":
        return False
    frac = case.pos @ np.linalg.inv(case.cell)
    return bool(((frac.max(0) - frac.min(0)) < 1.0).all())


def table_row(case: Case) -> str:
    g, deg, e = _grid(case), _degrees(case), enumerate_edges(case)
    return (f"{case.name:<20}{case.num_atoms:>4}{len(e):>8}  {deg.min():>3}..{deg.max():<3}  {margin(case):7.1e}  "
            f"{str(g.nb):<13}{str(g.reach):<13}{g.halvings:>3}    {g.max_bin:>4}  {g.max_run:>4}")
