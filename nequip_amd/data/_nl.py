"""Neighbour lists on the device (mirror of ``nequip/data/_nl.py:63-381`` for one backend, ``"nequip_amd"``).

``compute_neighborlist_(data, r_max)`` keeps the reference's contract (``_nl.py:364-381``): it adds ``edge_index``
(int64 ``[2, E]``, row 0 = convolution centre, row 1 = neighbour) and -- iff the data has a cell -- ``edge_cell_shift``
(``[E, 3]``, dtype of the positions) to ``data`` in place; batched input gives batched output, unbatched gives
unbatched, everything stays on the device of the positions.  Where the reference moves the positions to the host and
calls matscipy / ASE / vesin, this backend runs a cell-list search on the GPU (``nqa_neighbor_list_count/fill``,
``nequip_amd/csrc/neighbor_list.hip``) with the same pair semantics (``|r| < r_max``, no self pair with zero shift,
mixed periodicity, cells thinner than the cutoff).  Edges come out grouped by centre atom, so the dst-CSR of the
tensor-product kernels needs no sort for them.

Batched data goes through ``nqa_neighbor_list_batched_count/fill``: one set of launches and one host read (the edge count)
for the whole batch, bitwise the same list as the per-frame loop.  ``NQA_NL_PER_FRAME=1`` (read at every call) keeps the
per-frame loop.

``per_edge_type_cutoff`` (a dict as the model builders take it, with ``type_names``; a ``[T, T]`` tensor, rows = centre type; or
a ``CutoffTable``) makes every form of the list typed: the edge ``i <- j`` is kept iff ``r < r_max`` and
``r <= cutoff[type_i][type_j]`` (``nqa_neighbor_list_*_typed``), which is the reference's ``NeighborListTransform(
per_edge_type_cutoff=...)`` (``nequip/data/transforms/neighborlist.py:9-117``) without building the full list first.  The result
is bitwise the untyped list with the other edges removed.  ``None`` is the untyped code path, unchanged.
"""

import ctypes
import os
from typing import Dict, Final, List, Optional, Tuple, Union

import torch

from .. import _lib
from ..utils import ktimer
from . import AtomicDataDict

NEIGHBORLIST_BACKEND_NEQUIP_AMD: Final[str] = "nequip_amd"
DEFAULT_NEIGHBORLIST_BACKEND: Final[str] = NEIGHBORLIST_BACKEND_NEQUIP_AMD


_ptr = _lib.ptr


def _complete_cell_host(cell64: torch.Tensor, pbc: Tuple[bool, bool, bool]) -> torch.Tensor:
    """Cells with zero lattice vectors along non-periodic directions (ASE slabs / wires / molecules with pbc = (T, T, F)
    and c = 0): complete them with unit vectors orthogonal to the span of the others, as ``ase.geometry.complete_cell``
    does and the reference's backends accept -- the kernel inverts the cell.  A zero (or linearly dependent) vector
    along a *periodic* direction is an error.

    The check reads the nine numbers on the host: one small copy per call, next to the one synchronisation the
    neighbour list needs anyway (the data-dependent edge count).  Deliberately not memoised on the tensor's storage:
    a recycled allocation would look like the same cell."""
    import numpy as np

    c = cell64.detach().cpu().numpy().copy()
    norms = np.linalg.norm(c, axis=1)
    missing = [i for i in range(3) if norms[i] < 1e-12]
    if not missing:
        if abs(np.linalg.det(c)) < 1e-12 * max(1.0, norms.prod()):
            raise ValueError("cell vectors are linearly dependent")
        return cell64
    for i in missing:
        if pbc[i]:
            raise ValueError(f"lattice vector {i} is zero but the direction is periodic")
    # orthonormal basis of the span of the present vectors (Gram-Schmidt), then unit vectors orthogonal to it
    basis = []
    for i in range(3):
        if i in missing:
            continue
        v = c[i].copy()
        for b in basis:
            v -= np.dot(v, b) * b
        n = np.linalg.norm(v)
        if n < 1e-12 * norms[i]:
            raise ValueError("cell vectors are linearly dependent")
        basis.append(v / n)
    for i in missing:
        if len(basis) == 2:
            v = np.cross(basis[0], basis[1])
        else:
            # the coordinate axis with the largest component orthogonal to the basis so far
            best = None
            for axis in np.eye(3):
                w = axis.copy()
                for b in basis:
                    w -= np.dot(w, b) * b
                n = np.linalg.norm(w)
                if best is None or n > best[0]:
                    best = (n, w)
            v = best[1]
        v = v / np.linalg.norm(v)
        c[i] = v
        basis.append(v)
    if abs(np.linalg.det(c)) < 1e-12:
        raise ValueError("cell vectors are linearly dependent")
    return torch.as_tensor(c, dtype=torch.float64, device=cell64.device).contiguous()


_complete_cell = _complete_cell_host  # (the name the single-frame callers use; the batched list completes cells on the device)


_NL_BAD_TYPE = 32  # status bit of the typed entry points: an atom type outside [0, num_types)
_BAD_TYPE_MSG = "atom_types holds a type index outside [0, {T}): the per-edge-type cutoff table has {T} types"
_MISSING_TYPES_MSG = (
    f"Per-edge-type cutoffs require '{AtomicDataDict.ATOM_TYPE_KEY}' to be present in the data. "
    "This is likely because the chemical species have not been mapped to atom types before the neighborlist is built. "
    "Please check your data transform order.")


class CutoffTable:
    """A checked per-edge-type cutoff table: float64 ``[T, T]`` on the host, row-major (centre type, neighbour type), every
    entry positive and ``<= r_max`` (the reference asserts both, ``nequip/nn/embedding/utils.py``); device copies are made once
    per device."""

    def __init__(self, table: torch.Tensor, r_max: float):
        table = torch.as_tensor(table).detach().to(device="cpu", dtype=torch.float64)
        if table.dim() != 2 or table.shape[0] != table.shape[1] or table.shape[0] < 1:
            raise ValueError(f"per-edge-type cutoffs must be a [T, T] table, got shape {tuple(table.shape)}")
        if not bool(torch.all(table > 0)):  # (also refuses NaN)
            raise ValueError("per-edge-type cutoffs must be positive")
        if not bool(torch.all(table <= float(r_max))):
            raise ValueError(f"per-edge-type cutoffs cannot exceed r_max = {r_max} (largest entry: {float(table.max())})")
        self.table = table.contiguous()
        self.r_max = float(r_max)
        self.num_types = int(table.shape[0])
        self.symmetric = bool(torch.equal(table, table.t()))
        self._on: Dict[torch.device, torch.Tensor] = {}

    def on(self, device: torch.device) -> torch.Tensor:
        key = torch.device(device)
        if key not in self._on:
            self._on[key] = self.table.to(device)
        return self._on[key]


def as_cutoff_table(per_edge_type_cutoff, type_names: Optional[List[str]], r_max: float) -> Optional[CutoffTable]:
    """``None`` -> ``None``; a dict (``{"H": 3.0, "O": {"H": 3.5}}``, needs ``type_names``), a ``[T, T]`` tensor or a
    ``CutoffTable`` -> a ``CutoffTable`` checked against ``r_max`` (on the host, before anything is launched)."""
    if per_edge_type_cutoff is None:
        return None
    if isinstance(per_edge_type_cutoff, CutoffTable):
        if per_edge_type_cutoff.r_max > float(r_max):
            return CutoffTable(per_edge_type_cutoff.table, r_max)
        return per_edge_type_cutoff
    if isinstance(per_edge_type_cutoff, dict):
        if type_names is None:
            raise ValueError("`type_names` required for `per_edge_type_cutoff`")
        from ..nn.embedding import cutoff_partialdict_to_tensor

        per_edge_type_cutoff = cutoff_partialdict_to_tensor(per_edge_type_cutoff, list(type_names), float(r_max))
    return CutoffTable(per_edge_type_cutoff, r_max)


def _types_for(table: Optional[CutoffTable], atom_types: Optional[torch.Tensor], N: int, device) -> Optional[torch.Tensor]:
    if table is None:
        return None
    if atom_types is None:
        raise KeyError(_MISSING_TYPES_MSG)
    types = atom_types.detach().reshape(-1).to(device=device, dtype=torch.int64).contiguous()
    if types.numel() != N:
        raise ValueError(f"{types.numel()} atom types for {N} atoms")
    return types


def _norm_pbc(pbc: Union[bool, Tuple[bool, bool, bool], torch.Tensor]) -> Tuple[bool, bool, bool]:
    if isinstance(pbc, bool):
        return (pbc,) * 3
    if isinstance(pbc, torch.Tensor):
        pbc = pbc.detach().cpu().view(-1).tolist()
    return tuple(bool(b) for b in pbc)


# ---- the library calls: every form of the list goes through these three -------------------------------------------------
# The operands that are there pick the entry point: ``frame_ptr`` / ``F`` (a batched list), ``types`` and ``table`` / ``T`` (a
# typed list), ``padded`` (the extra outputs of a capacity-padded fill).


def _nl_workspace_bytes(lib, N: int, F: Optional[int] = None, T: int = 0) -> int:
    if F is None:
        return lib.nqa_neighbor_list_typed_workspace_bytes(N, T) if T else lib.nqa_neighbor_list_workspace_bytes(N)
    if T:
        return lib.nqa_neighbor_list_batched_typed_workspace_bytes(N, F, T)
    return lib.nqa_neighbor_list_batched_workspace_bytes(N, F)


def _nl_count(lib, pos64, cell64, pbc32, r_max: float, N: int, ws, ws_bytes: int, rowptr, stream, frame_ptr=None, types=None,
              table=None, symmetrise: bool = False, status=None) -> None:
    """The count pass into ``rowptr`` [N + 1].  ``table``: the cutoffs [T, T] on the device (with ``types`` [N]); ``status``: the
    int32 word of the batched and the typed forms; ``symmetrise``: single-frame typed lists only."""
    batched, typed = frame_ptr is not None, table is not None
    if batched:
        fn = lib.nqa_neighbor_list_batched_count_typed if typed else lib.nqa_neighbor_list_batched_count
    else:
        fn = lib.nqa_neighbor_list_count_typed if typed else lib.nqa_neighbor_list_count
    args = [_ptr(pos64), _ptr(cell64), _ptr(pbc32)] + ([_ptr(frame_ptr)] if batched else []) + [float(r_max)]
    if typed:
        args += [_ptr(types), _ptr(table), table.shape[0]] + ([] if batched else [int(bool(symmetrise))])
    args += [N] + ([frame_ptr.numel() - 1] if batched else []) + [_ptr(ws), ws_bytes, _ptr(rowptr)]
    if batched or typed:
        args.append(_ptr(status))
    _lib.check(fn(*args, stream), fn.__name__)


def _nl_fill(lib, ws, rowptr, N: int, E: int, edge_index, shifts, stream, F: Optional[int] = None, types=None, T: int = 0,
             padded=None) -> None:
    """The fill pass after a count with the same ``F`` / ``T``.  ``padded = (rowptr_padded, src32, status)``: the capacity-padded
    fill, ``E`` is then the capacity."""
    batched, typed = F is not None, types is not None
    if padded is not None:
        fn = lib.nqa_neighbor_list_fill_padded_typed if typed else lib.nqa_neighbor_list_fill_padded
    elif batched:
        fn = lib.nqa_neighbor_list_batched_fill_typed if typed else lib.nqa_neighbor_list_batched_fill
    else:
        fn = lib.nqa_neighbor_list_fill_typed if typed else lib.nqa_neighbor_list_fill
    args = [_ptr(ws), _ptr(rowptr)] + ([_ptr(types)] if typed else []) + [N] + ([F] if batched else [])
    args += ([T] if typed else []) + [E]
    if padded is None:
        args += [_ptr(edge_index), _ptr(shifts)]
    else:
        args += [_ptr(padded[0]), _ptr(edge_index), _ptr(shifts), _ptr(padded[1]), _ptr(padded[2])]
    _lib.check(fn(*args, stream), fn.__name__)


_BATCHED_STATUS_ERRORS = (
    (1, RuntimeError, "neighbour list has more than 2^31 - 1 edges"),
    (2, ValueError, "a lattice vector is zero but the direction is periodic"),
    (4, ValueError, "cell vectors are linearly dependent"),
    (8, ValueError, "the frame sizes (num_nodes / batch) do not add up to the number of atoms"),
    (16, ValueError, "Periodic boundary conditions requested but no cell was provided."),
)


def _raise_for_status(E: int, bad: int, T: int) -> None:
    """The errors a count reports on the device: ``bad`` is its status word (0 where the form has none), ``E`` the edge count
    (negative after an int32 overflow of the scan)."""
    if bad & _NL_BAD_TYPE:
        raise ValueError(_BAD_TYPE_MSG.format(T=T))
    for bit, exc, msg in _BATCHED_STATUS_ERRORS:
        if bad & bit:
            raise exc(msg)
    if E < 0:
        raise RuntimeError(_BATCHED_STATUS_ERRORS[0][2])


def _compute_neighborlist_single_frame(
    pos: torch.Tensor,
    r_max: float,
    cell: Optional[torch.Tensor] = None,
    pbc: Union[bool, Tuple[bool, bool, bool], torch.Tensor] = False,
    return_rowptr: bool = False,
    atom_types: Optional[torch.Tensor] = None,
    per_edge_type_cutoff=None,
    type_names: Optional[List[str]] = None,
    symmetrise: bool = False,
):
    """``(edge_index [2, E] int64, edge_cell_shift [E, 3])`` of one frame (``nequip/data/_nl.py:63-165``); with
    ``per_edge_type_cutoff`` (and ``atom_types``) the typed list; ``symmetrise``: typed by ``max(rc[a][b], rc[b][a])`` (the
    kernel's flag), the list the capacity-padded form holds."""
    table = as_cutoff_table(per_edge_type_cutoff, type_names, r_max)
    if not pos.is_cuda:
        raise RuntimeError("the `nequip_amd` neighbour list runs on the GPU: positions must be a CUDA/HIP tensor")
    pbc = _norm_pbc(pbc)
    if cell is None and any(pbc):
        raise ValueError("Periodic boundary conditions requested but no cell was provided.")
    lib = _lib.load()
    device = pos.device
    out_dtype = pos.dtype
    N = pos.shape[0]
    pos64 = pos.detach().to(torch.float64).contiguous()
    cell64 = cell.detach().to(torch.float64).reshape(3, 3).contiguous() if cell is not None else None
    if cell64 is not None:
        cell64 = _complete_cell(cell64, pbc)
    pbc_dev = torch.tensor([int(b) for b in pbc], dtype=torch.int32, device=device)
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    types = _types_for(table, atom_types, N, device)
    T = table.num_types if table is not None else 0
    ws_bytes = _nl_workspace_bytes(lib, N, T=T)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    if table is None:
        rowptr, status = torch.empty(N + 1, dtype=torch.int32, device=device), None
    else:
        aux = torch.empty(N + 2, dtype=torch.int32, device=device)  # rowptr [N + 1] and the status word, read back as one pair
        rowptr, status = aux[:N + 1], aux[N + 1:]
    with torch.cuda.device(device):
        _nl_count(lib, pos64, cell64, pbc_dev, r_max, N, ws, ws_bytes, rowptr, stream, types=types,
                  table=table.on(device) if table is not None else None, symmetrise=symmetrise, status=status)
        # the one synchronisation: the edge count is data dependent
        E, bad = (int(rowptr[N].item()), 0) if table is None else aux[N:].tolist()
        _raise_for_status(E, bad, T)
        edge_index = torch.empty((2, E), dtype=torch.int64, device=device)
        shifts = torch.empty((E, 3), dtype=torch.float64, device=device)
        _nl_fill(lib, ws, rowptr, N, E, edge_index, shifts, stream, types=types, T=T)
    if return_rowptr:
        return edge_index, shifts.to(out_dtype), rowptr
    return edge_index, shifts.to(out_dtype)


class PaddedNeighborList:
    """Neighbour list of ONE frame with a fixed number of edge slots and no host read-back (``nqa_neighbor_list_count`` +
    ``nqa_neighbor_list_fill_padded``): every launch of ``build`` goes to the current stream and every shape is static, so
    ``positions -> neighbour list -> pairing -> model`` can be captured in one hipGraph and replayed (molecular dynamics;
    the reference builds the list on the host at every step, ``nequip/integrations/ase.py:125-160`` ->
    ``nequip/data/_nl.py:63-165``).

    The ``edge_capacity - E`` unused slots hold padding edges: self-image pairs ``(i <- i, +-S)`` longer than ``r_max``, dealt
    out evenly over the atoms.  They lie outside the polynomial cutoff, so their radial embedding, their (bias-free) radial-MLP
    weights and all derivatives vanish: energies, forces and virials are those of the unpadded list.  Needs a cell.

    ``status()`` (a synchronising read, for AFTER the step) reports ``(fits, E)``: when the list did not fit, the output of that
    ``build`` holds padding only and the caller repeats the step with a larger capacity.

    With ``per_edge_type_cutoff`` and ``atom_types`` (fixed for the life of the object, checked against the table once, here)
    the real edges are the typed list of the SYMMETRISED table ``max(rc[a][b], rc[b][a])``: the padding comes in pairs, so the
    number of real edges has to be even, which a symmetric list guarantees.  The extra edges of an asymmetric table lie beyond
    their own type cutoff and are zeroed by the model, as every edge outside its cutoff is."""

    def __init__(self, num_atoms: int, r_max: float, cell: torch.Tensor,
                 pbc: Union[bool, Tuple[bool, bool, bool], torch.Tensor], edge_capacity: int,
                 shift_dtype: torch.dtype = torch.float32, atom_types: Optional[torch.Tensor] = None,
                 per_edge_type_cutoff=None, type_names: Optional[List[str]] = None):
        if cell is None:
            raise ValueError("a capacity-padded neighbour list needs a cell (its padding edges are lattice images)")
        if not cell.is_cuda:
            raise RuntimeError("the `nequip_amd` neighbour list runs on the GPU: the cell must be a CUDA/HIP tensor")
        pbc = _norm_pbc(pbc)
        self.num_atoms = int(num_atoms)
        if self.num_atoms < 1:
            raise ValueError("a capacity-padded neighbour list needs at least one atom")
        self.r_max = float(r_max)
        self.edge_capacity = int(edge_capacity) + (int(edge_capacity) & 1)  # (pairs of edges)
        if not 0 <= self.edge_capacity < 2**31 - 1:
            raise ValueError("edge capacity outside the int32 index range of the kernels")
        self.shift_dtype = shift_dtype
        self.device = cell.device
        self.pbc = pbc
        lib = _lib.load()
        self.cell64 = torch.empty(3, 3, dtype=torch.float64, device=self.device)
        self.set_cell(cell)
        self._pbc_dev = torch.tensor([int(b) for b in pbc], dtype=torch.int32, device=self.device)
        self.cutoff_table = as_cutoff_table(per_edge_type_cutoff, type_names, self.r_max)
        self._types = _types_for(self.cutoff_table, atom_types, self.num_atoms, self.device)
        self._table_dev = self._type_status = None
        self._num_types = T = self.cutoff_table.num_types if self.cutoff_table is not None else 0
        if self.cutoff_table is not None:
            if bool(((self._types < 0) | (self._types >= T)).any()):
                raise ValueError(_BAD_TYPE_MSG.format(T=T))
            self._table_dev = self.cutoff_table.on(self.device)  # (symmetrised by the count kernel: symmetrise = 1)
            self._type_status = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws_bytes = _nl_workspace_bytes(lib, self.num_atoms, T=T)
        self._ws = torch.empty(max(self._ws_bytes, 1), dtype=torch.uint8, device=self.device)
        self._rowptr = torch.empty(self.num_atoms + 1, dtype=torch.int32, device=self.device)
        self._status = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._edge_ids = torch.arange(max(self.edge_capacity, 1), dtype=torch.int32, device=self.device)
        self.last_csr = None

    def set_cell(self, cell: torch.Tensor) -> None:
        """New lattice vectors (variable-cell dynamics): written into the buffer the captured launches read.  Reads the cell on
        the host once (completion of missing lattice vectors, as ``_compute_neighborlist_single_frame`` does)."""
        c = _complete_cell(cell.detach().to(torch.float64).reshape(3, 3).contiguous(), self.pbc)
        self.cell64.copy_(c)

    def build(self, pos: torch.Tensor):
        """``(edge_index [2, capacity] int64, edge_cell_shift [capacity, 3], rowptr [N + 1] int32)`` for ``pos``; also leaves
        the fit flag in ``status_tensor`` (device).  No synchronisation."""
        if not pos.is_cuda or pos.shape != (self.num_atoms, 3):
            raise RuntimeError(f"positions must be a CUDA/HIP tensor of shape ({self.num_atoms}, 3)")
        lib = _lib.load()
        dev = self.device
        pos64 = pos.detach().to(torch.float64).contiguous()
        cap = self.edge_capacity
        edge_index = torch.empty((2, cap), dtype=torch.int64, device=dev)
        shifts = torch.empty((cap, 3), dtype=torch.float64, device=dev)
        rowptr = torch.empty(self.num_atoms + 1, dtype=torch.int32, device=dev)
        src32 = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        stream = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        with torch.cuda.device(dev):
            _nl_count(lib, pos64, self.cell64, self._pbc_dev, self.r_max, self.num_atoms, self._ws, self._ws_bytes, self._rowptr,
                      stream, types=self._types, table=self._table_dev, symmetrise=True, status=self._type_status)
            _nl_fill(lib, self._ws, self._rowptr, self.num_atoms, cap, edge_index, shifts, stream, types=self._types,
                     T=self._num_types, padded=(rowptr, src32, self._status))
        self.last_csr = (rowptr, self._edge_ids, src32)  # the dst-CSR of the list just built (edge ids = 0 .. capacity - 1)
        return edge_index, shifts.to(self.shift_dtype), rowptr

    @property
    def status_tensor(self) -> torch.Tensor:
        """int32[2] on the device: ``[did not fit, E]`` of the last ``build``."""
        return self._status

    def status(self) -> Tuple[bool, int]:
        """``(fits, E)`` of the last ``build`` (synchronises)."""
        bad, e = self._status.cpu().tolist()
        return bad == 0, int(e)


def compute_neighborlist_padded_(data: AtomicDataDict.Type, nl: PaddedNeighborList) -> AtomicDataDict.Type:
    """``compute_neighborlist_`` for one unbatched frame through a ``PaddedNeighborList``: adds ``edge_index`` and
    ``edge_cell_shift`` (both ``nl.edge_capacity`` long) in place and hands the row pointer to the topology cache."""
    K = AtomicDataDict
    if K.BATCH_KEY in data and K.num_frames(data) != 1:
        raise ValueError("a capacity-padded neighbour list holds one frame")
    edge_index, shifts, rowptr = nl.build(data[K.POSITIONS_KEY])
    data[K.EDGE_INDEX_KEY] = edge_index
    data[K.EDGE_CELL_SHIFT_KEY] = shifts
    from ..nn._topology import topology_cache

    topology_cache.hint_sorted(edge_index, rowptr, csr=nl.last_csr)
    return data


def _frame_from_batched(data: AtomicDataDict.Type, idx: int, node_offsets) -> AtomicDataDict.Type:
    K = AtomicDataDict
    lo, hi = int(node_offsets[idx]), int(node_offsets[idx + 1])
    out = {K.POSITIONS_KEY: data[K.POSITIONS_KEY][lo:hi]}
    if K.ATOM_TYPE_KEY in data:
        out[K.ATOM_TYPE_KEY] = data[K.ATOM_TYPE_KEY].view(-1)[lo:hi]
    if K.CELL_KEY in data:
        out[K.CELL_KEY] = data[K.CELL_KEY].view(-1, 3, 3)[idx]
    if K.PBC_KEY in data:
        out[K.PBC_KEY] = data[K.PBC_KEY].view(-1, 3)[idx]
    return out


def _batched_frame_count(data: AtomicDataDict.Type) -> int:
    """Number of frames from shapes alone where the data has them (no host read); ``num_frames`` otherwise."""
    K = AtomicDataDict
    if K.NUM_NODES_KEY in data:
        return data[K.NUM_NODES_KEY].size(0)
    for key, width in ((K.CELL_KEY, 9), (K.PBC_KEY, 3)):
        if data.get(key, None) is not None:
            return data[key].numel() // width
    return K.num_frames(data)


def _frame_ptr(data: AtomicDataDict.Type, num_frames: int, device: torch.device) -> torch.Tensor:
    """int64 [F + 1] atom offsets of the frames, built on the device: cumsum of ``num_nodes`` or, from ``batch`` (atoms grouped
    by frame), the first atom of every frame (a search with a known frame count: no host read)."""
    K = AtomicDataDict
    ptr = torch.zeros(num_frames + 1, dtype=torch.int64, device=device)
    if K.NUM_NODES_KEY in data:
        torch.cumsum(data[K.NUM_NODES_KEY].view(-1).to(device=device, dtype=torch.int64), 0, out=ptr[1:])
    else:
        batch = data[K.BATCH_KEY].view(-1).to(device=device, dtype=torch.int64).contiguous()
        ptr = torch.searchsorted(batch, torch.arange(num_frames + 1, dtype=torch.int64, device=device))
    return ptr


def _compute_neighborlist_batched(pos: torch.Tensor, r_max: float, frame_ptr: torch.Tensor,
                                  cell: Optional[torch.Tensor] = None, pbc: Optional[torch.Tensor] = None,
                                  atom_types: Optional[torch.Tensor] = None, per_edge_type_cutoff=None,
                                  type_names: Optional[List[str]] = None):
    """``(edge_index [2, E] int64, edge_cell_shift [E, 3], rowptr [N + 1] int32)`` of F frames in one pass: frame f holds the
    atoms ``frame_ptr[f]:frame_ptr[f + 1]`` with cell ``cell[f]`` ([F, 3, 3] or None) and periodicity ``pbc[f]`` ([F, 3] or
    None).  Equal to the concatenation of the frames' ``_compute_neighborlist_single_frame`` lists (atom indices offset);
    reads the edge count and the status word back together: the one synchronisation of the batch.  With
    ``per_edge_type_cutoff``: the typed list (``atom_types`` [N] over the whole batch, one table for all frames)."""
    table = as_cutoff_table(per_edge_type_cutoff, type_names, r_max)
    if not pos.is_cuda:
        raise RuntimeError("the `nequip_amd` neighbour list runs on the GPU: positions must be a CUDA/HIP tensor")
    lib = _lib.load()
    device = pos.device
    N = pos.shape[0]
    F = frame_ptr.numel() - 1
    if F < 1:
        raise ValueError("a batched neighbour list needs at least one frame")
    pos64 = pos.detach().to(torch.float64).contiguous()
    cell64 = None
    if cell is not None:
        if cell.numel() != 9 * F:
            raise ValueError(f"cell of shape {tuple(cell.shape)} for {F} frames: expected [{F}, 3, 3]")
        cell64 = cell.detach().to(device=device, dtype=torch.float64).reshape(F, 3, 3).contiguous()
    pbc32 = None
    if pbc is not None:
        if pbc.numel() != 3 * F:
            raise ValueError(f"pbc of shape {tuple(pbc.shape)} for {F} frames: expected [{F}, 3]")
        pbc32 = pbc.detach().to(device=device, dtype=torch.int32).reshape(F, 3).contiguous()
    frame_ptr = frame_ptr.to(device=device, dtype=torch.int64).contiguous()
    types = _types_for(table, atom_types, N, device)
    T = table.num_types if table is not None else 0
    ws_bytes = _nl_workspace_bytes(lib, N, F, T)
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=device)
    aux = torch.empty(N + 2, dtype=torch.int32, device=device)  # rowptr [N + 1] and the status word, read back as one pair
    rowptr, status = aux[:N + 1], aux[N + 1:]
    stream = ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)
    nbytes = 8.0 * (2 * 3 * N + 9 * F) + 4.0 * (8 * N + 3 * F)  # count pass: positions in, grid and row pointer out
    with torch.cuda.device(device), ktimer.region("nqa_neighbor_list_batched", nbytes):
        _nl_count(lib, pos64, cell64, pbc32, r_max, N, ws, ws_bytes, rowptr, stream, frame_ptr=frame_ptr, types=types,
                  table=table.on(device) if table is not None else None, status=status)
        E, bad = aux[N:].tolist()  # the one synchronisation: the edge count is data dependent
        _raise_for_status(E, bad, T)
        edge_index = torch.empty((2, E), dtype=torch.int64, device=device)
        shifts = torch.empty((E, 3), dtype=torch.float64, device=device)
        _nl_fill(lib, ws, rowptr, N, E, edge_index, shifts, stream, F=F, types=types, T=T)
    return edge_index, shifts.to(pos.dtype), rowptr


def _concat_rowptrs(rowptrs: List[torch.Tensor], edge_counts: List[int]) -> torch.Tensor:
    """Row pointer [N + 1] of the concatenation of per-frame lists from their row pointers and edge counts."""
    if len(rowptrs) == 1:
        return rowptrs[0]
    parts, eoff = [], 0
    for rp, e in zip(rowptrs, edge_counts):
        parts.append(rp[:-1] + eoff)
        eoff += e
    parts.append(torch.tensor([eoff], dtype=torch.int32, device=rowptrs[0].device))
    return torch.cat(parts).to(torch.int32)


def _per_frame_requested() -> bool:
    return os.environ.get("NQA_NL_PER_FRAME", "") not in ("", "0")


def compute_neighborlist_(data: AtomicDataDict.Type, r_max: float, backend: str = DEFAULT_NEIGHBORLIST_BACKEND,
                          per_edge_type_cutoff=None, type_names: Optional[List[str]] = None) -> AtomicDataDict.Type:
    """Add a neighbour list to ``data`` in place (contract of ``nequip/data/_nl.py:364-381``).  Batched data: one batched list
    (``NQA_NL_PER_FRAME=1``: one list per frame, concatenated; the same result).  ``per_edge_type_cutoff``: the typed list
    (needs ``atom_types`` in ``data``); the topology hint is the row pointer of the pruned list."""
    if backend not in NEIGHBORLIST_BACKEND_OPTIONS:
        supported = ", ".join(f"`{b}`" for b in NEIGHBORLIST_BACKEND_OPTIONS)
        raise ValueError(f"Unknown neighborlist backend = `{backend}`. Supported backends: {supported}")
    K = AtomicDataDict
    table = as_cutoff_table(per_edge_type_cutoff, type_names, r_max)
    if table is not None and K.ATOM_TYPE_KEY not in data:
        raise KeyError(_MISSING_TYPES_MSG)
    batched = K.BATCH_KEY in data
    if batched and not _per_frame_requested():
        return _compute_neighborlist_batched_(data, r_max, table)
    nframes = K.num_frames(data)
    if batched:
        counts = data[K.NUM_NODES_KEY].view(-1).cpu().tolist() if K.NUM_NODES_KEY in data else torch.bincount(
            data[K.BATCH_KEY], minlength=nframes).cpu().tolist()
    else:
        counts = [data[K.POSITIONS_KEY].shape[0]]
    offsets = [0]
    for c in counts:
        offsets.append(offsets[-1] + int(c))
    has_cell = data.get(K.CELL_KEY, None) is not None
    eidx, shifts, rowptrs = [], [], []
    for f in range(nframes):
        frame = _frame_from_batched(data, f, offsets)
        cell = frame.get(K.CELL_KEY, None)
        pbc = frame.get(K.PBC_KEY, None)
        if pbc is None:
            pbc = False
        ei, sh, rp = _compute_neighborlist_single_frame(frame[K.POSITIONS_KEY], r_max, cell=cell, pbc=pbc,
                                                        return_rowptr=True, atom_types=frame.get(K.ATOM_TYPE_KEY, None),
                                                        per_edge_type_cutoff=table)
        eidx.append(ei + offsets[f])
        rowptrs.append(rp)
        shifts.append(sh)
    data[K.EDGE_INDEX_KEY] = torch.cat(eidx, dim=1) if len(eidx) > 1 else eidx[0]
    # the list is grouped by centre atom: give the tensor-product kernels its row pointer (saves the dst sort)
    from ..nn._topology import topology_cache

    topology_cache.hint_sorted(data[K.EDGE_INDEX_KEY], _concat_rowptrs(rowptrs, [int(ei.shape[1]) for ei in eidx]))
    if has_cell:
        data[K.EDGE_CELL_SHIFT_KEY] = torch.cat(shifts, dim=0) if len(shifts) > 1 else shifts[0]
    return data


def _compute_neighborlist_batched_(data: AtomicDataDict.Type, r_max: float,
                                   table: Optional[CutoffTable] = None) -> AtomicDataDict.Type:
    K = AtomicDataDict
    pos = data[K.POSITIONS_KEY]
    F = _batched_frame_count(data)
    frame_ptr = _frame_ptr(data, F, pos.device)
    cell = data.get(K.CELL_KEY, None)
    edge_index, shifts, rowptr = _compute_neighborlist_batched(pos, r_max, frame_ptr, cell=cell, pbc=data.get(K.PBC_KEY, None),
                                                               atom_types=data.get(K.ATOM_TYPE_KEY, None),
                                                               per_edge_type_cutoff=table)
    data[K.EDGE_INDEX_KEY] = edge_index
    from ..nn._topology import topology_cache

    topology_cache.hint_sorted(edge_index, rowptr)
    if cell is not None:
        data[K.EDGE_CELL_SHIFT_KEY] = shifts
    return data


NEIGHBORLIST_BACKEND_OPTIONS: Final[Dict[str, object]] = {NEIGHBORLIST_BACKEND_NEQUIP_AMD: compute_neighborlist_}
