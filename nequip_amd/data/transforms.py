"""Neighbour-list transforms (the interface of ``nequip/data/transforms/neighborlist.py:9-117``).

``NeighborListTransform(r_max, per_edge_type_cutoff, type_names, backend)`` adds the device neighbour list to a data dict; with
``per_edge_type_cutoff`` the list is typed on the device (``nqa_neighbor_list_*_typed``): the pruned list is what the search
emits, where the reference builds the full list and masks it.  ``NeighborListPruneTransform`` masks a list that already exists
(from any source, on any device, CPU tensors included) together with every registered per-edge field, by the same rule: the edge
``i <- j`` stays iff ``|r_ij| <= cutoff[type_i][type_j]``.

``cutoff_table_from_model`` is what the calculators use to find a model's table (``basic_transforms``,
``nequip/integrations/utils.py:28-70``, reads the same metadata key).
"""

from typing import Dict, List, Optional, Union

import torch

from . import AtomicDataDict
from ._key_registry import _EDGE_FIELDS
from ._nl import DEFAULT_NEIGHBORLIST_BACKEND, CutoffTable, _MISSING_TYPES_MSG, as_cutoff_table, compute_neighborlist_

PER_EDGE_TYPE_CUTOFF_KEY = "per_edge_type_cutoff"
CutoffSpec = Union[Dict[str, Union[float, Dict[str, float]]], torch.Tensor, CutoffTable]


class NeighborListTransform(torch.nn.Module):
    """Builds the neighbour list on the device and adds it to the data dict.

    Args:
        r_max: cutoff radius
        per_edge_type_cutoff: optional per-edge-type cutoffs (``<= r_max``): a dict as the model builders take it, a
            ``[T, T]`` table (rows = centre type) or a ``CutoffTable``
        type_names: atom type names (needed for a dict)
        backend: neighbour-list backend (``"nequip_amd"``)
    """

    def __init__(self, r_max: float, per_edge_type_cutoff: Optional[CutoffSpec] = None,
                 type_names: Optional[List[str]] = None, backend: str = DEFAULT_NEIGHBORLIST_BACKEND):
        super().__init__()
        self.r_max = float(r_max)
        self.backend = backend
        self.type_names = None if type_names is None else list(type_names)
        self.per_edge_type_cutoff = per_edge_type_cutoff
        if isinstance(per_edge_type_cutoff, dict):
            assert type_names is not None, "`type_names` required for `per_edge_type_cutoff`"
        self._table = as_cutoff_table(per_edge_type_cutoff, self.type_names, self.r_max)

    def forward(self, data: AtomicDataDict.Type) -> AtomicDataDict.Type:
        return compute_neighborlist_(data, self.r_max, backend=self.backend, per_edge_type_cutoff=self._table)


class NeighborListPruneTransform(torch.nn.Module):
    """Prunes an existing neighbour list by per-edge-type cutoffs (pure torch: any device).

    Args:
        r_max: global cutoff radius
        per_edge_type_cutoff: per-edge-type cutoffs (``<= r_max``)
        type_names: atom type names
    """

    def __init__(self, r_max: float, per_edge_type_cutoff: CutoffSpec, type_names: Optional[List[str]] = None):
        super().__init__()
        self.r_max = float(r_max)
        self.per_edge_type_cutoff = per_edge_type_cutoff
        self.type_names = None if type_names is None else list(type_names)
        table = as_cutoff_table(per_edge_type_cutoff, self.type_names, self.r_max)
        if table is None:
            raise ValueError("NeighborListPruneTransform needs `per_edge_type_cutoff`")
        self.num_types = table.num_types
        self.register_buffer("_cutoffs", table.table.clone().view(-1), persistent=False)

    def keep_mask(self, data: AtomicDataDict.Type) -> torch.Tensor:
        """bool ``[E]``: ``|r_ij| <= cutoff[type_i][type_j]`` (lengths in float64 from positions, cell and shifts)."""
        K = AtomicDataDict
        if K.ATOM_TYPE_KEY not in data:
            raise KeyError(_MISSING_TYPES_MSG)
        ei = data[K.EDGE_INDEX_KEY]
        if K.EDGE_VECTORS_KEY in data:
            vec = data[K.EDGE_VECTORS_KEY].to(torch.float64)
        else:
            pos = data[K.POSITIONS_KEY].to(torch.float64)
            vec = pos.index_select(0, ei[1]) - pos.index_select(0, ei[0])
            if K.EDGE_CELL_SHIFT_KEY in data and data.get(K.CELL_KEY, None) is not None:
                cell = data[K.CELL_KEY].to(torch.float64).view(-1, 3, 3)
                shifts = data[K.EDGE_CELL_SHIFT_KEY].to(torch.float64)
                if cell.shape[0] > 1:
                    frame = data[K.BATCH_KEY].view(-1).index_select(0, ei[0])
                    vec = vec + torch.einsum("ni,nij->nj", shifts, cell.index_select(0, frame))
                else:
                    vec = vec + shifts @ cell[0]
        types = data[K.ATOM_TYPE_KEY].view(-1).to(torch.int64)
        if types.numel() and (int(types.min()) < 0 or int(types.max()) >= self.num_types):
            raise ValueError(f"atom_types holds a type index outside [0, {self.num_types})")
        rc = self._cutoffs.to(vec.device).index_select(
            0, types.index_select(0, ei[0]) * self.num_types + types.index_select(0, ei[1]))
        return torch.linalg.norm(vec, dim=-1) <= rc

    def forward(self, data: AtomicDataDict.Type) -> AtomicDataDict.Type:
        K = AtomicDataDict
        mask = self.keep_mask(data)
        data[K.EDGE_INDEX_KEY] = data[K.EDGE_INDEX_KEY][:, mask]
        for field in list(data.keys()):
            if field != K.EDGE_INDEX_KEY and field in _EDGE_FIELDS:
                data[field] = data[field][mask]
        return data


def cutoff_table_from_model(model: torch.nn.Module, r_max: float) -> Optional[CutoffTable]:
    """The per-edge-type cutoff table of ``model`` as a checked ``CutoffTable``, or ``None`` for a model without one: from
    ``model.metadata["per_edge_type_cutoff"]`` (``T * T`` values, row-major), else from the model's own
    ``EdgeLengthNormalizer`` (a model that is not wrapped in a ``GraphModel``)."""
    metadata = getattr(model, "metadata", None)
    text = metadata.get(PER_EDGE_TYPE_CUTOFF_KEY, None) if isinstance(metadata, dict) else None
    if text:
        values = [float(x) for x in str(text).split()]
        T = int(round(len(values) ** 0.5))
        if T * T != len(values):
            raise ValueError(f"per_edge_type_cutoff metadata holds {len(values)} values: not a square table")
        return CutoffTable(torch.tensor(values, dtype=torch.float64).view(T, T), r_max)
    from ..nn.embedding import EdgeLengthNormalizer

    for m in model.modules():
        if isinstance(m, EdgeLengthNormalizer) and m._per_edge_type:
            table = m._rmax_recip.detach().to("cpu", torch.float64).reciprocal().view(m.num_types, m.num_types)
            return CutoffTable(table.clamp(max=float(r_max)), r_max)
    return None
