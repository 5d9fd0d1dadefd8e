"""Field modifiers: what a metric entry of ``MetricsManager`` is computed on (the interface of ``nequip/data/modifier.py``).

A modifier turns the ``(preds, target)`` data dicts into the pair of tensors to compare, names itself for automatic metric
names (``str(modifier)``) and says whether its field is per-frame, per-atom or per-edge (``modifier.type``).
``MetricsManager`` recognises the three classes below and hands their tensors to the fused reduction directly --
``PerAtomModifier`` as the raw field plus a per-row scale ``factor / num_atoms``, so the normalised copies are never
materialised.  A subclass that overrides ``_func`` or ``__call__`` is called as it is.

``NumNeighbors`` and ``EdgeLengths`` are for ``DataStatisticsManager`` (one dict).  ``NumNeighbors`` differs from the reference
on purpose: there the counts come compacted out of ``torch.unique`` and zeros are padded at the END, so an isolated atom in the
middle of the index range shifts every later count to the wrong atom (and the wrong type); here atom ``i`` gets its own count.
The mean over all atoms is the same either way.
"""

from typing import Optional

import torch

from . import AtomicDataDict, _key_registry


def _short(field: str) -> str:
    return _key_registry.ABBREV.get(field, field)


class BaseModifier:
    """The field itself, from both dicts."""

    def __init__(self, field: str) -> None:
        self.field = field

    def _func(self, data: AtomicDataDict.Type) -> torch.Tensor:
        return data[self.field]

    def __call__(self, data1: AtomicDataDict.Type, data2: Optional[AtomicDataDict.Type] = None):
        """One dict: its tensor (data statistics); two dicts: ``(from data1, from data2)`` (metrics)."""
        first = self._func(data1)
        return first if data2 is None else (first, self._func(data2))

    def __str__(self) -> str:
        return _short(self.field)

    @property
    def type(self) -> str:
        return _key_registry.get_field_type(self.field)


class PerAtomModifier(BaseModifier):
    """A per-frame field divided by the frame's number of atoms, times an optional ``factor`` (unit conversion)."""

    def __init__(self, field: str, factor: Optional[float] = None) -> None:
        assert field in _key_registry._GRAPH_FIELDS
        super().__init__(field)
        self._factor = factor

    def row_scale(self, data: AtomicDataDict.Type) -> torch.Tensor:
        """``[num_frames]`` float64: ``factor / num_atoms`` -- the per-row scale of the fused reduction."""
        scale = data[AtomicDataDict.NUM_NODES_KEY].reshape(-1).to(torch.float64).reciprocal()
        return scale if self._factor is None else self._factor * scale

    def _func(self, data: AtomicDataDict.Type) -> torch.Tensor:
        x = data[self.field]
        inv = data[AtomicDataDict.NUM_NODES_KEY].reshape(-1).reciprocal()
        x = x * inv.reshape((-1,) + (1,) * (x.dim() - 1))
        return x if self._factor is None else self._factor * x

    def __str__(self) -> str:
        return "per_atom_" + _short(self.field)


class MappedFieldModifier(BaseModifier):
    """Predictions from one field, targets from another of the same kind."""

    def __init__(self, pred_field: str, target_field: str) -> None:
        super().__init__(pred_field)
        self.pred_field, self.target_field = pred_field, target_field
        kinds = [_key_registry.get_field_type(f) for f in (pred_field, target_field)]
        assert kinds[0] == kinds[1], (
            f"`pred_field` ({pred_field}) and `target_field` ({target_field}) must have the same field type, but got "
            f"`{kinds[0]}` and `{kinds[1]}`")
        self._type = kinds[0]

    def __call__(self, data1: AtomicDataDict.Type, data2: Optional[AtomicDataDict.Type] = None):
        pred = data1[self.pred_field]
        return pred if data2 is None else (pred, data2[self.target_field])

    def __str__(self) -> str:
        return f"pred_{_short(self.pred_field)}_label_{_short(self.target_field)}"

    @property
    def type(self) -> str:
        return self._type


class EdgeLengths(BaseModifier):
    """``[E, 1]`` edge lengths, from positions, cell and shifts through ``with_edge_vectors_`` (which also leaves the vectors
    and lengths in ``data``)."""

    def __init__(self) -> None:
        super().__init__(AtomicDataDict.EDGE_INDEX_KEY)

    def _func(self, data: AtomicDataDict.Type) -> torch.Tensor:
        from ..nn.utils import with_edge_vectors_

        return with_edge_vectors_(data, with_lengths=True)[AtomicDataDict.EDGE_LENGTH_KEY]

    def __str__(self) -> str:
        return "edge_lengths"

    @property
    def type(self) -> str:
        return "edge"


class NumNeighbors(BaseModifier):
    """``[N]`` number of edges that each atom is the centre of, for an edge list in any order; an atom without edges has 0 at
    its own index.  GPU tensors: ``nqa_stats_neighbor_counts`` (int32; the statistics manager makes the same call into a
    workspace of its own); CPU tensors: ATen (int64)."""

    def __init__(self) -> None:
        super().__init__(AtomicDataDict.EDGE_INDEX_KEY)

    def _func(self, data: AtomicDataDict.Type) -> torch.Tensor:
        center = data[AtomicDataDict.EDGE_INDEX_KEY][0].to(torch.int64).contiguous()
        n = data[AtomicDataDict.POSITIONS_KEY].shape[0]
        if not center.is_cuda:
            return torch.zeros(n, dtype=torch.int64).index_add_(0, center, torch.ones_like(center))
        from .. import _lib

        counts = torch.empty(n, dtype=torch.int32, device=center.device)
        with torch.cuda.device(center.device):
            rc = _lib.load().nqa_stats_neighbor_counts(_lib.ptr(center), center.numel(), n, _lib.ptr(counts),
                                                       _lib.stream_ptr(center.device))
        _lib.check(rc, "nqa_stats_neighbor_counts")
        return counts

    def __str__(self) -> str:
        return "num_neighbors"

    @property
    def type(self) -> str:
        return "node"
