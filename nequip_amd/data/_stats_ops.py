"""Host driver of the fused statistics reduction (``nqa_stats_update`` / ``nqa_stats_neighbor_counts``, csrc/stats.hip).

A ``StatsPlan`` holds what is fixed for a ``DataStatisticsManager``: the TERMS (one entry on one stream each), their slots (one
per group: 1, T for a per-type node term, T^2 for a per-type edge term) and per device the workspace of partial states, the
neighbour-count workspace and the running state -- allocated once.  The state of a slot is ``count`` (int64) and ``mean``,
``mean_lo``, ``M2 = sum (y - mean)^2``, ``min``, ``max`` (float64) of ``y = m(x)``, ``m`` the term's element modifier; every
metric kind is formed from it in ``compute()``.  The mean is ``mean + mean_lo`` -- the rounded value and what the rounding lost
-- because Chan's merge squares the DIFFERENCE of two means: held in one double each, means of 1e6 carry an error of 1e-10 and
data with a spread of 1e-2 would leave the merged M2 with nine digits.  ``update`` takes the STREAMS of a batch
(``StreamInput``):

* GPU tensors: two launches for any number of terms and types (plus a memset and one launch when neighbours are counted);
  nothing is read by the host, so the call captures into ``torch.cuda.graph``.  A missing library raises (``_lib.load``).
* CPU tensors: ``_aten_update``, the same arithmetic as vectorised ATen operations without boolean indexing (batch mean, a
  second pass about it for its correction and M2, Chan's merge into the running state), so that the host logic is testable
  without a GPU.

Merging two states (``merge``: a batch into the running state, the states of several devices, the states of the ranks of a
process group) is Chan's parallel formula: ``n = na + nb``, ``delta = mean_b - mean_a`` (formed as ``(hi_b - hi_a) + (lo_b -
lo_a)``), ``mean = mean_a + delta nb / n`` (renormalised by a two-sum), ``M2 = M2_a + M2_b + delta^2 na nb / n``; minima and
maxima keep a NaN; an empty side leaves the other one unchanged.
"""

from __future__ import annotations

import dataclasses
import math
from typing import List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..utils._slot_plan import SlotPlan, canonical_row_scale, canonical_rows, membership

IDENTITY, ABS, SQUARE = _lib.NQA_STATS_MOD_IDENTITY, _lib.NQA_STATS_MOD_ABS, _lib.NQA_STATS_MOD_SQUARE
GROUP_NONE, GROUP_NODE, GROUP_EDGE = _lib.NQA_STATS_GROUP_NONE, _lib.NQA_STATS_GROUP_NODE, _lib.NQA_STATS_GROUP_EDGE
MAX_STREAMS, MAX_TERMS, MAX_SLOTS = _lib.NQA_STATS_MAX_STREAMS, _lib.NQA_STATS_MAX_TERMS, _lib.NQA_STATS_MAX_SLOTS
MAX_NODE_TYPES, MAX_EDGE_TYPES = _lib.NQA_STATS_MAX_NODE_TYPES, _lib.NQA_STATS_MAX_EDGE_TYPES
NUM_WORKGROUPS = _lib.NQA_STATS_GROUPS  # workgroups (= rows of partial states) of the first launch

# count, mean, mean_lo, M2, min, max: [slots] each
State = Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]


class StreamInput(NamedTuple):
    data: torch.Tensor  # any shape with the rows first
    row_scale: Optional[torch.Tensor] = None  # [rows]
    atom_types: Optional[torch.Tensor] = None  # grouped streams
    edge_index: Optional[torch.Tensor] = None  # edge streams: [2, rows]


@dataclasses.dataclass
class TermSpec:
    stream: int
    mod: int
    per_type: bool = False
    ignore_nan: bool = False
    n_groups: int = 1  # filled by StatsPlan
    slot0: int = 0


class StatsPlan(SlotPlan):
    """Terms in the caller's order; the table handed to the kernels is ordered by stream.  ``group_kinds[s]`` says how the
    per-type terms of stream ``s`` are grouped (``GROUP_NONE`` / ``GROUP_NODE`` / ``GROUP_EDGE``)."""

    MAX_STREAMS, MAX_TERMS, MAX_SLOTS = MAX_STREAMS, MAX_TERMS, MAX_SLOTS
    TOO_MANY_STREAMS = "{n} distinct fields: the statistics kernels take at most {max} (NQA_STATS_MAX_STREAMS)"
    TOO_MANY_TERMS = "{n} statistics entries: the statistics kernels take at most {max} (NQA_STATS_MAX_TERMS)"
    TOO_MANY_SLOTS = "{n} groups over all entries: the statistics kernels take at most {max} (NQA_STATS_MAX_SLOTS)"
    TERM_STRUCT, WORKSPACE_BYTES = _lib.StatsTerm, "nqa_stats_workspace_bytes"
    PLANES = (("count", torch.int64, 0), ("mean", torch.float64, 0.0), ("mean_lo", torch.float64, 0.0),
              ("m2", torch.float64, 0.0), ("min", torch.float64, math.inf), ("max", torch.float64, -math.inf))

    def __init__(self, terms: Sequence[TermSpec], group_kinds: Sequence[int], num_types: int = 0):
        self.group_kinds, self.num_types = list(group_kinds), int(num_types)
        super().__init__(terms, len(self.group_kinds))

    def check_terms(self) -> None:
        num_types = self.num_types
        for t in self.terms:
            kind = self.group_kinds[t.stream]
            if t.per_type:
                assert kind != GROUP_NONE, "a per-type term needs a node or edge stream"
                if kind == GROUP_NODE and num_types > MAX_NODE_TYPES:
                    raise ValueError(f"{num_types} atom types: per-type node statistics take at most {MAX_NODE_TYPES} "
                                     "(NQA_STATS_MAX_NODE_TYPES)")
                if kind == GROUP_EDGE and num_types > MAX_EDGE_TYPES:
                    raise ValueError(f"{num_types} atom types: per-type edge statistics take at most {MAX_EDGE_TYPES} "
                                     "(NQA_STATS_MAX_EDGE_TYPES)")
                t.n_groups = num_types if kind == GROUP_NODE else num_types * num_types
            else:
                t.n_groups = 1

    @staticmethod
    def fill_row(c, t: TermSpec) -> None:
        c.stream, c.mod, c.n_groups, c.ignore_nan, c.slot0 = t.stream, t.mod, t.n_groups, int(t.ignore_nan), t.slot0

    def device_buffers(self, bufs: dict, device: torch.device) -> None:
        bufs["counts"] = torch.empty(0, dtype=torch.int32, device=device)

    def device_state(self, device) -> State:
        """Views of the running state on one device (no copy)."""
        b = self.buffers(device)
        return b["count"], b["mean"], b["mean_lo"], b["m2"], b["min"], b["max"]

    def state(self) -> State:
        """The running state on the host: one copy per device this plan has run on, merged in the order of first use."""
        out = empty_state(self.n_slots)
        for bufs in self._dev.values():
            host = bufs["state"].cpu()  # (one copy)
            planes = host[self.n_slots:].view(torch.float64).view(5, self.n_slots)
            out = merge(out, (host[:self.n_slots], *planes.unbind(0)))
        return out

    # ---- neighbour counts ----------------------------------------------------------------------------------------------------
    def neighbor_counts(self, edge_index: torch.Tensor, num_atoms: int) -> torch.Tensor:
        """``[num_atoms]`` number of edges each atom is the centre of (``edge_index[0]``, in any order): int32 in the plan's
        workspace on the GPU (``nqa_stats_neighbor_counts``; the buffer is kept while it is large enough, so a captured graph
        keeps its address), int64 on the CPU."""
        center = edge_index[0].to(torch.int64).contiguous()
        dev = center.device
        if dev.type != "cuda":
            return torch.zeros(num_atoms, dtype=torch.int64).index_add_(0, center, torch.ones_like(center))
        bufs = self.buffers(dev)
        if bufs["counts"].numel() < num_atoms:
            bufs["counts"] = torch.empty(num_atoms, dtype=torch.int32, device=dev)
        counts = bufs["counts"][:num_atoms]
        with torch.cuda.device(dev):
            rc = _lib.load().nqa_stats_neighbor_counts(_lib.ptr(center), center.numel(), num_atoms, _lib.ptr(counts),
                                                       _lib.stream_ptr(dev))
        _lib.check(rc, "nqa_stats_neighbor_counts")
        return counts

    # ---- update ----------------------------------------------------------------------------------------------------------------
    def update(self, streams: Sequence[StreamInput], force_aten: bool = False) -> None:
        """Merge one batch into the running state of the streams' device.  ``force_aten``: the ATen form on GPU tensors too
        (for ``scripts/bench_data_statistics.py``; never taken otherwise)."""
        assert len(streams) == len(self.group_kinds)
        streams = [_canonical(s, k, self.num_types) for s, k in zip(streams, self.group_kinds)]
        device = streams[0].data.device
        assert all(s.data.device == device for s in streams), "the fields of one batch live on one device"
        if device.type == "cuda" and not force_aten:
            self._hip_update(streams, device)
        else:
            _aten_update(self, streams, device)

    def _hip_update(self, streams: Sequence[StreamInput], device: torch.device) -> None:
        lib = _lib.load()
        bufs = self.buffers(device)
        arr = (_lib.StatsStream * len(streams))()
        for c, s, kind in zip(arr, streams, self.group_kinds):
            c.data = s.data.data_ptr()
            c.row_scale = s.row_scale.data_ptr() if s.row_scale is not None else None
            c.atom_types = s.atom_types.data_ptr() if s.atom_types is not None else None
            c.edge_index = s.edge_index.data_ptr() if s.edge_index is not None else None
            c.rows, c.cols = s.data.shape
            c.num_atoms = s.atom_types.numel() if s.atom_types is not None else 0
            c.dtype, c.group_kind, c.num_types = _DT[s.data.dtype], kind, self.num_types
        with torch.cuda.device(device):
            rc = lib.nqa_stats_update(arr, len(streams), self.host_table(), len(self.terms), _lib.ptr(bufs["workspace"]),
                                      bufs["workspace_bytes"], _lib.ptr(bufs["state"]), _lib.stream_ptr(device))
        _lib.check(rc, "nqa_stats_update")


_DT = {torch.float32: _lib.NQA_STATS_F32, torch.float64: _lib.NQA_STATS_F64, torch.int32: _lib.NQA_STATS_I32,
       torch.int64: _lib.NQA_STATS_I64}


def _canonical(s: StreamInput, kind: int, num_types: int) -> StreamInput:
    """[rows, cols] contiguous float32 / float64 / int32 / int64 data, float64 scale, int64 types and edge index."""
    data = canonical_rows(s.data.detach(), keep=tuple(_DT), integers=torch.int64)
    rows, dev = data.shape[0], data.device
    scale = canonical_row_scale(s.row_scale, rows, dev)
    types = edge_index = None
    if kind != GROUP_NONE and s.atom_types is not None:
        types = s.atom_types.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if kind == GROUP_NODE:
            assert types.numel() == rows, "one atom type per row of a per-atom field"
        else:
            edge_index = s.edge_index.detach().to(device=dev, dtype=torch.int64).contiguous()
            assert edge_index.shape == (2, rows), "one column of edge_index per row of a per-edge field"
    return StreamInput(data, scale, types, edge_index)


# ---- states on the host / in ATen ------------------------------------------------------------------------------------------
def empty_state(n_slots: int, device=None) -> State:
    z = torch.zeros(n_slots, dtype=torch.float64, device=device)
    return (torch.zeros(n_slots, dtype=torch.int64, device=device), z, z.clone(), z.clone(), torch.full_like(z, math.inf),
            torch.full_like(z, -math.inf))


def _two_sum(hi: torch.Tensor, lo: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """``hi + lo`` as (rounded sum, what the rounding lost); a sum that is not finite keeps no remainder."""
    s = hi + lo
    b = s - hi
    e = (hi - (s - b)) + (lo - b)
    return s, torch.where(torch.isfinite(s), e, torch.zeros_like(e))


def merge(a: State, b: State) -> State:
    """``a`` followed by ``b`` (Chan), slot by slot; an empty side leaves the other one bit for bit."""
    na, ha, la, qa, mna, mxa = a
    nb, hb, lb, qb, mnb, mxb = b
    n = na + nb
    delta = (hb - ha) + (lb - la)
    change = delta * (nb.to(torch.float64) / n.clamp(min=1).to(torch.float64))
    hi, lo = _two_sum(ha, la + change)
    m2 = qa + qb + delta * change * na.to(torch.float64)
    keep_a, keep_b = nb == 0, na == 0
    hi = torch.where(keep_a, ha, torch.where(keep_b, hb, hi))
    lo = torch.where(keep_a, la, torch.where(keep_b, lb, lo))
    m2 = torch.where(keep_a, qa, torch.where(keep_b, qb, m2))
    return n, hi, lo, m2, torch.minimum(mna, mnb), torch.maximum(mxa, mxb)  # (both keep a NaN)


def _groups(s: StreamInput, kind: int, num_types: int) -> torch.Tensor:
    """[rows] group index, -1 for a type or an atom index out of range (as the kernel)."""
    types = s.atom_types
    if kind == GROUP_NODE:
        return torch.where((types >= 0) & (types < num_types), types, torch.full_like(types, -1))
    n = types.numel()
    ei = s.edge_index
    ok = ((ei >= 0) & (ei < n)).all(0)
    t = torch.index_select(types, 0, ei.clamp(0, max(n - 1, 0)).reshape(-1)).view(2, -1)
    ok = ok & ((t >= 0) & (t < num_types)).all(0)
    return torch.where(ok, t[0] * num_types + t[1], torch.full_like(t[0], -1))


def _aten_update(plan: StatsPlan, streams: Sequence[StreamInput], device: torch.device) -> None:
    state = plan.device_state(device)
    inf = math.inf
    for i in plan.table_order:
        t = plan.terms[i]
        s, kind = streams[t.stream], plan.group_kinds[t.stream]
        if s.data.numel() == 0:
            continue
        x = s.data.to(torch.float64)  # promoted first
        if s.row_scale is not None:
            x = x * s.row_scale[:, None]
        y = x.abs() if t.mod == ABS else (x * x if t.mod == SQUARE else x)
        contrib = ~torch.isnan(x) if t.ignore_nan else torch.ones_like(x, dtype=torch.bool)
        member = membership(_groups(s, kind, plan.num_types) if t.per_type else None, t.n_groups, contrib)
        yb = y[None]
        cnt = member.sum((1, 2))
        safe = cnt.clamp(min=1).to(torch.float64)
        zero = torch.zeros_like(yb)
        b_mean = torch.where(member, yb, zero).sum((1, 2)) / safe
        dev = torch.where(member, yb - b_mean[:, None, None], zero)  # second pass about the batch mean:
        b_lo = dev.sum((1, 2)) / safe  # what the first pass lost of the mean,
        b_m2 = torch.where(member, (dev - b_lo[:, None, None]).square(), zero).sum((1, 2))  # and M2 about the corrected mean
        b_mean, b_lo = _two_sum(b_mean, b_lo)
        pad = torch.full((member.shape[0], 1), inf, dtype=torch.float64, device=device)
        b_min = torch.cat([torch.where(member, yb, torch.full_like(yb, inf)).flatten(1), pad], 1).amin(1)
        b_max = torch.cat([torch.where(member, yb, torch.full_like(yb, -inf)).flatten(1), -pad], 1).amax(1)
        sl = slice(t.slot0, t.slot0 + t.n_groups)
        new = merge(tuple(x[sl] for x in state), (cnt, b_mean, b_lo, b_m2, b_min, b_max))
        for dst, src in zip(state, new):
            dst[sl] = src
