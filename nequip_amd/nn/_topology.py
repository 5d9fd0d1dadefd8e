"""Edge topology (CSR by destination and by source) shared by all layers of one model evaluation.

The reference passes raw ``edge_index`` rows to every ``TensorProductScatter.forward``
(``nequip/nn/interaction_block.py:193-199``) and lets ATen gather/scatter with them
(``nequip/nn/_tp_scatter_base.py:36-37``, ``nequip/nn/utils.py:42-51``).  The fused kernels instead
walk per-node edge lists, so the (unsorted, possibly repeated) int64 indices are grouped once on the
device by ``nqa_csr_build`` and reused by the three convolution layers and their backward passes.
"""

from __future__ import annotations

import contextlib
import os
import weakref
from typing import Optional, Tuple

import torch

from .. import _lib


_ptr, current_stream_ptr = _lib.ptr, _lib.stream_ptr


class EdgeTopology:
    """CSR views of one edge list.  ``by_dst`` drives forward / edge gradients, ``by_src`` the feature gradient."""

    check_indices: bool = False  # set True to validate 0 <= index < num_nodes (costs a device sync)
    # Deferred pairing verdict (set per instance by a caller that cannot synchronise: a hipGraph capture of a whole MD step,
    # ``integrations/graphed_step.py``): ``pairing`` launches the kernels and hands out the pairing WITHOUT reading the flag;
    # ``pairing_ok`` is the device flag the caller reads after the evaluation (0 = the list did not pair up, results void -- the
    # indices stay in range and the pair-centric kernels get empty lists, ``nqa_pair_owner_lists_guard``).
    defer_pairing_verdict: bool = False
    pairing_ok: Optional[torch.Tensor] = None

    def __init__(self, edge_dst: torch.Tensor, edge_src: torch.Tensor, num_nodes: int,
                 rowptr_dst: Optional[torch.Tensor] = None, csr_dst=None):
        if not edge_dst.is_cuda:
            raise RuntimeError(
                "nequip_amd kernels run on the GPU only (got CPU index tensors); there is no CPU fallback"
            )
        assert edge_dst.dtype == torch.int64 and edge_src.dtype == torch.int64, "edge indices must be int64"
        assert edge_dst.dim() == 1 and edge_dst.shape == edge_src.shape
        self.device = edge_dst.device
        self.num_nodes = int(num_nodes)
        self.num_edges = int(edge_dst.numel())
        self._dst = edge_dst.contiguous()
        self._src = edge_src.contiguous()
        self._by_dst: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
        self._by_src: Optional[Tuple[torch.Tensor, torch.Tensor, torch.Tensor]] = None
        self._dst_is_identity = False  # the dst-CSR lists the edges in edge order (a list grouped by centre atom)
        self._side_ready: Optional[torch.cuda.Event] = None  # see prefetch_backward_lists
        self._pair_ready: Optional[torch.cuda.Event] = None
        if csr_dst is not None and csr_dst[0].numel() == self.num_nodes + 1:
            # (the neighbour list handed over its complete dst-CSR: row pointer, edge ids in order, int32 neighbours)
            self._by_dst = tuple(csr_dst)
            self._dst_is_identity = True
        elif rowptr_dst is not None and rowptr_dst.numel() == self.num_nodes + 1:
            # edges already grouped by destination in ascending order (the device neighbour list emits them that way and
            # hands over its row pointer): the dst-CSR is the identity permutation, no sort needed
            eid = torch.arange(max(self.num_edges, 1), dtype=torch.int32, device=self.device)
            oth = self._src.to(torch.int32) if self.num_edges else torch.zeros(1, dtype=torch.int32, device=self.device)
            self._by_dst = (rowptr_dst, eid, oth)
            self._dst_is_identity = True

    def _build(self, key: torch.Tensor, other: torch.Tensor):
        lib = _lib.load()
        N, E = self.num_nodes, self.num_edges
        dev = self.device
        rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        eid = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        oth = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        ws_bytes = lib.nqa_csr_workspace_bytes(N, E)
        if ws_bytes < 0:
            raise RuntimeError("edge list exceeds the int32 index range supported by the kernels")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        status = torch.zeros(1, dtype=torch.int32, device=dev) if self.check_indices else None
        with torch.cuda.device(dev):
            rc = lib.nqa_csr_build(
                _ptr(key), _ptr(other), N, E, _ptr(rowptr), _ptr(eid), _ptr(oth), _ptr(status), _ptr(ws),
                ws_bytes, current_stream_ptr(dev),
            )  # fmt: skip
        _lib.check(rc, "nqa_csr_build")
        if status is not None and int(status.item()) != 0:
            raise RuntimeError("edge index out of range [0, num_nodes)")
        return rowptr, eid, oth

    @staticmethod
    def _shift_key(shifts: Optional[torch.Tensor]):
        return None if shifts is None else (shifts.data_ptr(), shifts._version, tuple(shifts.shape))

    def start_pairing(self, shifts: Optional[torch.Tensor]) -> None:
        """Launch the pairing kernels NOW and start copying their verdict to pinned host memory; ``pairing()`` then only
        waits for that copy.  Called at the top of an evaluation (``GraphModel.forward``), so that the verdict's round trip to
        the host overlaps with the launches of the embedding and the first node kernels instead of stalling the queue in front
        of the first convolution (what a new neighbour list per step -- MD -- pays on every step).  No-op when the pairing of
        this list is known, running, switched off or cannot be read (hipGraph capture)."""
        key = self._shift_key(shifts)
        cached = getattr(self, "_pairing", None)
        pending = getattr(self, "_pairing_pending", None)
        if (cached is not None and cached[0] == key) or (pending is not None and pending[0] == key):
            return
        E = self.num_edges
        if (E == 0 or E % 2 != 0 or os.environ.get("NQA_NO_PAIRED", "") not in ("", "0")
                or torch.cuda.is_current_stream_capturing() or self.defer_pairing_verdict):
            return
        dev = self.device
        rows, rep, partner, ok = self._launch_pairing(shifts)
        with torch.cuda.device(dev):
            verdict = torch.empty(1, dtype=torch.int32, pin_memory=True)
            verdict.copy_(ok, non_blocking=True)
            done = torch.cuda.Event()
            done.record(torch.cuda.current_stream(dev))
        self._pairing_pending = (key, rows, rep, partner, verdict, done, ok)

    def _launch_pairing(self, shifts: Optional[torch.Tensor], zero_rep: bool = False):
        """``nqa_edge_pairs`` on the current stream: ``(weight_rows, rep_edge, partner, ok)`` device tensors, nothing read."""
        lib = _lib.load()
        dev = self.device
        E = self.num_edges
        sh = None
        if shifts is not None:
            sh = shifts.detach()
            if sh.dtype not in (torch.float32, torch.float64):
                sh = sh.to(torch.float64)
            sh = sh.contiguous()
        rows = torch.empty(E, dtype=torch.int32, device=dev)
        partner = torch.empty(E, dtype=torch.int32, device=dev)
        # (deferred verdict: a pair number the kernels never assign must still name an edge)
        rep = (torch.zeros if zero_rep else torch.empty)(E // 2, dtype=torch.int64, device=dev)
        ok = torch.empty(1, dtype=torch.int32, device=dev)  # (initialised by nqa_edge_pairs)
        ws_bytes = lib.nqa_edge_pairs_workspace_bytes(E)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
        sdt = _lib.NQA_F32 if (sh is not None and sh.dtype == torch.float32) else _lib.NQA_F64
        rowptr, eid, nbr = self.by_dst  # (the reverse of (i <- j) is looked up in row j of the dst-CSR: no sort)
        with torch.cuda.device(dev):
            # (edge ids NULL = "in edge order": a list grouped by centre atom, one load less per look-up)
            rc = lib.nqa_edge_pairs(_ptr(self._dst), _ptr(self._src), _ptr(sh), sdt, _ptr(rowptr),
                                    _ptr(None if self._dst_is_identity else eid), _ptr(nbr),
                                    E, self.num_nodes, _ptr(ws), ws_bytes, _ptr(rows), _ptr(rep), _ptr(partner),
                                    _ptr(ok), current_stream_ptr(dev))
            _lib.check(rc, "nqa_edge_pairs")
        return rows, rep, partner, ok

    def pairing_if_known(self, shifts: Optional[torch.Tensor]):
        """``pairing(shifts)`` when its verdict has been read already (no wait, no launch), else ``None``."""
        cached = getattr(self, "_pairing", None)
        if cached is not None and cached[0] == self._shift_key(shifts):
            self._wait_pair()
            return cached[1]
        if self.defer_pairing_verdict:  # (nothing to wait for: the flag is read after the evaluation)
            return self.pairing(shifts)
        return None

    def pairing(self, shifts: Optional[torch.Tensor]):
        """Reverse-edge pairing of this list (``nqa_edge_pairs``): ``None`` when some edge has no unique reverse
        partner, else an ``EdgePairing`` with the weight rows in the slot order of both CSRs.  Computed once per
        topology (one wait for the verdict -- a host synchronisation unless ``start_pairing`` ran early enough)."""
        key = self._shift_key(shifts)
        cached = getattr(self, "_pairing", None)
        if cached is not None and cached[0] == key:
            self._wait_pair()
            return cached[1]
        if self.defer_pairing_verdict:
            if (self.num_edges == 0 or self.num_edges % 2 != 0
                    or os.environ.get("NQA_NO_PAIRED", "") not in ("", "0")):
                self._pairing = (key, None)
                return None
            rows, rep, partner, ok = self._launch_pairing(shifts, zero_rep=True)
            result = EdgePairing(self, rows, rep)
            result.partner = partner
            result.ok_flag = ok
            self.pairing_ok = ok
            self._pairing = (key, result)
            return result
        if torch.cuda.is_current_stream_capturing():
            return None  # reading the verdict needs a synchronisation: not inside a hipGraph capture (not cached)
        self.start_pairing(shifts)
        result = None
        pending = getattr(self, "_pairing_pending", None)
        if pending is not None and pending[0] == key:
            _, rows, rep, partner, verdict, done, _ok = pending
            self._pairing_pending = None
            done.synchronize()
            if int(verdict[0]) == 1:
                result = EdgePairing(self, rows, rep)
                result.partner = partner
        self._pairing = (key, result)
        return result

    def prefetch_backward_lists(self, shifts: Optional[torch.Tensor], side: "torch.cuda.Stream") -> None:
        """Build what only the backward pass reads -- the by-source CSR, the owner lists of the pair-centric kernels, the
        weight rows in by-source order -- on ``side`` NOW, next to the forward pass on the current stream, instead of lazily in
        front of their first consumer (~0.1 ms of small launches at 400 k edges that a new list per step would otherwise pay
        on the critical path).  Every later access waits for ``side`` on the stream it is made from.  For callers that know
        the pairing without waiting (a deferred verdict, or a verdict already read)."""
        if self._side_ready is not None:
            return
        cur = torch.cuda.current_stream(self.device)
        if os.environ.get("NQA_PAIR_ON_MAIN", "") not in ("", "0"):  # (experiment: only the backward's lists on `side`)
            self.pairing_if_known(shifts)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            # (a deferred verdict: the pairing itself starts here too, next to the edge vectors / type embedding on `cur`)
            pairing = self.pairing_if_known(shifts)
            paired = torch.cuda.Event()
            paired.record(side)
            self._pair_ready = paired
            if pairing is not None:
                self.by_src
                pairing.owner_csr
                pairing.slots_src
                ready = torch.cuda.Event()
                ready.record(side)
                self._side_ready = ready

    def _side_tensors(self):
        """Everything ``prefetch_backward_lists`` allocated on the side stream (the caching allocator ties a block to the
        stream it was allocated on: a consumer on another stream has to be recorded, or an evicted topology's lists could be
        handed out again while that consumer's kernels still read them)."""
        out = []
        cached = getattr(self, "_pairing", None)
        pairing = cached[1] if cached is not None else None
        if pairing is not None:
            out += [pairing.rows, pairing.rep_edge, pairing.partner, pairing._slots_src, pairing._slots_dst]
            if pairing._owner_csr is not None:
                out += list(pairing._owner_csr)
        if self._by_src is not None:
            out += list(self._by_src)
        return [t for t in out if isinstance(t, torch.Tensor) and t.is_cuda]

    def _record_side(self, cur) -> None:
        if torch.cuda.is_current_stream_capturing():
            return  # (inside a capture the graph owns the memory; GraphedStep keeps the topology alive)
        seen = self.__dict__.setdefault("_side_recorded", set())
        key = (cur.cuda_stream, self._side_ready is not None)
        if key in seen:
            return
        seen.add(key)
        for t in self._side_tensors():
            t.record_stream(cur)

    def _wait_pair(self) -> None:
        if self._pair_ready is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._pair_ready)
            self._record_side(cur)

    def _wait_side(self) -> None:
        if self._side_ready is not None:
            cur = torch.cuda.current_stream(self.device)
            cur.wait_event(self._side_ready)
            self._record_side(cur)

    @property
    def by_dst(self):
        if self._by_dst is None:
            self._by_dst = self._build(self._dst, self._src)
        return self._by_dst

    @property
    def by_src(self):
        self._wait_side()
        if self._by_src is None:
            paired = getattr(self, "_pairing", None)
            if paired is not None and paired[1] is not None and self._by_dst is not None and self.num_edges > 0:
                # a paired list: row j of the by-source CSR holds the partners of the edges of row j of the dst-CSR
                rowptr, eid, nbr = self._by_dst
                eid_s = torch.empty_like(eid)
                with torch.cuda.device(self.device):
                    rc = _lib.load().nqa_csr_from_pairs(_ptr(eid), _ptr(paired[1].partner), self.num_edges, _ptr(eid_s),
                                                        current_stream_ptr(self.device))
                _lib.check(rc, "nqa_csr_from_pairs")
                self._by_src = (rowptr, eid_s, nbr)
            else:
                self._by_src = self._build(self._src, self._dst)
        return self._by_src


def owner_lists(topo: "EdgeTopology", pairing: "EdgePairing"):
    """``nqa_pair_owner_lists``: the owner lists on the device, from the pairing and the dst-CSR.  Same content as
    ``build_owner_csr`` below (the host-side statement of the rule, tested on the CPU) up to the order of the slots within a
    node, which here is the CSR order."""
    lib = _lib.load()
    E, N, P = topo.num_edges, topo.num_nodes, pairing.num_pairs
    dev = topo.device
    rowptr, eid, nbr = topo.by_dst
    i32 = lambda n: torch.empty(max(n, 1), dtype=torch.int32, device=dev)  # noqa: E731
    owner_rowptr, other_rowptr = i32(N + 1), i32(N + 1)
    pair_other, pair_row, e_in, e_out, other_slot = i32(P), i32(P), i32(P), i32(P), i32(P)
    ws_bytes = lib.nqa_pair_owner_workspace_bytes(E, N)
    if ws_bytes < 0:
        raise RuntimeError("edge list exceeds the int32 index range supported by the kernels")
    ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        rc = lib.nqa_pair_owner_lists(_ptr(pairing.rows), _ptr(pairing.rep_edge), _ptr(rowptr), _ptr(eid), _ptr(nbr), E, N,
                                      _ptr(ws), ws_bytes, _ptr(owner_rowptr), _ptr(pair_other), _ptr(pair_row), _ptr(e_in),
                                      _ptr(e_out), _ptr(other_rowptr), _ptr(other_slot), current_stream_ptr(dev))
    _lib.check(rc, "nqa_pair_owner_lists")
    ok = getattr(pairing, "ok_flag", None)
    if ok is not None:  # deferred verdict: empty lists for a list that did not pair up
        with torch.cuda.device(dev):
            rc = lib.nqa_pair_owner_lists_guard(_ptr(ok), N, _ptr(owner_rowptr), _ptr(other_rowptr), current_stream_ptr(dev))
        _lib.check(rc, "nqa_pair_owner_lists_guard")
    return owner_rowptr, pair_other, pair_row, e_in, e_out, other_rowptr, other_slot


def build_owner_csr(edge_dst: torch.Tensor, edge_src: torch.Tensor, rows: torch.Tensor, num_pairs: int, num_nodes: int):
    """Owner lists of the pair-centric backward from a paired edge list (``rows[e]`` = p for the representative edge of pair
    p, p + P for its reverse).  Pure index arithmetic (a few sorts, no synchronisation; runs on any device -- the host
    logic is tested on the CPU).  Owner of the pair {i <- j, j <- i}: i when ``(i < j) xor (i + j odd)``, a self image
    pair (i == j) belongs to i.  Returns int32 tensors ``(owner_rowptr [N+1], pair_other, pair_row, edge_in, edge_out,
    other_rowptr [N+1], other_slot)``: slots grouped by owner (within an owner by the other node), ``edge_in`` /
    ``edge_out`` the directed edges with dst = owner / dst = other, ``other_slot`` the slots grouped by their other node."""
    P, N = int(num_pairs), int(num_nodes)
    dev = rows.device
    order = torch.argsort(rows.to(torch.int64))  # rows are a permutation of 0 .. 2P-1
    ea, eb = order[:P], order[P:]  # representative edge and its reverse, in pair order
    i, j = edge_dst.index_select(0, ea), edge_src.index_select(0, ea)
    own_i = (i == j) | ((i < j) ^ (((i + j) & 1) == 1))
    owner, other = torch.where(own_i, i, j), torch.where(own_i, j, i)
    e_in, e_out = torch.where(own_i, ea, eb), torch.where(own_i, eb, ea)  # dst = owner / dst = other
    perm = torch.argsort(owner * N + other, stable=True)  # (stable: several periodic images of one neighbour tie)
    owner_s, other_s = owner.index_select(0, perm), other.index_select(0, perm)
    nodes = torch.arange(N + 1, dtype=torch.int64, device=dev)
    owner_rowptr = torch.searchsorted(owner_s, nodes).to(torch.int32)
    perm2 = torch.argsort(other_s, stable=True)
    other_rowptr = torch.searchsorted(other_s.index_select(0, perm2), nodes).to(torch.int32)
    i32 = lambda t: t.to(torch.int32).contiguous()  # noqa: E731
    return (owner_rowptr.contiguous(), i32(other_s), i32(perm), i32(e_in.index_select(0, perm)),
            i32(e_out.index_select(0, perm)), other_rowptr.contiguous(), i32(perm2))


class EdgePairing:
    """Weight rows of a paired edge list: ``rows[e]`` (see include/nequip_amd.h ``nqa_edge_pairs``), gathered into the
    slot order of the two CSRs on first use, and the representative edge of every pair."""

    def __init__(self, topo: EdgeTopology, rows: torch.Tensor, rep_edge: torch.Tensor):
        self.rows = rows
        self.rep_edge = rep_edge
        self.num_pairs = int(rep_edge.numel())
        self._topo = weakref.ref(topo)
        self.partner: Optional[torch.Tensor] = None  # int32 [E]: the reverse edge of every edge
        self.ok_flag: Optional[torch.Tensor] = None  # deferred verdict only: int32 [1] on the device (see EdgeTopology)
        self._slots_dst: Optional[torch.Tensor] = None
        self._slots_src: Optional[torch.Tensor] = None
        self._owner_csr = None

    @property
    def slots_dst(self) -> torch.Tensor:
        if self._slots_dst is None:
            topo = self._topo()
            if topo._dst_is_identity:  # slot k of the dst-CSR is edge k
                self._slots_dst = self.rows
            else:
                eid = topo.by_dst[1][: self.rows.numel()]
                self._slots_dst = self.rows.index_select(0, eid.to(torch.int64)).contiguous()
        return self._slots_dst

    @property
    def slots_src(self) -> torch.Tensor:
        self._topo()._wait_side()
        if self._slots_src is None:
            eid = self._topo().by_src[1][: self.rows.numel()]
            self._slots_src = self.rows.index_select(0, eid.to(torch.int64)).contiguous()
        return self._slots_src


    @property
    def owner_csr(self):
        """Pair lists of the pair-centric backward (``nqa_tp_scatter_bwd_pairs``): every pair gets an owner node --
        ``(i < j) xor (i + j odd)`` picks i, which hands every node about half of its pairs -- and the pairs are grouped by
        owner (within an owner by the other node, for the locality of the gathered rows) and, separately, by the other node.
        Returns int32 device tensors ``(owner_rowptr, pair_other, pair_row, edge_in, edge_out, other_rowptr, other_slot)``.
        Built once per neighbour list from the dst-CSR (``nqa_pair_owner_lists``: counting passes and prefix sums, no sort,
        no synchronisation; slots keep the CSR order)."""
        self._topo()._wait_side()
        if self._owner_csr is None:
            topo = self._topo()
            self._owner_csr = owner_lists(topo, self)
        return self._owner_csr


class _TopologyCache:
    """Reuse of the CSRs / pairing of an edge list: across the layers of one forward, and across forwards for as long as
    the caller keeps handing in the SAME index tensor (static neighbour list: benchmark loops, MD between list rebuilds).

    An entry is keyed on the identity of the index storage (which the entry keeps alive, so a recycled address cannot
    alias), with the same version counter, data pointer, size and strides.  What
    this cannot see is a caller that rewrites the index memory behind PyTorch's back (a DLPack / Kokkos view refilled
    by LAMMPS, ``.data`` writes, raw-pointer kernels): the version counter does not move and a stale CSR would give
    silently wrong forces.  Three guards:

    * ``scope(trust_identity=False)``: inside, nothing is taken from or left in the cross-call cache -- the topology is
      built on first use and shared by the layers of that one evaluation only.  ``GraphModel.forward`` opens such a
      scope for callers known to alias buffers (LAMMPS ML-IAP data) and when ``NQA_TOPOLOGY_CACHE=0``.
    * ``invalidate()`` / ``clear()`` for callers that know they rewrote a list in place.
    * ``NQA_TOPOLOGY_VERIFY=1``: every cache hit is checked against a checksum of the index values taken when the
      entry was built (one reduction + a host synchronisation per hit: a debugging mode) and raises on a mismatch.

    A few entries are kept (least recently used first out), so alternating graphs do not rebuild on every call.

    Memory: an entry holds the storage of the caller's int64 index tensors, both int32 CSRs and the pairing / owner
    lists -- about 100 bytes per directed edge, i.e. ~0.4 GB per cached graph at the 100 000-atom Cu box.  A driver that
    builds a new neighbour list every step (MD) therefore keeps the last ``MAX_ENTRIES`` graphs resident;
    ``NQA_TOPOLOGY_CACHE_ENTRIES=1`` (or ``topology_cache.MAX_ENTRIES = 1``) bounds that to the current graph."""

    MAX_ENTRIES = max(1, int(os.environ.get("NQA_TOPOLOGY_CACHE_ENTRIES", "4") or 4))

    def __init__(self):
        self._entries = []  # [(key, (ref_dst, ref_src), topo, checksum)] most recent last
        self._scope = None  # dict while an untrusted scope is open
        self._hint = None

    @staticmethod
    def _base(t: torch.Tensor) -> torch.Tensor:
        return t._base if t._base is not None else t

    def hint_sorted(self, edge_index: torch.Tensor, rowptr_dst: torch.Tensor, csr=None) -> None:
        """Called by the device neighbour list: `edge_index` ([2, E], rows = dst, src) is grouped by dst in ascending order
        and `rowptr_dst` ([N+1] int32) is its row pointer (`csr`: the complete dst-CSR ``(rowptr, edge ids, int32
        neighbours)`` when the list has it).  Used by the next `get` on views of that very tensor."""
        self._hint = (weakref.ref(edge_index), edge_index.data_ptr(), edge_index._version, rowptr_dst, csr)

    def _rowptr_hint(self, bd: torch.Tensor, edge_dst: torch.Tensor, num_nodes: int):
        hint = getattr(self, "_hint", None)
        if os.environ.get("NQA_NO_NL_HINT", "") not in ("", "0"):
            return None
        if hint is None or hint[0]() is not bd or bd.data_ptr() != hint[1] or bd._version != hint[2]:
            return None
        if edge_dst.data_ptr() != bd.data_ptr() or hint[3].numel() != num_nodes + 1:
            return None  # not row 0 of the hinted tensor
        return hint[3] if len(hint) < 5 or hint[4] is None else hint[4]

    @staticmethod
    def _checksum(edge_dst: torch.Tensor, edge_src: torch.Tensor) -> int:
        if edge_dst.numel() == 0:
            return 0
        pos = torch.arange(1, edge_dst.numel() + 1, device=edge_dst.device, dtype=torch.int64)
        return int(((edge_dst.to(torch.int64) * 1000003 + edge_src.to(torch.int64)) * pos).sum().item())

    @contextlib.contextmanager
    def scope(self, trust_identity: bool = True):
        """One model evaluation.  ``trust_identity=False``: build on first use, share within the scope, forget afterwards."""
        if trust_identity or self._scope is not None:
            yield self
            return
        self._scope = {}
        try:
            yield self
        finally:
            self._scope = None

    def get(self, edge_dst: torch.Tensor, edge_src: torch.Tensor, num_nodes: int) -> EdgeTopology:
        # identity of the STORAGE behind the two index tensors (the rule of csrc/torch_ops/nequip_amd_torch.cpp): every
        # `edge_index[0]` / `edge_index[1]` view of one input tensor maps to the same entry, whoever made the view -- the
        # model, an FX graph, or the AOTInductor runtime, whose views are new Python objects at every op call.  An entry
        # holds the two storages, so their addresses cannot be recycled under it.
        bd, bs = self._base(edge_dst), self._base(edge_src)
        sd, ss = edge_dst.untyped_storage(), edge_src.untyped_storage()
        key = (
            sd._cdata, ss._cdata, edge_dst._version, edge_src._version, edge_dst.data_ptr(), edge_src.data_ptr(),
            edge_dst.numel(), edge_dst.stride(0), edge_src.stride(0), int(num_nodes), str(edge_dst.device),
        )  # fmt: skip
        if self._scope is not None:  # untrusted caller: per-evaluation sharing only
            topo = self._scope.get(key)
            if topo is None:
                topo = self._scope[key] = EdgeTopology(edge_dst, edge_src, num_nodes)
            return topo
        verify = os.environ.get("NQA_TOPOLOGY_VERIFY", "") not in ("", "0")
        for i, (k, refs, topo, csum) in enumerate(self._entries):
            if k == key:
                if verify:
                    now = self._checksum(edge_dst, edge_src)
                    if csum is None:
                        self._entries[i] = (k, refs, topo, now)
                    elif now != csum:
                        raise RuntimeError(
                            "nequip_amd: the edge index tensor was rewritten in place without PyTorch noticing (same "
                            "tensor, same version counter, different contents): the cached CSR is stale.  Call "
                            "nequip_amd.nn.topology_cache.invalidate() after such writes, or hand in a new tensor.")
                if i != len(self._entries) - 1:
                    self._entries.append(self._entries.pop(i))
                return topo
        hint = self._rowptr_hint(bd, edge_dst, num_nodes)
        if isinstance(hint, tuple):
            topo = EdgeTopology(edge_dst, edge_src, num_nodes, csr_dst=hint)
        else:
            topo = EdgeTopology(edge_dst, edge_src, num_nodes, rowptr_dst=hint)
        self._entries.append((key, (sd, ss), topo, self._checksum(edge_dst, edge_src) if verify else None))
        while len(self._entries) > self.MAX_ENTRIES:
            self._entries.pop(0)
        return topo

    def forget(self, topo: EdgeTopology) -> None:
        """Drop one topology from the cross-call cache (its owner keeps it alive: a captured graph)."""
        self._entries = [e for e in self._entries if e[2] is not topo]

    def invalidate(self) -> None:
        """Forget every cached topology (after rewriting an index tensor in place)."""
        self._entries = []
        self._hint = None
        if self._scope is not None:
            self._scope.clear()

    def clear(self):
        self.invalidate()


topology_cache = _TopologyCache()
