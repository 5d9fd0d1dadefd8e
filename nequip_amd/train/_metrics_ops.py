"""Host driver of the fused loss / metric reduction (``nqa_metrics_fwd`` / ``nqa_metrics_bwd``, csrc/metrics.hip).

A ``FusedPlan`` holds what is fixed for a ``MetricsManager`` (or for one stand-alone metric): the TERMS (one metric on one
stream each), their slots (one per group: 1, or one per atom type), where each returned value sits in the value vector, and per
device the term table, the workspace of partial sums and the running epoch state -- allocated once.  ``evaluate`` takes the
STREAMS of a call (prediction, target, optional per-row scale, optional group index) and returns the float64 value vector:

* GPU tensors: two launches forward, one backward, inside one ``torch.autograd.Function``; nothing is read by the host, so the
  call captures into ``torch.cuda.graph``.  A missing library raises (``_lib.load``).  (``epoch_values``, behind
  ``compute()``, is the exception by design: once per epoch it copies the state to the host and finishes there.)
* CPU tensors: ``_aten_forward``, the same arithmetic as vectorised ATen operations without boolean indexing
  (differentiated by autograd), so that the host logic is testable without a GPU.

Max-abs terms are metrics, not losses: they are computed detached and receive no gradient.  Targets never receive one.
"""

from __future__ import annotations

import dataclasses
import math
from typing import List, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..utils._slot_plan import SlotPlan, canonical_row_scale, canonical_rows, membership

MSE, MAE, RMSE, MAXABS, HUBER, STRATIFIED_HUBER = range(6)
MAX_STREAMS, MAX_TERMS = _lib.NQA_METRICS_MAX_STREAMS, _lib.NQA_METRICS_MAX_TERMS
MAX_TYPES, MAX_STRATA = _lib.NQA_METRICS_MAX_TYPES, _lib.NQA_METRICS_MAX_STRATA
NUM_WORKGROUPS = _lib.NQA_METRICS_GROUPS  # workgroups (= rows of partials) of the first forward launch

# (pred, target, row_scale or None, group or None) of one stream
StreamInput = Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor], Optional[torch.Tensor]]


@dataclasses.dataclass
class TermSpec:
    stream: int
    kind: int
    n_groups: int = 1
    ignore_nan: bool = False
    reduce_sum: bool = False
    delta: float = 1.0
    strata: Optional[List[Tuple[float, float]]] = None  # (lower bound, delta), in the order given
    coeff: Optional[float] = None
    group_coeffs: Optional[List[float]] = None
    slot0: int = 0  # filled by FusedPlan
    out0: int = 0

    @property
    def n_values(self) -> int:
        return self.n_groups + 1 if self.n_groups > 1 else 1

    @property
    def value_index(self) -> int:
        """Index of the term's own value (the aggregate of a per-type term)."""
        return self.out0 + (self.n_groups if self.n_groups > 1 else 0)


class FusedPlan(SlotPlan):
    """Terms in the caller's order (= order of the returned values); the device table is ordered by stream."""

    MAX_STREAMS, MAX_TERMS = MAX_STREAMS, MAX_TERMS
    TOO_MANY_STREAMS = "{n} distinct prediction/target pairs: the fused metric kernels take at most {max}"
    TOO_MANY_TERMS = "{n} metric terms: the fused metric kernels take at most {max}"
    TERM_STRUCT, WORKSPACE_BYTES = _lib.MetricTerm, "nqa_metrics_workspace_bytes"
    PLANES = (("sum", torch.float64, 0.0), ("count", torch.int64, 0), ("max", torch.float64, -math.inf))

    def __init__(self, terms: Sequence[TermSpec], n_streams: int):
        super().__init__(terms, n_streams)
        out = 0
        for t in self.terms:
            t.out0 = out
            out += t.n_values
        self.n_term_values = out
        self.table_version = 0  # counts coeffs_changed: a backward must see the table its forward saw
        self.last_device: Optional[torch.device] = None

    def check_terms(self) -> None:
        for t in self.terms:
            if t.n_groups > MAX_TYPES:
                raise ValueError(f"{t.n_groups} atom types: per-type metrics take at most {MAX_TYPES}")
            if t.kind == STRATIFIED_HUBER and not 2 <= len(t.strata) <= MAX_STRATA:
                raise ValueError(f"{len(t.strata)} strata: the stratified Huber loss takes 2 to {MAX_STRATA}")

    # ---- what depends on the coefficients --------------------------------------------------------------------------------
    @property
    def ws_index(self) -> int:
        return self.n_term_values  # (the last entry is weighted_sum: 0 while no term carries a coefficient)

    @property
    def n_values(self) -> int:
        return self.n_term_values + 1

    def coeffs_changed(self) -> None:
        """Rewrite the term tables IN PLACE: a captured graph keeps reading the same device buffer."""
        self._host_table = None
        self.table_version += 1
        for dev, bufs in self._dev.items():
            if dev.type == "cuda":
                bufs["table"].copy_(self._table_tensor())

    @staticmethod
    def fill_row(c, t: TermSpec) -> None:
        c.stream, c.kind, c.n_groups, c.ignore_nan = t.stream, t.kind, t.n_groups, int(t.ignore_nan)
        c.reduce_sum, c.slot0, c.out0 = int(t.reduce_sum), t.slot0, t.out0
        c.has_coeff, c.coeff = int(t.coeff is not None), float(t.coeff or 0.0)
        c.delta = float(t.delta)
        strata = t.strata or []
        c.n_strata = len(strata)
        for j, (b, d) in enumerate(strata):
            c.bound[j], c.stratum_delta[j] = float(b), float(d)
        c.has_group_coeffs = int(t.group_coeffs is not None)
        for j, g in enumerate(t.group_coeffs or []):
            c.group_coeff[j] = float(g)

    def _table_tensor(self) -> torch.Tensor:
        raw = bytes(memoryview(self.host_table()).cast("B"))
        return torch.frombuffer(bytearray(raw), dtype=torch.uint8)

    def device_buffers(self, bufs: dict, device: torch.device) -> None:
        bufs["table"] = self._table_tensor().to(device)

    def state(self, device=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Copies of the running (sum, count, max) per slot, over every device this plan has run on."""
        device = torch.device(device) if device is not None else (self.last_device or torch.device("cpu"))
        S = self.n_slots
        s = torch.zeros(S, dtype=torch.float64, device=device)
        c = torch.zeros(S, dtype=torch.int64, device=device)
        m = torch.full((S,), -math.inf, dtype=torch.float64, device=device)
        for bufs in self._dev.values():
            s = s + bufs["sum"].to(device)
            c = c + bufs["count"].to(device)
            m = torch.maximum(m, bufs["max"].to(device))
        return s, c, m

    # ---- evaluation ------------------------------------------------------------------------------------------------------
    def evaluate(self, streams: Sequence[StreamInput], accumulate: bool = True, force_aten: bool = False) -> torch.Tensor:
        """The float64 value vector ``[n_values]`` of one batch (term values at ``TermSpec.out0``, weighted_sum last).
        ``force_aten``: the ATen form on GPU tensors too (for ``scripts/bench_metrics.py``; never taken otherwise)."""
        assert len(streams) == self.n_streams
        streams = [_canonical(*s) for s in streams]
        device = streams[0][0].device
        self.last_device = device
        if device.type == "cuda" and not force_aten:
            preds = [s[0] for s in streams]
            rest = [x for s in streams for x in s[1:]]
            return _MetricsFn.apply(self, accumulate, len(streams), *preds, *rest)
        return _aten_forward(self, streams, accumulate)

    def epoch_values(self, state: Tuple[torch.Tensor, torch.Tensor, torch.Tensor]) -> torch.Tensor:
        """The value vector of the accumulated state: every configured type enters an aggregate, NaN propagates.  Done on
        the host (a synchronisation, once per epoch): a step never comes here."""
        device = state[0].device
        s, c, m = (x.cpu() for x in state)  # (one small copy; a dozen scalar operations are not worth launches)
        out = torch.full((self.n_values,), math.nan, dtype=torch.float64)
        ws = 0.0
        for t in self.terms:
            sl = slice(t.slot0, t.slot0 + t.n_groups)
            v = _slot_values(t, s[sl], c[sl], m[sl])
            if t.n_groups > 1:
                out[t.out0:t.out0 + t.n_groups] = v
                w = torch.ones_like(v) if t.group_coeffs is None else torch.tensor(t.group_coeffs, dtype=torch.float64)
                tv = (w * v).sum() / w.sum()
            else:
                tv = v[0]
            out[t.value_index] = tv
            if t.coeff is not None:
                ws = ws + tv * t.coeff
        out[self.ws_index] = ws
        return out.to(device)


def _slot_values(t: TermSpec, s, c, m):
    if t.kind == MAXABS:
        return m
    if t.kind in (HUBER, STRATIFIED_HUBER) and t.reduce_sum:
        return s
    mean = s / c  # (no element: 0 / 0 = NaN)
    return mean.sqrt() if t.kind == RMSE else mean


def _canonical(pred, target, row_scale, group) -> StreamInput:
    """[rows, cols] contiguous float32 / float64 on both sides, float64 scale, int64 groups."""
    if pred.shape != target.shape:
        pred, target = torch.broadcast_tensors(pred, target)
    pred, target = canonical_rows(pred), canonical_rows(target.detach().to(pred.device))
    rows = pred.shape[0]
    row_scale = canonical_row_scale(row_scale, rows, pred.device)
    if group is not None:
        group = group.detach().to(device=pred.device, dtype=torch.int64).reshape(-1).contiguous()
        assert group.numel() == rows, "one group index per row (per-type metrics are for per-atom fields)"
    return pred, target, row_scale, group


# ---- GPU: the HIP kernels --------------------------------------------------------------------------------------------------
_DT = {torch.float32: _lib.NQA_F32, torch.float64: _lib.NQA_F64}


def _stream_array(streams: Sequence[StreamInput], grads: Optional[Sequence[Optional[torch.Tensor]]] = None):
    arr = (_lib.MetricStream * len(streams))()
    for i, (p, t, sc, g) in enumerate(streams):
        c = arr[i]
        c.pred, c.target = p.data_ptr(), t.data_ptr()
        c.row_scale = sc.data_ptr() if sc is not None else None
        c.group = g.data_ptr() if g is not None else None
        c.grad_pred = grads[i].data_ptr() if grads is not None and grads[i] is not None else None
        c.rows, c.cols = p.shape
        c.pred_dtype, c.target_dtype = _DT[p.dtype], _DT[t.dtype]
    return arr


class _MetricsFn(torch.autograd.Function):
    """``(pred_0, ..., pred_{n-1}) -> values``: ``nqa_metrics_fwd`` (two launches), backward ``nqa_metrics_bwd`` (one)."""

    @staticmethod
    def forward(ctx, plan: FusedPlan, accumulate: bool, n: int, *tensors):
        lib = _lib.load()
        preds, rest = tensors[:n], tensors[n:]
        streams = [(preds[i], rest[3 * i], rest[3 * i + 1], rest[3 * i + 2]) for i in range(n)]
        dev = preds[0].device
        bufs = plan.buffers(dev)
        values = torch.empty(plan.n_values, dtype=torch.float64, device=dev)
        saved = torch.empty(2 * plan.n_slots, dtype=torch.int64, device=dev)  # [2, S]: batch sums (f64), counts (i64)
        host = plan.host_table()
        with torch.cuda.device(dev):
            rc = lib.nqa_metrics_fwd(_stream_array(streams), n, host, _lib.ptr(bufs["table"]), len(plan.terms), plan.n_values,
                                     plan.ws_index, _lib.ptr(bufs["workspace"]), bufs["workspace_bytes"],
                                     _lib.ptr(bufs["state"]) if accumulate else None, _lib.ptr(saved), _lib.ptr(values),
                                     _lib.stream_ptr(dev))
        _lib.check(rc, "nqa_metrics_fwd")
        ctx.plan, ctx.n, ctx.host, ctx.ws_index, ctx.table_version = plan, n, host, plan.ws_index, plan.table_version
        ctx.save_for_backward(saved, *tensors)
        return values

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        saved, *tensors = ctx.saved_tensors
        plan, n = ctx.plan, ctx.n
        if plan.table_version != ctx.table_version:
            # the device table is rewritten in place (a captured graph keeps reading it): the gradient would pair the new
            # coefficients with values formed under the old ones
            raise RuntimeError("the metric coefficients were changed (set_coeffs) between this backward and its forward; "
                               "change them between steps")
        preds, rest = tensors[:n], tensors[n:]
        streams = [(preds[i], rest[3 * i], rest[3 * i + 1], rest[3 * i + 2]) for i in range(n)]
        grads = [torch.empty_like(p) if ctx.needs_input_grad[3 + i] else None for i, p in enumerate(preds)]
        dev = preds[0].device
        g = g.to(torch.float64).contiguous()
        with torch.cuda.device(dev):
            rc = _lib.load().nqa_metrics_bwd(_stream_array(streams, grads), n, ctx.host, _lib.ptr(plan.buffers(dev)["table"]),
                                             len(plan.terms), plan.n_values, ctx.ws_index, _lib.ptr(saved), _lib.ptr(g),
                                             _lib.stream_ptr(dev))
        _lib.check(rc, "nqa_metrics_bwd")
        return (None, None, None, *grads) + (None,) * len(rest)


# ---- CPU: the same arithmetic in ATen ----------------------------------------------------------------------------------------
def _huber(d, delta):
    """``|d| < delta ? d^2 / 2 : delta (|d| - delta / 2)`` for a float or per-row ``delta``; the branch not taken is kept
    finite (an infinite delta would put 0 * inf into its gradient)."""
    a = d.abs()
    delta = torch.as_tensor(delta, dtype=d.dtype, device=d.device)
    quad = a < delta
    dl = torch.where(quad, torch.ones_like(a), delta.expand_as(a))
    return torch.where(quad, 0.5 * d * d, dl * (a - 0.5 * dl))


def _element_values(t: TermSpec, d, target):
    if t.kind in (MSE, RMSE):
        return d * d
    if t.kind == MAE:
        return d.abs()
    if t.kind == MAXABS:
        return d.abs().detach()
    if t.kind == HUBER:
        return _huber(d, t.delta)
    norm = target.square().sum(-1).sqrt()
    delta = torch.ones_like(norm)
    found = torch.zeros_like(norm, dtype=torch.bool)
    for i, (b, dl) in enumerate(t.strata):
        hit = norm >= b
        if i + 1 < len(t.strata):
            hit = hit & ~(norm >= t.strata[i + 1][0])
        delta = torch.where(hit, torch.full_like(norm, dl), delta)
        found = found | hit
    return torch.where(found[:, None], _huber(d, delta[:, None]), torch.zeros_like(d))


def _aten_forward(plan: FusedPlan, streams: Sequence[StreamInput], accumulate: bool) -> torch.Tensor:
    dev = streams[0][0].device
    bufs = plan.buffers(dev)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    values: List[Optional[torch.Tensor]] = [None] * plan.n_values
    ws = zero
    for i in plan.table_order:
        t = plan.terms[i]
        pred, target, scale, group = streams[t.stream]
        p, tg = pred.to(torch.float64), target.to(torch.float64)  # promoted BEFORE the subtraction
        if scale is not None:
            p, tg = p * scale[:, None], tg * scale[:, None]
        contrib = ~torch.isnan(target) if t.ignore_nan else torch.ones_like(target, dtype=torch.bool)
        d = p - tg
        if t.ignore_nan:  # a masked element must not reach the modifier: its derivative there could be NaN
            d = torch.where(contrib, d, torch.zeros_like(d))
        v = _element_values(t, d, tg)
        member = membership(group if t.n_groups > 1 else None, t.n_groups, contrib)
        cnt = member.sum((1, 2))
        if t.kind == MAXABS:
            mx = torch.where(member, v[None], torch.full_like(v, -math.inf)[None]).flatten(1)
            mx = torch.cat([mx, torch.full((mx.shape[0], 1), -math.inf, dtype=torch.float64, device=dev)], 1).amax(1)
            sm = torch.zeros_like(mx)
        else:
            sm = torch.where(member, v[None], torch.zeros_like(v)[None]).sum((1, 2))
            mx = torch.full_like(sm, -math.inf)
        if accumulate:
            sl = slice(t.slot0, t.slot0 + t.n_groups)
            bufs["sum"][sl] += sm.detach()
            bufs["count"][sl] += cnt
            bufs["max"][sl] = torch.maximum(bufs["max"][sl], mx)
        # slot values: an empty slot must not put 0 / 0 into the gradient
        has = cnt > 0
        safe = torch.where(has, cnt, torch.ones_like(cnt)).to(torch.float64)
        nan = torch.full_like(sm, math.nan)
        if t.kind == MAXABS:
            sv = mx
        elif t.kind in (HUBER, STRATIFIED_HUBER) and t.reduce_sum:
            sv = sm
        elif t.kind == RMSE:
            sv = torch.where(has, torch.where(has, sm / safe, torch.ones_like(sm)).sqrt(), nan)
        else:
            sv = torch.where(has, sm / safe, nan)
        if t.n_groups > 1:
            for g in range(t.n_groups):
                values[t.out0 + g] = sv[g]
            ok = ~torch.isnan(sv.detach())
            w = (torch.ones_like(sv) if t.group_coeffs is None
                 else torch.tensor(t.group_coeffs, dtype=torch.float64, device=dev))
            tv = torch.where(ok, w * sv, torch.zeros_like(sv)).sum() / torch.where(ok, w, torch.zeros_like(w)).sum()
        else:
            tv = sv[0]
        values[t.value_index] = tv
        if t.coeff is not None:
            ws = ws + tv * t.coeff
    values[-1] = ws
    return torch.stack(values)
