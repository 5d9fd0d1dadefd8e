"""``TensorProductScatter`` on MI355X: fused gather -> Clebsch-Gordan 'uvu' product -> scatter-add.

Mirrors ``nequip.nn._tp_scatter_base.TensorProductScatter`` (``nequip/nn/_tp_scatter_base.py:9-38``):
same constructor arguments ``(feature_irreps_in, irreps_edge_attr, irreps_mid, instructions)``, same
``forward(x, edge_attr, edge_weight, edge_dst, edge_src)`` signature and semantics, the ``tp`` /
``model_dtype`` attributes and the ``_nequip_custom_ops_libs`` marker of the reference's accelerated
adapters (``nequip/nn/_tp_scatter_oeq.py:4-57``).  The arithmetic runs in the hand-written HIP kernels
of ``libnequip_amd.so`` (``include/nequip_amd.h``); there is no eager / CPU implementation in this
package -- a CPU tensor or a missing library raises.

Differentiability (``tests/unit/nn/test_tp_scatter_kernel.py:160-177`` for first order,
``nequip/nn/grad_output.py:217-221`` ``create_graph=self.training`` for second order): the op is
trilinear in ``(x, edge_attr, edge_weight)``, so its derivative kernels ``bwd_x`` / ``bwd_edge`` are
the same contraction with one operand replaced by a cotangent and the family
{fwd, bwd_x, bwd_edge} is closed under differentiation; double backward is expressed with the same
three kernels.
"""

from __future__ import annotations

import os
from typing import Optional, Tuple

import torch

from .. import _lib
from ..utils import ktimer
from ..o3.irreps import Irreps
from ..o3.tensor_product import NativePlan, TensorProduct
from ._topology import EdgeTopology, _ptr, current_stream_ptr, topology_cache


def _nqa_dtype(dtype: torch.dtype) -> int:
    if dtype == torch.float32:
        return _lib.NQA_F32
    if dtype == torch.float64:
        return _lib.NQA_F64
    raise RuntimeError(f"nequip_amd kernels support float32/float64 model dtypes, got {dtype}")


def _switched_off(name: str) -> bool:
    """An ``NQA_NO_...`` switch is set (to anything but the empty string or ``0``)?"""
    return os.environ.get(name, "") not in ("", "0")


class _Kernels:
    """Thin launcher around the native tensor-product entry points for one plan."""

    def __init__(self, plan: NativePlan, image: torch.Tensor):
        self.plan = plan
        self.image = image  # device uint8 tensor
        self.dim_in1 = plan.query(_lib.NQA_PLAN_DIM_IN1)
        self.dim_in2 = plan.query(_lib.NQA_PLAN_DIM_IN2)
        self.dim_out = plan.query(_lib.NQA_PLAN_DIM_OUT)
        self.weight_numel = plan.query(_lib.NQA_PLAN_WEIGHT_NUMEL)
        self.out_needs_zero = bool(plan.query(_lib.NQA_PLAN_OUT_NEEDS_ZERO))
        # The fused backward trades the per-edge gather of grad_out rows (dim_out) and a second read of the weights for
        # a per-edge row of grad_x contributions written and read once (2 * dim_in1): worth it for wide outputs only.
        self.prefer_fused_bwd = (self.weight_numel + self.dim_out) >= 3 * self.dim_in1
        # ... and only while the kernel's per-channel operands fit the register file (the pair-centric kernel, which is
        # split by input block for the wide structures, is not bound by this)
        self.fused_rows_ok = bool(plan.query(_lib.NQA_PLAN_FUSED_ROWS_OK))
        self._support = {}

    def _supports(self, kind: str, dtype: torch.dtype) -> bool:
        """Cached answer of the library for this plan: ``spec`` structure-specialised kernels (float32, uniform-mul NequIP
        shapes), ``pairs`` the pair-centric backward, ``jvp`` the one-pass second-order kernels, ``dual`` the dual
        pair-centric edge gradients."""
        if (kind, dtype) not in self._support:
            lib, h, dt = _lib.load(), self.plan.handle, _nqa_dtype(dtype)
            self._support[kind, dtype] = {
                "spec": lambda: lib.nqa_tp_bwd_fused_workspace_bytes(h, dt, 0) >= 0,
                "pairs": lambda: lib.nqa_tp_bwd_pairs_workspace_bytes(h, dt, 0) >= 0,
                "jvp": lambda: bool(lib.nqa_tp_fwd_jvp_supported(h, dt)),
                "dual": lambda: bool(lib.nqa_tp_bwd_pairs_dual_supported(h, dt)),
            }[kind]()
        return self._support[kind, dtype]

    def has_spec(self, dtype: torch.dtype) -> bool:
        return self._supports("spec", dtype)

    def has_pairs_kernel(self, dtype: torch.dtype) -> bool:
        return self._supports("pairs", dtype)

    def has_fwd_jvp(self, dtype: torch.dtype) -> bool:
        return self._supports("jvp", dtype)

    def has_dual_pairs_kernel(self, dtype: torch.dtype) -> bool:
        return self._supports("dual", dtype)

    def _call(self, name: str, pairing, slots: Optional[str], ref: torch.Tensor, *args) -> None:
        """``nqa_tp_scatter_<name>(plan, image, dtype, *args, stream)`` on ``ref``'s dtype and stream; tensors (or None)
        in ``args`` go by address, integers as they are.  With ``pairing``: the ``_paired`` entry point, which takes
        ``(pairing.<slots>, num_pairs)`` -- the weight row of every CSR slot -- before the stream."""
        fn = f"nqa_tp_scatter_{name}"
        argv = [self.plan.handle, _ptr(self.image), _nqa_dtype(ref.dtype)]
        argv += [a if isinstance(a, int) else _ptr(a) for a in args]
        if pairing is not None:
            argv += [_ptr(getattr(pairing, slots)), pairing.num_pairs]
        rc = getattr(_lib.load(), fn + ("_paired" if pairing is not None else ""))(*argv, current_stream_ptr(ref.device))
        _lib.check(rc, fn)

    def _check(self, x, y, w, topo: EdgeTopology, pairing=None):
        N, E = topo.num_nodes, topo.num_edges
        if x is not None:
            assert x.shape == (N, self.dim_in1), f"x has shape {tuple(x.shape)}, expected {(N, self.dim_in1)}"
        if y is not None:
            assert y.shape == (E, self.dim_in2), f"edge_attr has shape {tuple(y.shape)}, expected {(E, self.dim_in2)}"
        if w is not None:
            rows = E if pairing is None else pairing.num_pairs
            assert w.shape == (rows, self.weight_numel), (
                f"edge_weight has shape {tuple(w.shape)}, expected {(rows, self.weight_numel)}"
            )

    def fwd(self, x, y, w, topo: EdgeTopology, pairing=None) -> torch.Tensor:
        """``pairing`` (``EdgePairing``): ``w`` holds one row per reverse-edge pair (``nqa_tp_scatter_fwd_paired``)."""
        self._check(x, y, w, topo, pairing)
        alloc = torch.zeros if self.out_needs_zero else torch.empty
        out = alloc((topo.num_nodes, self.dim_out), dtype=x.dtype, device=x.device)
        csr = topo.by_dst
        es = x.element_size()
        nbytes = topo.num_edges * (es * (self.weight_numel + self.dim_in2) + 16) + topo.num_nodes * es * (
            self.dim_in1 + self.dim_out
        )
        with torch.cuda.device(x.device), ktimer.region("tp_fwd", nbytes, 0.0, topo.num_edges * es * self.weight_numel,
                                                        self.weight_numel):
            self._call("fwd", pairing, "slots_dst", x, x, y, w, *csr, out,
                       topo.num_nodes, topo.num_edges)
        return out

    def bwd_edge(self, x, y, w, g, topo: EdgeTopology, need_gw: bool, need_gy: bool, pairing=None, gw_out=None):
        """With ``pairing``: ``gw`` is ``[2 * num_pairs, weight_numel]`` (the two halves of every pair's gradient).
        ``gw_out``: caller-provided (contiguous) destination of ``gw`` -- lets several calls write slices of one buffer
        that is then reduced in a single pass."""
        self._check(x, y, w, topo, pairing)
        lib = _lib.load()
        E = topo.num_edges
        gw_rows = E if pairing is None else 2 * pairing.num_pairs
        gw = None
        if need_gw:
            if gw_out is not None:
                assert gw_out.shape == (gw_rows, self.weight_numel) and gw_out.is_contiguous() and gw_out.dtype == x.dtype
                gw = gw_out
            else:
                gw = torch.empty((gw_rows, self.weight_numel), dtype=x.dtype, device=x.device)
        gy = torch.empty((E, self.dim_in2), dtype=x.dtype, device=x.device) if need_gy else None
        if not (need_gw or need_gy):
            return None, None
        ws, ws_bytes = None, 0
        if need_gy:
            ws_bytes = lib.nqa_tp_bwd_edge_workspace_bytes(self.plan.handle, _nqa_dtype(x.dtype), E)
            ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        csr = topo.by_dst
        es = x.element_size()
        nbytes = E * (es * (self.weight_numel + self.dim_in2) + 16) + topo.num_nodes * es * (
            self.dim_in1 + self.dim_out
        )
        nbytes += E * es * ((self.weight_numel if need_gw else 0) + (self.dim_in2 if need_gy else 0))
        with torch.cuda.device(x.device), ktimer.region("tp_bwd_edge", nbytes, 0.0,
                                                        E * es * self.weight_numel * (2 if need_gw else 1), self.weight_numel):
            self._call("bwd_edge", pairing, "slots_dst", x, x, y, w, g, *csr, gw, gy, ws,
                       ws_bytes, topo.num_nodes, E)
        return gw, gy

    def bwd_fused(self, x, y, w, g, topo: EdgeTopology, need_gw: bool = True, need_gy: bool = True, pairing=None):
        """(gx, gw, gy) in one pass over ``g`` (``nqa_tp_scatter_bwd_fused``), or None when the plan has no
        structure-specialised float32 kernel (the caller then uses bwd_x + bwd_edge)."""
        lib = _lib.load()
        E, N = topo.num_edges, topo.num_nodes
        ws_bytes = lib.nqa_tp_bwd_fused_workspace_bytes(self.plan.handle, _nqa_dtype(x.dtype), E)
        if ws_bytes < 0:
            return None
        self._check(x, y, w, topo, pairing)
        gx = torch.empty((N, self.dim_in1), dtype=x.dtype, device=x.device)
        gw_rows = E if pairing is None else 2 * pairing.num_pairs
        gw = torch.empty((gw_rows, self.weight_numel), dtype=x.dtype, device=x.device) if need_gw else None
        gy = torch.empty((E, self.dim_in2), dtype=x.dtype, device=x.device) if need_gy else None
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        csr = topo.by_dst
        rowptr_s, eid_s, _ = topo.by_src
        es = x.element_size()
        # algorithmic bytes: operands and results once (w, y, gw, gy per edge; x, g, gx per node) -- the intermediate
        # per-edge grad_x rows (written and read once, 2 * dim_in1 per edge) are traffic, not algorithm
        nbytes = E * (es * (self.weight_numel + self.dim_in2) + 16) + N * es * (2 * self.dim_in1 + self.dim_out)
        nbytes += E * es * ((self.weight_numel if need_gw else 0) + (self.dim_in2 if need_gy else 0))
        with torch.cuda.device(x.device), ktimer.region("tp_bwd_fused", nbytes, 0.0,
                                                        E * es * self.weight_numel * (2 if need_gw else 1), self.weight_numel):
            self._call("bwd_fused", pairing, "slots_dst", x, x, y, w, g, *csr, rowptr_s, eid_s,
                       gw, gy, gx, ws, ws_bytes, N, E)
        return gx, gw, gy

    def bwd_pairs(self, x, y, w, g, topo: EdgeTopology, pairing, need_gx: bool = True):
        """(gx, gw, gy) with ``gw = [num_pairs, weight_numel]`` already summed over the two directed edges of every pair
        (``nqa_tp_scatter_bwd_pairs``), or None when the plan has no pair-centric kernel.  ``need_gx=False``: gx is None
        (the edge gradients only)."""
        lib = _lib.load()
        E, N = topo.num_edges, topo.num_nodes
        ws_bytes = lib.nqa_tp_bwd_pairs_workspace_bytes(self.plan.handle, _nqa_dtype(x.dtype), E)
        if ws_bytes < 0:
            return None
        self._check(x, y, w, topo, pairing)
        P = pairing.num_pairs
        gx = torch.empty((N, self.dim_in1), dtype=x.dtype, device=x.device) if need_gx else None
        gw = torch.empty((P, self.weight_numel), dtype=x.dtype, device=x.device)
        gy = torch.empty((E, self.dim_in2), dtype=x.dtype, device=x.device)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        # (owner_rowptr, pair_other, pair_row, pair_edge_in, pair_edge_out, other_rowptr, other_slot)
        owner = pairing.owner_csr
        es = x.element_size()
        # algorithmic bytes: SURVEY.md 8(d)'s boundary figure of the backward, per DIRECTED edge as the reference's
        # interface defines it (the same formulas as bwd_fused / bwd_edge) -- this kernel moves less than that because it
        # reads the shared weight row and writes its gradient once per pair
        nbytes = E * (es * (2 * self.weight_numel + 2 * self.dim_in2) + 16) + N * es * (
            (2 if need_gx else 1) * self.dim_in1 + self.dim_out)
        with torch.cuda.device(x.device), ktimer.region("tp_bwd_fused" if need_gx else "tp_bwd_edge", nbytes, 0.0,
                                                        E * es * 2 * self.weight_numel, self.weight_numel):
            self._call("bwd_pairs", None, None, x, x, y, w, g, *owner, gw, gy, gx, ws, ws_bytes, N, E)
        return gx, gw, gy

    def fwd_jvp(self, x, y, w, c_x, c_y, c_w, topo: EdgeTopology, pairing=None) -> torch.Tensor:
        """``F(c_x, y, w) + F(x, c_y, w) + F(x, y, c_w)`` in one pass (``nqa_tp_scatter_fwd_jvp``); a cotangent that is
        None drops its term."""
        self._check(x, y, w, topo, pairing)
        out = torch.empty((topo.num_nodes, self.dim_out), dtype=x.dtype, device=x.device)
        csr = topo.by_dst
        es = x.element_size()
        nterms = sum(t is not None for t in (c_x, c_y, c_w))
        nbytes = topo.num_edges * (es * (self.weight_numel * (2 if c_w is not None else 1) + 2 * self.dim_in2) + 16) + \
            topo.num_nodes * es * (2 * self.dim_in1 + self.dim_out)
        with torch.cuda.device(x.device), ktimer.region("tp_fwd", nbytes):
            # (one entry point: the weight rows are optional)
            self._call("fwd_jvp", None, None, x, x, y, w, c_x, c_y, c_w, *csr, out, topo.num_nodes, topo.num_edges,
                       *((pairing.slots_dst, pairing.num_pairs) if pairing is not None else (None, 0)))
        assert nterms > 0
        return out

    def bwd_x_dual(self, y, w, c_y, c_w, g, topo: EdgeTopology, pairing=None) -> torch.Tensor:
        """``Bx(c_y, w, g) + Bx(y, c_w, g)`` in one pass (``nqa_tp_scatter_bwd_x_dual``)."""
        self._check(None, y, w, topo, pairing)
        gx = torch.empty((topo.num_nodes, self.dim_in1), dtype=g.dtype, device=g.device)
        csr = topo.by_src
        es = g.element_size()
        nbytes = topo.num_edges * (es * 2 * (self.weight_numel + self.dim_in2) + 16) + topo.num_nodes * es * (
            self.dim_in1 + self.dim_out)
        with torch.cuda.device(g.device), ktimer.region("tp_bwd_x", nbytes):
            self._call("bwd_x_dual", None, None, g, y, w, c_y, c_w, g, *csr, gx, topo.num_nodes, topo.num_edges,
                       *((pairing.slots_src, pairing.num_pairs) if pairing is not None else (None, 0)))
        return gx

    def edge_grads_dual(self, x, x_cot, y, y_cot, w, g, topo: EdgeTopology, pairing, w_cot=None):
        """``(Bw(x_cot, y, g) + Bw(x, y_cot, g), By(x_cot, w, g) [+ By(x, w_cot, g)])`` in one pair-centric pass
        (``nqa_tp_scatter_bwd_pairs_dual``): the two weight-gradient terms of the second-order backward, summed over the
        directed edges of every pair, and its grad_y terms."""
        lib = _lib.load()
        E, N = topo.num_edges, topo.num_nodes
        self._check(x, y, w, topo, pairing)
        ws_bytes = lib.nqa_tp_bwd_pairs_workspace_bytes(self.plan.handle, _nqa_dtype(x.dtype), E)
        gw = torch.empty((pairing.num_pairs, self.weight_numel), dtype=x.dtype, device=x.device)
        gy = torch.empty((E, self.dim_in2), dtype=x.dtype, device=x.device)
        ws = torch.empty(max(ws_bytes, 1), dtype=torch.uint8, device=x.device)
        owner = pairing.owner_csr[:5]
        es = x.element_size()
        nbytes = E * (es * (2 * self.weight_numel + 3 * self.dim_in2) + 16) + N * es * (2 * self.dim_in1 + self.dim_out)
        with torch.cuda.device(x.device), ktimer.region("tp_bwd_edge", nbytes):
            self._call("bwd_pairs_dual", None, None, x, x, x_cot, y, y_cot, w, w_cot, g, *owner, gw, gy,
                       ws, ws_bytes, N, E)
        return gw, gy

    def use_pairs(self, dtype: torch.dtype, pairing) -> bool:
        """Pair-centric backward applicable (paired weights, kernel generated for this structure, not switched off)?"""
        return pairing is not None and not _switched_off("NQA_NO_PAIR_BWD") and self.has_pairs_kernel(dtype)

    def edge_grads_folded(self, x, y, w, g, topo: EdgeTopology, pairing, need_gw: bool, need_gy: bool):
        """(gw, gy) of the edge operands with ``gw`` per weight ROW (per pair when ``pairing`` is given, summed over its
        two directed edges): the pair-centric kernel when it applies, else ``bwd_edge`` + the fold of the two halves."""
        if need_gw and self.use_pairs(x.dtype, pairing):
            res = self.bwd_pairs(x, y, w, g, topo, pairing, need_gx=False)
            if res is not None:  # (None: the pair kernel does not apply to this call after all)
                _, gw, gy = res
                return gw, (gy if need_gy else None)
        gw, gy = self.bwd_edge(x, y, w, g, topo, need_gw=need_gw, need_gy=need_gy, pairing=pairing)
        return _fold(gw, pairing), gy

    def bwd_x(self, y, w, g, topo: EdgeTopology, pairing=None) -> torch.Tensor:
        self._check(None, y, w, topo, pairing)
        gx = torch.empty((topo.num_nodes, self.dim_in1), dtype=g.dtype, device=g.device)
        csr = topo.by_src
        es = g.element_size()
        nbytes = topo.num_edges * (es * (self.weight_numel + self.dim_in2) + 16) + topo.num_nodes * es * (
            self.dim_in1 + self.dim_out
        )
        with torch.cuda.device(g.device), ktimer.region("tp_bwd_x", nbytes, 0.0, topo.num_edges * es * self.weight_numel,
                                                        self.weight_numel):
            self._call("bwd_x", pairing, "slots_src", g, y, w, g, *csr, gx,
                       topo.num_nodes, topo.num_edges)
        return gx


def _fold(G, pairing):
    """Gradient w.r.t. paired weights: the two directed edges of pair p wrote rows p and p + P."""
    if G is None or pairing is None:
        return G
    P = pairing.num_pairs
    return G[:P] + G[P:]


class _TPScatterFn(torch.autograd.Function):
    """``pairing`` (``EdgePairing`` or None): ``w`` holds one row per reverse-edge pair instead of one per edge."""

    @staticmethod
    def forward(ctx, x, y, w, k: _Kernels, topo: EdgeTopology, pairing=None):
        x, y, w = x.contiguous(), y.contiguous(), w.contiguous()
        out = k.fwd(x, y, w, topo, pairing)
        ctx.save_for_backward(x, y, w)
        ctx.k, ctx.topo, ctx.pairing = k, topo, pairing
        return out

    @staticmethod
    def backward(ctx, g):
        x, y, w = ctx.saved_tensors
        need = tuple(ctx.needs_input_grad[:3])
        gx, gy, gw = _TPScatterBwdFn.apply(g, x, y, w, ctx.k, ctx.topo, need, ctx.pairing)
        return gx, gy, gw, None, None, None


class _TPScatterBwdFn(torch.autograd.Function):
    """(g, x, y, w) -> (gx, gy, gw); itself differentiable once more (force-matching training)."""

    @staticmethod
    def forward(ctx, g, x, y, w, k: _Kernels, topo: EdgeTopology, need: Tuple[bool, bool, bool], pairing=None):
        g = g.contiguous()
        fused = None
        folded = False
        if need[0] and need[1] and need[2] and k.prefer_fused_bwd and not _switched_off("NQA_NO_FUSED_BWD"):
            if k.use_pairs(x.dtype, pairing):
                fused = k.bwd_pairs(x, y, w, g, topo, pairing)
                folded = fused is not None
            if fused is None and k.fused_rows_ok:
                fused = k.bwd_fused(x, y, w, g, topo, need_gw=need[2], need_gy=need[1], pairing=pairing)
        if fused is not None:
            gx, gw, gy = fused
            if not folded:
                gw = _fold(gw, pairing)
        else:
            gx = k.bwd_x(y, w, g, topo, pairing) if need[0] else None
            gw, gy = k.edge_grads_folded(x, y, w, g, topo, pairing, need_gw=need[2], need_gy=need[1])
        ctx.save_for_backward(g, x, y, w)
        ctx.k, ctx.topo, ctx.pairing = k, topo, pairing
        ctx.mark_non_differentiable(*[t for t, n in zip((gx, gy, gw), need) if not n and t is not None])
        return gx, gy, gw

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, c_x, c_y, c_w):
        g, x, y, w = ctx.saved_tensors
        k, topo, pr = ctx.k, ctx.topo, ctx.pairing
        need_g, need_x, need_y, need_w = ctx.needs_input_grad[:4]
        c_x = c_x.contiguous() if c_x is not None else None
        c_y = c_y.contiguous() if c_y is not None else None
        c_w = c_w.contiguous() if c_w is not None else None

        def add(a, b):
            return b if a is None else (a if b is None else a + b)

        gg = gxx = gyy = gww = None
        if need_g and sum(t is not None for t in (c_x, c_y, c_w)) > 1 and k.has_fwd_jvp(x.dtype) and \
                not _switched_off("NQA_NO_FWD_JVP"):
            gg = k.fwd_jvp(x, y, w, c_x, c_y, c_w, topo, pr)  # the three terms in one pass
        elif need_g:
            if c_x is not None:
                gg = add(gg, k.fwd(c_x, y, w, topo, pr))
            if c_y is not None:
                gg = add(gg, k.fwd(x, c_y, w, topo, pr))
            if c_w is not None:
                gg = add(gg, k.fwd(x, y, c_w, topo, pr))
        if need_x and c_y is not None and c_w is not None and k.has_fwd_jvp(x.dtype) and \
                not _switched_off("NQA_NO_FWD_JVP"):
            gxx = k.bwd_x_dual(y, w, c_y, c_w, g, topo, pr)  # both terms in one pass
        elif need_x:
            if c_y is not None:
                gxx = add(gxx, k.bwd_x(c_y, w, g, topo, pr))
            if c_w is not None:
                gxx = add(gxx, k.bwd_x(y, c_w, g, topo, pr))
        if (need_w and c_x is not None and c_y is not None and k.use_pairs(x.dtype, pr)
                and k.has_dual_pairs_kernel(x.dtype) and not _switched_off("NQA_NO_DUAL_PAIR_BWD")):
            # both weight-gradient terms (and By(c_x, w, g)) in one pair-centric pass over the shared intermediate
            gww, a_y = k.edge_grads_dual(x, c_x, y, c_y, w, g, topo, pr, w_cot=c_w if need_y else None)
            gyy = add(gyy, a_y if need_y else None)
            if c_w is not None and need_y:
                c_w = None  # its grad_y term is in a_y already
        elif need_w and c_x is not None and c_y is not None and k.use_pairs(x.dtype, pr):
            # pair-centric kernels: both contributions arrive summed over the directed edges of every pair
            a_w1, a_y = k.edge_grads_folded(c_x, y, w, g, topo, pr, need_gw=True, need_gy=need_y)
            a_w2, _ = k.edge_grads_folded(x, c_y, w, g, topo, pr, need_gw=True, need_gy=False)
            gww, gyy = a_w1 + a_w2, add(gyy, a_y)
        elif pr is not None and need_w and c_x is not None and c_y is not None:
            # paired weights, both contributions: the four half-row streams (two directed edges x two kernels) land in
            # one buffer and are summed in a single pass (5 array passes instead of 9 for fold, fold, add)
            P = pr.num_pairs
            buf = torch.empty((2, 2 * P, k.weight_numel), dtype=w.dtype, device=w.device)
            _, a_y = k.bwd_edge(c_x, y, w, g, topo, need_gw=True, need_gy=need_y, pairing=pr, gw_out=buf[0])
            k.bwd_edge(x, c_y, w, g, topo, need_gw=True, need_gy=False, pairing=pr, gw_out=buf[1])
            gww, gyy = buf.view(4, P, k.weight_numel).sum(0), add(gyy, a_y)
        else:
            if c_x is not None and (need_y or need_w):
                # one pass yields both Bw(c_x, y, g) and By(c_x, g, w)
                a_w, a_y = k.edge_grads_folded(c_x, y, w, g, topo, pr, need_gw=need_w, need_gy=need_y)
                gww, gyy = add(gww, a_w), add(gyy, a_y)
            if c_y is not None and need_w:
                a_w, _ = k.edge_grads_folded(x, c_y, w, g, topo, pr, need_gw=True, need_gy=False)
                gww = add(gww, a_w)
        if c_w is not None and need_y:
            _, a_y = k.bwd_edge(x, y, c_w, g, topo, need_gw=False, need_gy=True, pairing=pr)
            gyy = add(gyy, a_y)
        return gg, gxx, gyy, gww, None, None, None, None


class TensorProductScatter(torch.nn.Module):
    """Drop-in for ``nequip.nn._tp_scatter_base.TensorProductScatter`` backed by gfx950 HIP kernels."""

    _nequip_custom_ops_libs = ("nequip_amd",)

    def __init__(self, feature_irreps_in, irreps_edge_attr, irreps_mid, instructions,
                 use_dispatcher_ops: bool = False) -> None:
        super().__init__()
        # True: always go through torch.ops.nequip_amd.tp_scatter_* (the opaque, traceable form; cf. `use_opaque` of the
        # reference's OpenEquivariance adapter, nequip/nn/_tp_scatter_oeq.py:13).  While a compiler is tracing the
        # module that form is selected automatically.
        self.use_dispatcher_ops = bool(use_dispatcher_ops)
        # keep the caller's objects (e3nn Irreps when used under nequip) for introspection, and our own
        # e3nn-free copies for the plan
        self.feature_irreps_in = feature_irreps_in
        self.irreps_edge_attr = irreps_edge_attr
        self.irreps_mid = irreps_mid
        self.instructions = instructions

        irreps_in1 = Irreps(str(feature_irreps_in))
        irreps_in2 = Irreps(str(irreps_edge_attr))
        irreps_out = Irreps(str(irreps_mid))
        # parameter-free descriptor under the same attribute name as the reference (`self.tp`)
        self.tp = TensorProduct(
            irreps_in1, irreps_in2, irreps_out, instructions, shared_weights=False, internal_weights=False
        )
        self.model_dtype = torch.get_default_dtype()

        from ._tp_scatter_ops import plan_key

        self._plan_key = plan_key(irreps_in1, irreps_in2, irreps_out, self.tp.instructions)
        self._plan = NativePlan(irreps_in1, irreps_in2, irreps_out, self.tp.instructions)
        # device image of the path tables: a non-persistent buffer so it follows .to(device) and never
        # enters the state dict (the reference module owns no persistent state of its own)
        self.register_buffer("_plan_image", self._plan.image, persistent=False)
        self._kernels: Optional[_Kernels] = None

    def _get_kernels(self) -> _Kernels:
        k = self._kernels
        if k is None or k.image.data_ptr() != self._plan_image.data_ptr():
            k = _Kernels(self._plan, self._plan_image)
            self._kernels = k
        return k

    def forward(self, x, edge_attr, edge_weight, edge_dst, edge_src, topology: Optional[EdgeTopology] = None,
                pairing=None):
        """``pairing`` (extension, ``EdgeTopology.pairing``): ``edge_weight`` has one row per reverse-edge pair."""
        from ..utils.tracing import traceable

        tracing = self.use_dispatcher_ops or traceable()
        if not x.is_cuda and not tracing:  # (fake CPU tensors may flow through the dispatcher ops while tracing)
            raise RuntimeError(
                "nequip_amd.nn.TensorProductScatter runs on the GPU only (HIP kernels); no CPU fallback exists"
            )
        if self._plan_image.device != x.device and not tracing:
            raise RuntimeError("module and inputs are on different devices; call .to(device) on the model")
        # explicit cast to account for AMP (as nequip/nn/_tp_scatter_oeq.py:49-57)
        x = x.to(self.model_dtype)
        edge_attr = edge_attr.to(self.model_dtype)
        edge_weight = edge_weight.to(self.model_dtype)
        if pairing is not None and not tracing:
            if topology is None:
                topology = topology_cache.get(edge_dst, edge_src, x.size(0))
            return _TPScatterFn.apply(x, edge_attr, edge_weight, self._get_kernels(), topology, pairing)
        if tracing:
            from ._tp_scatter_ops import tp_scatter

            return tp_scatter(x, edge_attr, edge_weight, edge_dst, edge_src, self._plan_key)
        if topology is None:
            topology = topology_cache.get(edge_dst, edge_src, x.size(0))
        return _TPScatterFn.apply(x, edge_attr, edge_weight, self._get_kernels(), topology)

    def extra_repr(self) -> str:
        return f"{self.tp.extra_repr()} | dtype={self.model_dtype}"
