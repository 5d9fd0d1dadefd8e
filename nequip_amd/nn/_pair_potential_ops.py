"""ZBL pair term on the GPU (``csrc/pair_potential.hip``): launches, autograd Functions and dispatcher ops.

The term is a function of the float64 edge vectors alone (the leaf ``ForceStressOutput`` differentiates), added to the
per-atom energies (``nequip/nn/pair_potential.py:348-389``).  Three kernels walk the centre-atom CSR of the cached topology:
``nqa_zbl_fwd`` (per-atom sums, fixed order), ``nqa_zbl_bwd`` (``dE/d edge_vec``) and ``nqa_zbl_bwd_bwd`` (the derivative of
that map w.r.t. the per-atom cotangent and the edge vectors: force-matching training differentiates it once more).

Dispatcher ops (``torch.ops.nequip_amd``; a tracer keeps them, ``utils/tracing.py``; also registered from C++):

``zbl_fwd(edge_vec [E, 3], pe_in [n, 1]?, edge_index [2, E], atom_types [N], z_table [T, 2], qqr2e_half [],
  rmax_recip_edge [E]?, rmax_recip, p, f32) -> pe_out [n, 1]``   (n = pe_in rows, or N; all float64 but the indices)
``zbl_bwd(g_pe [n, 1], edge_vec, edge_index, atom_types, z_table, qqr2e_half, rmax_recip_edge?, rmax_recip, p, f32)
  -> g_edge_vec [E, 3]``

``zbl_bwd`` is differentiable once more through ``nqa_zbl_bwd_bwd`` (Python only, as for the other training ops).
"""

from __future__ import annotations

from typing import Optional

import torch

from .. import _lib
from ..utils import ktimer
from ._topology import _ptr, current_stream_ptr, topology_cache


def _geometry(edge_vec, edge_index, types, z_table, qq, rmax_edge, rmax_recip: float, p: float, f32: bool, num_out: int):
    """The leading arguments every nqa_zbl_* entry shares (keeps the tensors it points at alive in the returned tuple)."""
    if not edge_vec.is_cuda:
        raise RuntimeError("nequip_amd ZBL runs on the GPU only (HIP kernel); no CPU fallback exists")
    assert edge_vec.dtype == torch.float64, "edge vectors must be float64 (nequip _GLOBAL_DTYPE)"
    vec = edge_vec.detach().contiguous()
    types = types.reshape(-1)
    types = (types if types.dtype == torch.int64 else types.to(torch.int64)).contiguous()
    n = types.shape[0]
    if not 0 <= num_out <= n:
        raise ValueError(f"ZBL: {num_out} per-atom energies for {n} atoms")
    rp, eid, nbr = topology_cache.get(edge_index[0], edge_index[1], n).by_dst
    zt = z_table.detach().to(torch.float64).contiguous()
    q = qq.detach().to(torch.float64).contiguous()
    re = None if rmax_edge is None else rmax_edge.detach().reshape(-1).to(torch.float64).contiguous()
    keep = (vec, types, rp, eid, nbr, zt, q, re)
    args = [_ptr(vec), _ptr(rp), _ptr(eid), _ptr(nbr), _ptr(types), _ptr(zt), _ptr(re), float(rmax_recip), float(p),
            int(bool(f32)), _ptr(q), n, int(num_out)]
    return keep, args


def _as_rows(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    if t is None:
        return None
    t = t.detach().to(torch.float64).reshape(-1)
    return t if t.is_contiguous() and t.stride(0) == 1 else t.contiguous()  # (the expanded gradient of a sum: stride 0)


def zbl_forward(edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, rmax_recip, p, f32) -> torch.Tensor:
    n_out = pe_in.shape[0] if pe_in is not None else types.numel()
    keep, args = _geometry(edge_vec, edge_index, types, z_table, qq, rmax_edge, rmax_recip, p, f32, n_out)
    pe = _as_rows(pe_in)
    out = torch.empty((n_out, 1), dtype=torch.float64, device=edge_vec.device)
    lib = _lib.load()
    with torch.cuda.device(edge_vec.device), ktimer.region("zbl_fwd", 40.0 * edge_vec.shape[0] + 24.0 * n_out):
        rc = lib.nqa_zbl_fwd(*args, _ptr(pe), _ptr(out), current_stream_ptr(edge_vec.device))
    _lib.check(rc, "nqa_zbl_fwd")
    return out


def zbl_backward(g_pe, edge_vec, edge_index, types, z_table, qq, rmax_edge, rmax_recip, p, f32) -> torch.Tensor:
    g = _as_rows(g_pe)
    keep, args = _geometry(edge_vec, edge_index, types, z_table, qq, rmax_edge, rmax_recip, p, f32, g.shape[0])
    out = torch.empty((edge_vec.shape[0], 3), dtype=torch.float64, device=edge_vec.device)
    lib = _lib.load()
    with torch.cuda.device(edge_vec.device), ktimer.region("zbl_bwd", 64.0 * edge_vec.shape[0] + 8.0 * g.shape[0]):
        rc = lib.nqa_zbl_bwd(*args, _ptr(g), _ptr(out), current_stream_ptr(edge_vec.device))
    _lib.check(rc, "nqa_zbl_bwd")
    return out


def zbl_backward_backward(g_pe, cot, edge_vec, edge_index, types, z_table, qq, rmax_edge, rmax_recip, p, f32,
                          want_gg_pe: bool, want_g_vec: bool):
    """(gg_pe [n, 1] or None, g_edge_vec2 [E, 3] or None) for the cotangent ``cot [E, 3]`` of ``zbl_backward``'s output."""
    g = _as_rows(g_pe)
    c = cot.detach().to(torch.float64).contiguous()
    keep, args = _geometry(edge_vec, edge_index, types, z_table, qq, rmax_edge, rmax_recip, p, f32, g.shape[0])
    dev = edge_vec.device
    gg = torch.empty((g.shape[0], 1), dtype=torch.float64, device=dev) if want_gg_pe else None
    gv = torch.empty((edge_vec.shape[0], 3), dtype=torch.float64, device=dev) if want_g_vec else None
    if gg is None and gv is None:
        return None, None
    lib = _lib.load()
    with torch.cuda.device(dev), ktimer.region("zbl_bwd_bwd", 88.0 * edge_vec.shape[0] + 16.0 * g.shape[0]):
        rc = lib.nqa_zbl_bwd_bwd(*args, _ptr(g), _ptr(c), _ptr(gg), _ptr(gv), current_stream_ptr(dev))
    _lib.check(rc, "nqa_zbl_bwd_bwd")
    return gg, gv


# ---- autograd (eager path) ------------------------------------------------------------------------------------------------
class _ZBLFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, cfg):
        ctx.save_for_backward(edge_vec)
        ctx.geo = (edge_index, types, z_table, qq, rmax_edge, cfg)
        ctx.pe_shape = None if pe_in is None else pe_in.shape
        return zbl_forward(edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, *cfg)

    @staticmethod
    def backward(ctx, g):
        (edge_vec,) = ctx.saved_tensors
        g_vec = _ZBLBwdFn.apply(g, edge_vec, *ctx.geo) if ctx.needs_input_grad[0] else None
        g_pe = g.reshape(ctx.pe_shape) if (ctx.pe_shape is not None and ctx.needs_input_grad[1]) else None
        return g_vec, g_pe, None, None, None, None, None, None


class _ZBLBwdFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g_pe, edge_vec, edge_index, types, z_table, qq, rmax_edge, cfg):
        ctx.save_for_backward(g_pe, edge_vec)
        ctx.geo = (edge_index, types, z_table, qq, rmax_edge, cfg)
        return zbl_backward(g_pe, edge_vec, edge_index, types, z_table, qq, rmax_edge, *cfg)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, c):
        g_pe, edge_vec = ctx.saved_tensors
        edge_index, types, z_table, qq, rmax_edge, cfg = ctx.geo
        gg, gv = zbl_backward_backward(g_pe, c, edge_vec, edge_index, types, z_table, qq, rmax_edge, *cfg,
                                       ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (None if gg is None else gg.view(g_pe.shape)), gv, None, None, None, None, None, None


def zbl(edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, rmax_recip: float, p: float, f32: bool) -> torch.Tensor:
    """``[n, 1]`` float64: ``pe_in`` (or 0) plus the ZBL energy of each centre atom's edges; differentiable twice w.r.t.
    ``edge_vec`` and once w.r.t. ``pe_in``."""
    return _ZBLFn.apply(edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, (float(rmax_recip), float(p), bool(f32)))


# ---- the same kernels as dispatcher ops (traced / AOTInductor form) ------------------------------------------------------
_NS = "nequip_amd"
_lib_def = torch.library.Library(_NS, "FRAGMENT")
_GEO = "Tensor edge_index, Tensor atom_types, Tensor z_table, Tensor qqr2e_half, Tensor? rmax_recip_edge, float rmax_recip, " \
       "float p, bool f32"
_lib_def.define(f"zbl_fwd(Tensor edge_vec, Tensor? pe_in, {_GEO}) -> Tensor")
_lib_def.define(f"zbl_bwd(Tensor g_pe, Tensor edge_vec, {_GEO}) -> Tensor")


def _fwd_cuda(edge_vec, pe_in, edge_index, atom_types, z_table, qq, rmax_edge, rmax_recip, p, f32):
    return zbl_forward(edge_vec, pe_in, edge_index, atom_types, z_table, qq, rmax_edge, rmax_recip, p, f32)


def _bwd_cuda(g_pe, edge_vec, edge_index, atom_types, z_table, qq, rmax_edge, rmax_recip, p, f32):
    return zbl_backward(g_pe, edge_vec, edge_index, atom_types, z_table, qq, rmax_edge, rmax_recip, p, f32)


_lib_def.impl("zbl_fwd", _fwd_cuda, "CUDA")
_lib_def.impl("zbl_bwd", _bwd_cuda, "CUDA")


@torch.library.register_fake(f"{_NS}::zbl_fwd")
def _fwd_fake(edge_vec, pe_in, edge_index, atom_types, z_table, qq, rmax_edge, rmax_recip, p, f32):
    n = pe_in.shape[0] if pe_in is not None else atom_types.shape[0]
    return edge_vec.new_empty((n, 1), dtype=torch.float64)


@torch.library.register_fake(f"{_NS}::zbl_bwd")
def _bwd_fake(g_pe, edge_vec, edge_index, atom_types, z_table, qq, rmax_edge, rmax_recip, p, f32):
    return edge_vec.new_empty((edge_vec.shape[0], 3), dtype=torch.float64)


def _fwd_setup(ctx, inputs, output):
    edge_vec, pe_in = inputs[:2]
    ctx.save_for_backward(edge_vec)
    ctx.geo = inputs[2:]
    ctx.pe_shape = None if pe_in is None else pe_in.shape


def _fwd_backward(ctx, g):
    (edge_vec,) = ctx.saved_tensors
    g_vec = torch.ops.nequip_amd.zbl_bwd(g, edge_vec, *ctx.geo) if ctx.needs_input_grad[0] else None
    g_pe = g.reshape(ctx.pe_shape) if (ctx.pe_shape is not None and ctx.needs_input_grad[1]) else None
    return (g_vec, g_pe) + (None,) * 8


torch.library.register_autograd(f"{_NS}::zbl_fwd", _fwd_backward, setup_context=_fwd_setup)


def _bwd_setup(ctx, inputs, output):
    g_pe, edge_vec = inputs[:2]
    ctx.save_for_backward(g_pe, edge_vec)
    ctx.geo = inputs[2:]


def _bwd_backward(ctx, c):
    g_pe, edge_vec = ctx.saved_tensors
    gg, gv = zbl_backward_backward(g_pe, c, edge_vec, *ctx.geo, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
    return ((None if gg is None else gg.view(g_pe.shape)), gv) + (None,) * 8


torch.library.register_autograd(f"{_NS}::zbl_bwd", _bwd_backward, setup_context=_bwd_setup)


def zbl_op(edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, rmax_recip: float, p: float,
           f32: bool) -> torch.Tensor:
    return torch.ops.nequip_amd.zbl_fwd(edge_vec, pe_in, edge_index, types, z_table, qq, rmax_edge, float(rmax_recip),
                                        float(p), bool(f32))
