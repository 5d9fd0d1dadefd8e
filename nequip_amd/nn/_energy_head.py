"""Per-atom energy head in one launch per direction (``nqa_energy_head``, csrc/energy_head.hip).

In eval mode on the GPU the tail of the energy model -- the last layer's Gate (scalars only), the depth-0 ``ScalarMLP``
readout and ``PerTypeScaleShift`` (``nequip/model/nequip_models.py:371-399``, ``nequip/nn/atomwise.py:116-284``) -- and its
backward are a dozen launches on ``[N, 64]`` / ``[N, 1]`` tensors; here they are two.  The modules, their parameters and
their state-dict keys stay where the reference has them: the last ``ConvNetLayer`` defers its gate (``_nqa_pregate``), the
readout module consumes it and marks the per-atom energies as already scaled, ``PerTypeScaleShift`` then passes them on.

With trainable scale / shift tables (``PerTypeScaleShift(scales_trainable / shifts_trainable)``) the parameters are inputs:
``energy_head_train`` is the same forward launch inside a twice-differentiable Function pair whose backward launches
(``nqa_energy_head_train_bwd`` / ``_bwd_bwd``) also return the gradients of the readout weight and of the two tables, as
sums over atoms taken in a fixed order (no atomics: bit-reproducible).
"""

from __future__ import annotations

import torch

from .. import _lib
from ..utils import ktimer
from ..utils import wgrad as _wgrad


_ptr = _lib.ptr


def _launch(backward: int, h, w, scales, shifts, types, g_e, out, act: int, cst: float):
    lib = _lib.load()
    N, D = h.shape
    ns = 0 if scales is None else scales.numel()
    nh = 0 if shifts is None else shifts.numel()
    with torch.cuda.device(h.device), ktimer.region("energy_head", 4.0 * N * D * (2 if backward else 1) + 8.0 * N):
        rc = lib.nqa_energy_head(backward, _ptr(h), _ptr(w), _ptr(scales), ns, _ptr(shifts), nh, _ptr(types), _ptr(g_e),
                                 _ptr(out), D, act, float(cst), N,
                                 _lib.stream_ptr(h.device))
    _lib.check(rc, "nqa_energy_head")


class _EnergyHeadFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, scales, shifts, types, act: int, cst: float):
        h = h.contiguous()
        e = torch.empty((h.shape[0], 1), dtype=torch.float64, device=h.device)
        _launch(0, h, w, scales, shifts, types, None, e, act, cst)
        ctx.save_for_backward(h, w, scales, types)
        ctx.act, ctx.cst = act, cst
        return e

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        h, w, scales, types = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return (None,) * 7
        g = g.to(torch.float64)
        if not g.is_contiguous() or g.stride(0) != 1:  # (the expanded gradient of a sum: stride 0)
            g = g.contiguous()
        gh = torch.empty_like(h)
        _launch(1, h, w, scales, None, types, g.view(-1), gh, ctx.act, ctx.cst)
        return gh, None, None, None, None, None, None


def energy_head(h, w, scales, shifts, types, act: int, cst: float) -> torch.Tensor:
    """``[N, 1]`` float64 per-atom energies ``shift[t] + scale[t] * double(sum_c w[c] cst act(h[:, c]))``; the gradient
    w.r.t. ``h`` is one launch (constant weights: eval mode)."""
    return _EnergyHeadFn.apply(h, w, scales, shifts, types, act, cst)


# ---- training: the weight and the tables are differentiable inputs ------------------------------------------------------------
def _launch_train(order: int, h, w, scales, types, g_e, v, n_shifts: int, want_h: bool, want_w: bool, want_scales: bool,
                  want_shifts: bool, act: int, cst: float):
    """``order`` 1: ``(g_h, g_w, g_scales, g_shifts)`` of the head for the energy gradient ``g_e``; ``order`` 2: ``(gg_e, g_h,
    g_w, g_scales)`` of the map ``(g_e, h, w, scales) -> g_h`` for the cotangent ``v``.  Entries not asked for are None."""
    lib = _lib.load()
    N, D = h.shape
    ns = 0 if scales is None else scales.numel()
    want_scales = want_scales and ns > 0
    want_shifts = want_shifts and n_shifts > 0 and order == 1
    dev = h.device
    g_h = torch.empty_like(h) if want_h else None
    g_w = torch.empty_like(w) if want_w else None
    g_sc = torch.empty(ns, dtype=torch.float64, device=dev) if want_scales else None
    g_sh = torch.empty(n_shifts, dtype=torch.float64, device=dev) if want_shifts else None
    gg_e = torch.empty(N, dtype=torch.float64, device=dev) if order == 2 else None
    dims = (D if want_w else 0, ns if want_scales else 0, n_shifts if want_shifts else 0)
    nbytes = int(lib.nqa_energy_head_train_workspace_bytes(N, *dims))
    work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=dev) if any(dims) else None
    with torch.cuda.device(dev), ktimer.region("energy_head_train", 4.0 * N * D * (2 if order == 1 else 3) + 8.0 * N):
        if order == 1:
            rc = lib.nqa_energy_head_train_bwd(_ptr(h), _ptr(w), _ptr(scales), ns, n_shifts, _ptr(types), _ptr(g_e), _ptr(g_h),
                                               _ptr(g_w), _ptr(g_sc), _ptr(g_sh), _ptr(work), nbytes, D, act, float(cst), N,
                                               _lib.stream_ptr(dev))
        else:
            rc = lib.nqa_energy_head_train_bwd_bwd(_ptr(h), _ptr(w), _ptr(scales), ns, _ptr(types), _ptr(g_e), _ptr(v),
                                                   _ptr(gg_e), _ptr(g_h), _ptr(g_w), _ptr(g_sc), _ptr(work), nbytes, D, act,
                                                   float(cst), N, _lib.stream_ptr(dev))
    _lib.check(rc, "nqa_energy_head_train_bwd" if order == 1 else "nqa_energy_head_train_bwd_bwd")
    return (g_h, g_w, g_sc, g_sh) if order == 1 else (gg_e, g_h, g_w, g_sc)


def _energy_gradient(g) -> torch.Tensor:
    g = g.to(torch.float64)
    if not g.is_contiguous() or g.stride(0) != 1:  # (the expanded gradient of a sum: stride 0)
        g = g.contiguous()
    return g.view(-1)


class _EnergyHeadTrainFn(torch.autograd.Function):
    """``(h, w, scales, shifts) -> E``; the gradient w.r.t. ``h`` comes from a Function of its own, so it can be differentiated
    once more (forces in the loss).  The parameter gradients are by-products of that launch; they are left out where only data
    gradients are asked for (``wgrad.inputs_only_backward``: the force evaluation inside ``ForceStressOutput``)."""

    @staticmethod
    def forward(ctx, h, w, scales, shifts, types, act: int, cst: float):
        h, w = h.contiguous(), w.contiguous()
        e = torch.empty((h.shape[0], 1), dtype=torch.float64, device=h.device)
        if h.shape[0] > 0:  # (no atoms: nothing to launch; the backward still returns zero parameter gradients)
            _launch(0, h, w, scales, shifts, types, None, e, act, cst)
        ctx.save_for_backward(h, w, scales, types)
        ctx.act, ctx.cst, ctx.n_shifts = act, cst, (0 if shifts is None else shifts.numel())
        return e

    @staticmethod
    def backward(ctx, g):
        h, w, scales, types = ctx.saved_tensors
        params = _wgrad.param_grads_wanted()
        need = ctx.needs_input_grad
        gh, gw, gsc, gsh = _EnergyHeadTrainBwdFn.apply(
            _energy_gradient(g), h, w, scales, types, ctx.act, ctx.cst, ctx.n_shifts, need[0], params and need[1],
            params and need[2], params and need[3])
        return gh, gw, gsc, gsh, None, None, None


class _EnergyHeadTrainBwdFn(torch.autograd.Function):
    """``(g_e, h, w, scales) -> g_h`` (+ the parameter gradients of the head, not differentiable further)."""

    @staticmethod
    def forward(ctx, g_e, h, w, scales, types, act: int, cst: float, n_shifts: int, want_h: bool, want_w: bool,
                want_scales: bool, want_shifts: bool):
        out = _launch_train(1, h, w, scales, types, g_e, None, n_shifts, want_h, want_w, want_scales, want_shifts, act, cst)
        ctx.mark_non_differentiable(*[t for t in out[1:] if t is not None])
        ctx.save_for_backward(g_e, h, w, scales, types)
        ctx.act, ctx.cst = act, cst
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v, *unused):
        if v is None:
            return (None,) * 12
        g_e, h, w, scales, types = ctx.saved_tensors
        params = _wgrad.param_grads_wanted()
        need = ctx.needs_input_grad
        gg_e, gh, gw, gsc = _launch_train(2, h, w, scales, types, g_e, v.contiguous(), 0, need[1], params and need[2],
                                          params and need[3], False, ctx.act, ctx.cst)
        return (gg_e if need[0] else None, gh, gw, gsc) + (None,) * 8


def energy_head_train(h, w, scales, shifts, types, act: int, cst: float) -> torch.Tensor:
    """``energy_head`` with ``w``, ``scales`` and ``shifts`` as differentiable inputs, to second order in ``h``."""
    return _EnergyHeadTrainFn.apply(h, w, scales, shifts, types, act, cst)


# ---- the same two launches as dispatcher ops (a tracer keeps them: utils/tracing.py) ----------------------------------------
_NS = "nequip_amd"
_lib_def = torch.library.Library(_NS, "FRAGMENT")
_lib_def.define("energy_head_fwd(Tensor h, Tensor w, Tensor? scales, Tensor? shifts, Tensor types, int act, float cst) "
                "-> Tensor")
_lib_def.define("energy_head_bwd(Tensor g_e, Tensor h, Tensor w, Tensor? scales, Tensor types, int act, float cst) -> Tensor")


def _fwd_cuda(h, w, scales, shifts, types, act, cst):
    h = h.contiguous()
    e = torch.empty((h.shape[0], 1), dtype=torch.float64, device=h.device)
    _launch(0, h, w.contiguous(), scales, shifts, types.contiguous(), None, e, int(act), float(cst))
    return e


def _bwd_cuda(g_e, h, w, scales, types, act, cst):
    h = h.contiguous()
    g = g_e.to(torch.float64).contiguous().view(-1)
    gh = torch.empty_like(h)
    _launch(1, h, w.contiguous(), scales, None, types.contiguous(), g, gh, int(act), float(cst))
    return gh


_lib_def.impl("energy_head_fwd", _fwd_cuda, "CUDA")
_lib_def.impl("energy_head_bwd", _bwd_cuda, "CUDA")


@torch.library.register_fake(f"{_NS}::energy_head_fwd")
def _fwd_fake(h, w, scales, shifts, types, act, cst):
    torch._check(h.dim() == 2 and w.dim() == 1 and w.shape[0] == h.shape[1], lambda: "h [N, D], w [D]")
    return h.new_empty((h.shape[0], 1), dtype=torch.float64)


@torch.library.register_fake(f"{_NS}::energy_head_bwd")
def _bwd_fake(g_e, h, w, scales, types, act, cst):
    return torch.empty_like(h)


def _op_setup(ctx, inputs, output):
    h, w, scales, shifts, types, act, cst = inputs
    ctx.save_for_backward(h, w, scales, types)
    ctx.act, ctx.cst = act, cst


def _op_backward(ctx, g):
    h, w, scales, types = ctx.saved_tensors
    gh = None
    if ctx.needs_input_grad[0]:
        gh = torch.ops.nequip_amd.energy_head_bwd(g, h, w, scales, types, ctx.act, ctx.cst)
    return gh, None, None, None, None, None, None


torch.library.register_autograd(f"{_NS}::energy_head_fwd", _op_backward, setup_context=_op_setup)


def energy_head_op(h, w, scales, shifts, types, act: int, cst: float) -> torch.Tensor:
    return torch.ops.nequip_amd.energy_head_fwd(h, w, scales, shifts, types, int(act), float(cst))
