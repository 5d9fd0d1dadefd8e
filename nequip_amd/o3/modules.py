"""Node-side equivariant modules of the hot path: channel-mixing ``Linear``, the self-connection
``FullyConnectedTensorProduct`` and ``Gate``.

In the reference these are ``e3nn.o3.Linear`` (``nequip/nn/interaction_block.py:82-87,129-138``),
``e3nn.o3.FullyConnectedTensorProduct`` (``:142-146``) and ``e3nn.nn.Gate``
(``nequip/nn/convnetlayer.py:104-112``); semantics restated from SURVEY.md A.5-A.7.  They act on the N
node rows only (dense GEMMs with K = mul), so they are expressed as plain matmuls that rocBLAS/hipBLASLt
executes on MFMA -- "library GEMM" plumbing, not hand-written kernels.  Parameter names, shapes, flat
weight layout and initialisation (N(0,1)) follow e3nn so that state dicts are interchangeable.
"""

from __future__ import annotations

import math
from typing import Callable, List, Optional, Sequence

import torch

from .irreps import Irrep, Irreps
from ._node_kernels import GateMeta, NodeLinearMeta, gate as _gate_kernel, node_linear as _node_linear
from ..utils.wgrad import _WeightCacheMixin, differentiable_parameters


from ..utils.tracing import traceable
from . import _node_ops

class Linear(_WeightCacheMixin, torch.nn.Module):
    """``out[z, i_out, w, m] = sum_{i_in} fan_in(i_out)^-1/2 sum_u x[z, i_in, u, m] W[u, w]`` (no bias)."""

    def __init__(self, irreps_in, irreps_out, internal_weights: bool = True, shared_weights: bool = True):
        super().__init__()
        assert internal_weights and shared_weights
        self.irreps_in = Irreps(irreps_in)
        self.irreps_out = Irreps(irreps_out)
        self.instructions = [
            (i, o)
            for i, (_, ir_in) in enumerate(self.irreps_in)
            for o, (_, ir_out) in enumerate(self.irreps_out)
            if ir_in == ir_out
        ]
        fan_in = [0] * len(self.irreps_out)
        for i, o in self.instructions:
            fan_in[o] += self.irreps_in[i].mul
        self._scale = [1.0 / math.sqrt(f) if f > 0 else 0.0 for f in fan_in]
        self.weight_numel = sum(self.irreps_in[i].mul * self.irreps_out[o].mul for i, o in self.instructions)
        self.weight = torch.nn.Parameter(torch.randn(self.weight_numel))
        self._in_slices = self.irreps_in.slices()
        self._in_sizes = [mul_ir.dim for mul_ir in self.irreps_in]
        # e3nn-compatible view of where each 2-D weight sits in the flat parameter (cf. nequip/model/param_groups.py:71-88)
        self.weight_index_slices = []
        off = 0
        for i, o in self.instructions:
            n = self.irreps_in[i].mul * self.irreps_out[o].mul
            self.weight_index_slices.append((slice(off, off + n), (self.irreps_in[i].mul, self.irreps_out[o].mul)))
            off += n
        # fused HIP path: all per-irrep matrices in one launch (csrc/node_ops.hip)
        self._meta = NodeLinearMeta(self.irreps_in, self.irreps_out, self.instructions)
        self._op_key = _node_ops.linear_key(self.irreps_in, self.irreps_out, self.instructions)
        scale_vec = torch.cat(
            [torch.full((sl.stop - sl.start,), self._scale[o]) for (i, o), (sl, _) in zip(self.instructions, self.weight_index_slices)]
        ) if self.instructions else torch.zeros(0)
        self.register_buffer("_scale_vec", scale_vec, persistent=False)

    def forward(self, x: torch.Tensor, addend: Optional[torch.Tensor] = None, scale: float = 1.0) -> torch.Tensor:
        if x.is_cuda and not traceable() and x.dtype in (torch.float32, torch.float64) and self.weight_numel > 0:
            # eval mode: parameter gradients are not produced (inference fast path, as for the radial MLP) unless
            # nequip_amd.utils.wgrad.eval_parameter_gradients(True) asks for the reference's behaviour
            if differentiable_parameters(self.training, self.weight):
                wp = (self.weight * self._scale_vec).unsqueeze(0)
                # (what grad(wp) means for the parameter: lets the backward deliver it outside autograd, utils/wgrad.py)
                wp._nqa_param = (self.weight, self._scale_vec, False)
            else:
                wp = self.eval_weights(x.device, x.dtype)
            return _node_linear(x, wp, None, self._meta, addend=addend, scale=scale)
        if (traceable() and x.is_cuda and x.dtype == torch.float32 and self.weight_numel > 0
                and not differentiable_parameters(self.training, self.weight)):
            # while tracing, constant weights: the fused kernel as a dispatcher op (o3/_node_ops.py)
            return _node_ops.node_linear_op(x, self.traced_weights(), self._op_key, addend=addend, scale=scale)
        out = self._forward_reference(x)
        if scale != 1.0:
            out = out * scale
        return out if addend is None else out + addend

    def traced_weights(self) -> torch.Tensor:
        """``eval_weights`` as graph operations on the (possibly fake) parameter, for the dispatcher-op forms."""
        return (self.weight.detach() * self._scale_vec).unsqueeze(0)

    def eval_weights(self, device, dtype) -> torch.Tensor:
        """Packed, path-normalised weights ``[1, wstride]`` as constants (eval mode): built once per parameter version
        instead of with a handful of tiny kernels every step; the transposed copy for the backward rides on the tensor."""
        key = (id(self.weight), self.weight.data_ptr(), self.weight._version, device, dtype)
        cached = getattr(self, "_eval_wp", None)
        if cached is None or cached[0] != key:
            cached = (key, (self.weight.detach() * self._scale_vec).unsqueeze(0).contiguous())
            self._eval_wp = cached
        return cached[1]

    def _forward_reference(self, x: torch.Tensor) -> torch.Tensor:
        """ATen formulation (CPU tensors: host-side tests of the module algebra only)."""
        Z = x.shape[0]
        outs: List[Optional[torch.Tensor]] = [None] * len(self.irreps_out)
        # torch.split (backward = one cat) instead of slicing (backward = zero-fill + copy + add per slice)
        xs = torch.split(x, self._in_sizes, dim=1) if len(self._in_sizes) > 1 else (x,)
        for (i, o), (sl, shape) in zip(self.instructions, self.weight_index_slices):
            mul_in, ir = self.irreps_in[i]
            d = ir.dim
            W = self.weight[sl].view(shape) * self._scale[o]
            if d == 1:
                r = torch.mm(xs[i], W)
            else:
                r = torch.einsum("zum,uw->zwm", xs[i].view(Z, mul_in, d), W).reshape(Z, -1)
            outs[o] = r if outs[o] is None else outs[o] + r
        cols = [
            outs[o] if outs[o] is not None else x.new_zeros(Z, mul_ir.dim) for o, mul_ir in enumerate(self.irreps_out)
        ]
        return torch.cat(cols, dim=-1) if len(cols) > 1 else cols[0]

    def extra_repr(self) -> str:
        return f"{self.irreps_in} -> {self.irreps_out} | {self.weight_numel} weights"


class _SkinnyMMFn(torch.autograd.Function):
    """``a [T, V] @ b [V, K]`` with T, V small and K large (the per-type contraction of the self-connection weights: 5 x 64 x
    20480).  The product itself is fine in a library GEMM; its gradient w.r.t. ``a`` is ``g [T, K] @ b^T [K, V]`` -- a T x V
    output with a reduction of length K, which the library runs on ONE workgroup (57 us at K = 20480).  Here the reduction is
    split over S batches of a batched GEMM and summed (8 us).  Plain differentiable ops: double backward works as is."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return torch.mm(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        ga = gb = None
        if ctx.needs_input_grad[0]:
            T, K = g.shape
            V = b.shape[0]
            S = 1
            while S < 64 and K % (2 * S) == 0 and K // (2 * S) >= 256:
                S *= 2
            if S > 1:
                Kc = K // S
                gs = g.reshape(T, S, Kc).transpose(0, 1)            # [S, T, Kc]
                bs = b.reshape(V, S, Kc).permute(1, 2, 0)           # [S, Kc, V]
                ga = torch.bmm(gs, bs).sum(0)
            else:
                ga = torch.mm(g, b.t())
        if ctx.needs_input_grad[1]:
            gb = torch.mm(a.t(), g)
        return ga, gb


def _skinny_mm(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    return _SkinnyMMFn.apply(a, b)


class FullyConnectedTensorProduct(_WeightCacheMixin, torch.nn.Module):
    """Self-connection ``sc(x, node_attrs)`` with scalar (``Nx0e``) second operand.

    ``out[z, w, m] = (sum_paths mul1*mul2)^-1/2 sum_{u,v} W[u, v, w] x[z, u, m] a[z, v]``.
    Two evaluation orders are provided (identical in exact arithmetic):

    * ``forward(x, a)``: the reference's order -- outer product ``x (x) a`` then one GEMM with K = mul1*mul2
      (5.8 MFLOP/node/layer at 64 features, SURVEY.md hard part 6);
    * ``forward_typed(x, types, table)``: when ``a = table[types]`` (an embedding lookup), contract the weights
      with the T table rows first (``W_t[u, w] = sum_v table[t, v] W[u, v, w]``) and run one GEMM with
      K = T*mul1 over one-hot-expanded features -- mul2/T times fewer FLOPs.
    """

    _weight_cache_attrs = _WeightCacheMixin._weight_cache_attrs + ("_eval_wp_classes",)

    def __init__(self, irreps_in1, irreps_in2, irreps_out):
        super().__init__()
        self.irreps_in1 = Irreps(irreps_in1)
        self.irreps_in2 = Irreps(irreps_in2)
        self.irreps_out = Irreps(irreps_out)
        if any(ir.l != 0 or ir.p != 1 for _, ir in self.irreps_in2):
            raise NotImplementedError("self-connection second operand must be even scalars (node attributes)")
        self.instructions = [
            (i1, i2, io)
            for i1, (_, ir1) in enumerate(self.irreps_in1)
            for i2, (_, ir2) in enumerate(self.irreps_in2)
            for io, (_, iro) in enumerate(self.irreps_out)
            if iro in list(ir1 * ir2)
        ]
        fan = [0] * len(self.irreps_out)
        for i1, i2, io in self.instructions:
            fan[io] += self.irreps_in1[i1].mul * self.irreps_in2[i2].mul
        self._scale = [1.0 / math.sqrt(f) if f > 0 else 0.0 for f in fan]
        self.weight_numel = sum(
            self.irreps_in1[i1].mul * self.irreps_in2[i2].mul * self.irreps_out[io].mul
            for i1, i2, io in self.instructions
        )
        self.weight = torch.nn.Parameter(torch.randn(self.weight_numel))
        self._s1 = self.irreps_in1.slices()
        self._s2 = self.irreps_in2.slices()
        self._sizes1 = [mul_ir.dim for mul_ir in self.irreps_in1]
        self._wslices = []
        off = 0
        for i1, i2, io in self.instructions:
            shape = (self.irreps_in1[i1].mul, self.irreps_in2[i2].mul, self.irreps_out[io].mul)
            n = shape[0] * shape[1] * shape[2]
            self._wslices.append((slice(off, off + n), shape))
            off += n
        self._meta = (
            NodeLinearMeta(self.irreps_in1, self.irreps_out, [(i1, io) for i1, _, io in self.instructions])
            if len(self.irreps_in2) == 1
            else None
        )
        self._op_key = (_node_ops.linear_key(self.irreps_in1, self.irreps_out, [(i1, io) for i1, _, io in self.instructions])
                        if self._meta is not None else None)

    def _contract_index(self, device, dtype):
        key = (str(device), dtype)
        cache = self.__dict__.setdefault("_contract_cache", {})
        if key not in cache:
            V = self.irreps_in2[0].mul
            idx, scl = [], []
            for (i1, i2, io), (sl, shape) in zip(self.instructions, self._wslices):
                u, v, w = shape
                assert v == V
                block = torch.arange(sl.start, sl.stop).view(u, v, w).permute(1, 0, 2).reshape(v, u * w)
                idx.append(block)
                scl.append(torch.full((u * w,), self._scale[io], dtype=torch.float64))
            perm = torch.cat(idx, dim=1).reshape(-1).to(device)
            cache[key] = (perm, torch.cat(scl).to(device=device, dtype=dtype).view(1, -1))
        return cache[key]

    def _assemble(self, outs, x):
        Z = x.shape[0]
        cols = [
            outs[o] if outs[o] is not None else x.new_zeros(Z, mul_ir.dim) for o, mul_ir in enumerate(self.irreps_out)
        ]
        return torch.cat(cols, dim=-1) if len(cols) > 1 else cols[0]

    def forward(self, x: torch.Tensor, a: torch.Tensor) -> torch.Tensor:
        Z = x.shape[0]
        outs: List[Optional[torch.Tensor]] = [None] * len(self.irreps_out)
        for (i1, i2, io), (sl, shape) in zip(self.instructions, self._wslices):
            mul1, ir = self.irreps_in1[i1]
            d = ir.dim
            W = self.weight[sl].view(shape[0] * shape[1], shape[2]) * self._scale[io]
            xa = x[:, self._s1[i1]].reshape(Z, mul1, d)
            av = a[:, self._s2[i2]]
            # [Z, d, mul1, mul2] -> GEMM over (u v)
            xx = xa.transpose(1, 2).unsqueeze(-1) * av.view(Z, 1, 1, -1)
            r = torch.matmul(xx.reshape(Z, d, -1), W).transpose(1, 2).reshape(Z, -1)
            outs[io] = r if outs[io] is None else outs[io] + r
        return self._assemble(outs, x)

    def traced_weights_typed(self, table: torch.Tensor) -> torch.Tensor:
        """``eval_weights_typed`` as graph operations, for the dispatcher-op forms (per-instruction einsums on slices of the
        flat weight: no cached index tensors -- a real constant tensor is not allowed next to fake weights while make_fx
        traces symbolically)."""
        tb = table.detach()
        parts = []
        for (i1, i2, io), (sl, shape) in zip(self.instructions, self._wslices):
            W = self.weight.detach()[sl].view(shape)
            parts.append((torch.einsum("tv,uvw->tuw", tb[:, self._s2[i2]], W) * self._scale[io]).reshape(tb.shape[0], -1))
        return torch.cat(parts, dim=1) if len(parts) > 1 else parts[0]

    def eval_weights_typed(self, table: torch.Tensor, dtype) -> torch.Tensor:
        """Per-type pre-contracted weights ``W_t[u, w] = sum_v table[t, v] W[u, v, w]`` as constants, ``[T, wstride]``."""
        key = (id(self.weight), self.weight.data_ptr(), self.weight._version, table._version, table.data_ptr(),
               table.device, dtype)
        cached = getattr(self, "_eval_wp", None)
        if cached is None or cached[0] != key:
            perm, scale = self._contract_index(self.weight.device, self.weight.dtype)
            w = self.weight.detach()
            wp = torch.mm(table.detach(), w.index_select(0, perm).view(table.shape[1], -1) * scale)
            cached = (key, wp.contiguous())
            self._eval_wp = cached
        return cached[1]

    def _contract_cols(self, weight: torch.Tensor, table: torch.Tensor, v0: int) -> torch.Tensor:
        """``W_r[u, w] = sum_v table[r, v] W[u, v0 + v, w]`` for all instructions, ``[R, wstride]``: the contraction of
        ``forward_typed`` restricted to the ``table.shape[1]`` columns of the second operand that start at ``v0``."""
        perm, scale = self._contract_index(weight.device, weight.dtype)
        wm = weight.index_select(0, perm).view(self.irreps_in2[0].mul, -1)
        return _skinny_mm(table, wm[v0 : v0 + table.shape[1]] * scale)

    def _eval_weights_cols(self, table: torch.Tensor, v0: int, dtype) -> torch.Tensor:
        """``_contract_cols`` as constants (eval mode), one cache entry per (table, column offset)."""
        key = (v0, id(self.weight), self.weight.data_ptr(), self.weight._version, table._version, table.data_ptr(),
               tuple(table.shape), table.device, dtype)
        cache = self.__dict__.setdefault("_eval_wp_classes", {})
        hit = cache.get(key)
        if hit is None:
            if len(cache) >= 16:
                cache.clear()
            hit = cache[key] = self._contract_cols(self.weight.detach(), table.detach(), v0).contiguous()
        return hit

    def forward_classes(self, x: torch.Tensor, types: torch.Tensor, table: torch.Tensor, classes) -> torch.Tensor:
        """``sc(x, a)`` for ``a[z] = cat(table[types[z]], tb_1[idx_1[z]], ...)``, where ``classes`` lists ``(idx_k, tb_k,
        v0_k)`` and ``tb_k`` fills columns ``[v0_k, v0_k + tb_k.shape[1])`` of ``a`` (categorical graph fields of a batch:
        ``idx_k`` = the row of the atom's frame).  The map is linear in ``a``, so it is the sum of one typed map per table,
        each with its own pre-contracted weights -- ``T + sum_k R_k`` weight sets, independent of the number of frames --
        chained through the ``addend`` of the fused launch (fixed order: deterministic)."""
        if not (x.is_cuda and not traceable() and self._meta is not None and x.dtype in (torch.float32, torch.float64)):
            raise NotImplementedError("forward_classes: float32 / float64 CUDA features and a single scalar attribute "
                                      "block only")
        n = x.shape[0]
        out = None
        for idx, tb, v0 in [(types, table, 0)] + list(classes):
            if differentiable_parameters(self.training, self.weight):
                wp = self._contract_cols(self.weight, tb, v0)
            else:
                wp = self._eval_weights_cols(tb, v0, x.dtype)
            out = _node_linear(x, wp, idx.view(-1)[:n].contiguous(), self._meta, addend=out)
        return out

    def forward_typed(self, x: torch.Tensor, types: torch.Tensor, table: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and not traceable() and self._meta is not None and x.dtype in (torch.float32, torch.float64):
            # per-type pre-contraction W_t[u, w] = sum_v table[t, v] W[u, v, w] (tiny), then ONE fused launch
            def contract(weight, table):
                # all instructions at once: gather the flat [u, v, w] blocks into one [v, sum(u*w)] matrix (fixed
                # permutation, path scale folded in), then a single [T, v] x [v, sum(u*w)] product
                perm, scale = self._contract_index(weight.device, weight.dtype)
                return _skinny_mm(table, weight.index_select(0, perm).view(table.shape[1], -1) * scale)

            if differentiable_parameters(self.training, self.weight):
                wp = contract(self.weight, table)
            else:  # constants in eval mode: contracted once per (weight, table) version
                wp = self.eval_weights_typed(table, x.dtype)
            return _node_linear(x, wp, types.view(-1).contiguous(), self._meta)
        if (traceable() and x.is_cuda and x.dtype == torch.float32 and self._meta is not None
                and not differentiable_parameters(self.training, self.weight)):
            return _node_ops.node_linear_op(x, self.traced_weights_typed(table), self._op_key,
                                            types=types.view(-1).contiguous())
        Z = x.shape[0]
        T = table.shape[0]
        onehot = torch.nn.functional.one_hot(types.view(-1), T).to(x.dtype)  # [Z, T]
        outs: List[Optional[torch.Tensor]] = [None] * len(self.irreps_out)
        xs = torch.split(x, self._sizes1, dim=1) if len(self._sizes1) > 1 else (x,)
        for (i1, i2, io), (sl, shape) in zip(self.instructions, self._wslices):
            mul1, ir = self.irreps_in1[i1]
            d = ir.dim
            W = self.weight[sl].view(shape)
            tb = table[:, self._s2[i2]]  # [T, mul2]
            Wt = torch.einsum("tv,uvw->tuw", tb, W).reshape(T * mul1, shape[2]) * self._scale[io]
            # one-hot expansion over the atom types: [Z, T*mul1, d], then one GEMM with K = T*mul1
            xt = (onehot.view(Z, T, 1, 1) * xs[i1].view(Z, 1, mul1, d)).view(Z, T * mul1, d)
            if d == 1:
                r = torch.mm(xt.view(Z, T * mul1), Wt)
            else:
                r = torch.einsum("zkm,kw->zwm", xt, Wt).reshape(Z, -1)
            outs[io] = r if outs[io] is None else outs[io] + r
        return self._assemble(outs, x)

    def extra_repr(self) -> str:
        return f"{self.irreps_in1} x {self.irreps_in2} -> {self.irreps_out} | {self.weight_numel} weights"


_NORMALIZE2MOM_CACHE = {}


def normalize2mom_const(act: Callable, key: str) -> float:
    """e3nn ``normalize2mom``: ``(E_{z~N(0,1)} act(z)^2)^-1/2`` from 1e6 seeded float64 samples."""
    if key not in _NORMALIZE2MOM_CACHE:
        gen = torch.Generator(device="cpu").manual_seed(0)
        z = torch.randn(1_000_000, generator=gen, dtype=torch.float64)
        cst = act(z).pow(2).mean().pow(-0.5).item()
        _NORMALIZE2MOM_CACHE[key] = 1.0 if abs(cst - 1.0) < 1e-4 else cst
    return _NORMALIZE2MOM_CACHE[key]


class Gate(torch.nn.Module):
    """``scalars (+) gates (+) gated -> act(scalars) (+) act(gates)[u] * gated[u, :]``."""

    def __init__(self, irreps_scalars, act_scalars: Sequence[Callable], irreps_gates, act_gates: Sequence[Callable],
                 irreps_gated):
        super().__init__()
        self.irreps_scalars = Irreps(irreps_scalars)
        self.irreps_gates = Irreps(irreps_gates)
        self.irreps_gated = Irreps(irreps_gated)
        assert all(ir.l == 0 for _, ir in self.irreps_scalars) and all(ir.l == 0 for _, ir in self.irreps_gates)
        assert self.irreps_gates.num_irreps == self.irreps_gated.num_irreps
        assert len(act_scalars) == len(self.irreps_scalars) and len(act_gates) == len(self.irreps_gates)
        self.act_scalars = list(act_scalars)
        self.act_gates = list(act_gates)
        self._cst_scalars = [normalize2mom_const(a, getattr(a, "__name__", repr(a))) for a in self.act_scalars]
        self._cst_gates = [normalize2mom_const(a, getattr(a, "__name__", repr(a))) for a in self.act_gates]
        self.irreps_in = (self.irreps_scalars + self.irreps_gates + self.irreps_gated).simplify()
        out_scalars = []
        x = torch.linspace(0, 10, 256, dtype=torch.float64)
        for (mul, ir), act in zip(self.irreps_scalars, self.act_scalars):
            p_out = ir.p
            if ir.p == -1:
                a1, a2 = act(x), act(-x)
                if (a1 - a2).abs().max() < 1e-5:
                    p_out = 1  # even activation turns odd scalars even
                elif (a1 + a2).abs().max() < 1e-5:
                    p_out = -1
                else:
                    raise ValueError("activation of an odd scalar must be even or odd")
            out_scalars.append((mul, (0, p_out)))
        self.irreps_out = Irreps(out_scalars) + self.irreps_gated
        names = {torch.nn.functional.silu: "silu", torch.tanh: "tanh"}
        self._kernel_meta = None
        if all(a in names for a in self.act_scalars + self.act_gates):
            self._kernel_meta = GateMeta(
                self.irreps_scalars, [(names[a], c) for a, c in zip(self.act_scalars, self._cst_scalars)],
                self.irreps_gates, [(names[a], c) for a, c in zip(self.act_gates, self._cst_gates)],
                self.irreps_gated,
            )
            self._op_key = _node_ops.gate_key(
                self.irreps_scalars, [(names[a], c) for a, c in zip(self.act_scalars, self._cst_scalars)],
                self.irreps_gates, [(names[a], c) for a, c in zip(self.act_gates, self._cst_gates)],
                self.irreps_gated,
            )

    @staticmethod
    def _activate(t, irreps, acts, csts):
        if len(irreps) == 1:
            r = acts[0](t)
            return r * csts[0] if csts[0] != 1.0 else r
        cols, off = [], 0
        for (mul, _), act, cst in zip(irreps, acts, csts):
            r = act(t[:, off : off + mul])
            cols.append(r * cst if cst != 1.0 else r)
            off += mul
        return torch.cat(cols, dim=-1)

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        if x.is_cuda and not traceable() and self._kernel_meta is not None and x.dtype in (torch.float32, torch.float64):
            # one fused launch per pass: forward, backward and (training) the backward's own backward
            return _gate_kernel(x, self._kernel_meta)
        if traceable() and x.is_cuda and x.dtype == torch.float32 and self._kernel_meta is not None:
            return _node_ops.gate_op(x, self._op_key)  # while tracing: the fused kernel as a dispatcher op
        ns, ng = self.irreps_scalars.dim, self.irreps_gates.dim
        if ng == 0:
            return self._activate(x, self.irreps_scalars, self.act_scalars, self._cst_scalars)
        sizes = [ns, ng] + [mul_ir.dim for mul_ir in self.irreps_gated]
        parts = torch.split(x, sizes, dim=1)
        scalars = self._activate(parts[0], self.irreps_scalars, self.act_scalars, self._cst_scalars)
        gates = self._activate(parts[1], self.irreps_gates, self.act_gates, self._cst_gates)
        Z = x.shape[0]
        gsplit = torch.split(gates, [mul for mul, _ in self.irreps_gated], dim=1) if len(self.irreps_gated) > 1 else (gates,)
        cols = [scalars]
        for (mul, ir), g, blk in zip(self.irreps_gated, gsplit, parts[2:]):
            cols.append((blk.view(Z, mul, ir.dim) * g.unsqueeze(-1)).view(Z, mul * ir.dim))
        return torch.cat(cols, dim=-1)


class NormActivation(torch.nn.Module):
    """``x_u -> act(|x_u|) / |x_u| * x_u`` per irrep copy ``u`` (``|x_u|^2 = sum_m x_{u m}^2``, clamped below at
    ``epsilon^2``): e3nn ``NormActivation(irreps, scalar_nonlinearity, normalize=True, epsilon=1e-8, bias=False)`` as
    ``ConvNetLayer`` builds it for ``nonlinearity_type="norm"`` (``nequip/nn/convnetlayer.py:116-125``).  Semantics
    restated from e3nn 0.5/0.6 [RECALLED: ``o3.Norm(squared=True)`` = plain sum of squares, the clamp at ``epsilon**2``
    before the square root, ``ElementwiseTensorProduct`` of a 0e scalar with an irrep = plain product].  Plain ATen ops
    (elementwise node-sized work off the benchmarked path; traceable as is)."""

    def __init__(self, irreps_in, scalar_nonlinearity: Callable, normalize: bool = True, epsilon: Optional[float] = None,
                 bias: bool = False):
        super().__init__()
        self.irreps_in = Irreps(irreps_in)
        self.irreps_out = Irreps(irreps_in)
        if epsilon is None and normalize:
            epsilon = 1e-8
        elif epsilon is not None and not normalize:
            raise ValueError("epsilon and normalize = False don't make sense together")
        elif not normalize:
            epsilon = 0.0
        self.epsilon = float(epsilon)
        self.scalar_nonlinearity = scalar_nonlinearity
        self.normalize = normalize
        self.bias = bias
        if bias:
            self.biases = torch.nn.Parameter(torch.zeros(self.irreps_in.num_irreps))
        self._sizes = [(m.mul, m.ir.dim) for m in self.irreps_in]

    def forward(self, features: torch.Tensor) -> torch.Tensor:
        Z = features.shape[0]
        blocks = torch.split(features, [mul * d for mul, d in self._sizes], dim=1) if len(self._sizes) > 1 else (features,)
        eps2 = self.epsilon * self.epsilon
        outs, off = [], 0
        for (mul, d), blk in zip(self._sizes, blocks):
            xb = blk.reshape(Z, mul, d)
            norms = xb.square().sum(dim=-1)
            if eps2 > 0:
                norms = torch.clamp(norms, min=eps2).sqrt()
            arg = norms + self.biases[off : off + mul] if self.bias else norms
            scal = self.scalar_nonlinearity(arg)
            if self.normalize:
                scal = scal / norms
            outs.append((xb * scal.unsqueeze(-1)).reshape(Z, mul * d))
            off += mul
        return torch.cat(outs, dim=1) if len(outs) > 1 else outs[0]
