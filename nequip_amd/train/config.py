"""``ConFIGGradients``: conflict-free inverse gradients (ConFIG, arXiv 2408.11104) for losses of several terms -- the
framework-free form of the reference's ``nequip/train/config.py::ConFIGLightningModule._ConFIG_backwards`` plus its gradient
clipping, in the style of ``SimpleDDPStrategy`` and ``EMAWeights``::

    cf = ConFIGGradients(model, loss, norm_eps=1e-8, lsqr=True, gradient_clip_val=None, gradient_clip_algorithm=None)
    out = model(batch); loss_dict = loss(out, target, prefix=pfx)
    cf.backward(loss_dict, prefix=pfx)     # the conflict-free gradients are now in p.grad
    opt.step()

``loss`` is a ``MetricsManager``; the active terms are its entries whose ``coeff`` is not ``None``, in entry order, and the
coefficients are the ``b`` of the method's ``A x = b`` (read at every eager call).  One backward pass per term gives the rows
``g_k`` of ``A``; the reference normalises the rows, solves the underdetermined system on the ``[K, P]`` matrix with
``torch.linalg.lstsq`` (or ``pinv``: its docstring names ROCm as a device that may not do the former), and reads results back on
the host.  Both branches are the minimum-norm solution, every number of which is a function of the K x K Gram matrix, and the
new gradient is a linear combination of the ``g_k`` (``gram_weights`` below is that arithmetic in ATen).  On the GPU this is
``csrc/config.hip``: ``nqa_config_collect`` after each backward pass (copies every ``.grad`` into row k of a buffer and zeroes
it, one launch), ``nqa_config_gram`` (a fixed-order two-stage reduction in double, then cyclic Jacobi on the K x K matrix) and
``nqa_config_apply`` (writes ``sum_l w_l g_l`` into every ``.grad``, clipping folded in).  Nothing is read by the host, so the
whole step -- forward, K backward passes, ConFIG, a capturable optimizer -- captures into one hipGraph.

Differences from the reference, all deliberate:

1. *Frozen parameters.*  Only parameters with ``requires_grad=True`` take part.  The reference also assigns a zero ``.grad`` to
   frozen parameters (a decoupled weight decay then decays them); here their ``.grad`` is not touched.
2. *Pointer-stable gradients.*  On the kernels every participating parameter gets a ``.grad`` the first time ``backward`` runs
   eagerly, and keeps it: autograd accumulates into it in place, the collect kernel zeroes it after copying, the apply kernel
   overwrites it.  No ``zero_grad`` is needed; after ``zero_grad(set_to_none=True)`` the next eager call rebuilds the tables.
3. *Arithmetic in float64*, whatever the dtype of the gradients (the reference computes in the promoted dtype of the gradients,
   float32 for an all-float32 model).  The ``[K, P]`` buffer is float64 if any participating parameter is, else float32 (the
   reference's ``torch.cat`` promotion; float32 widens exactly), and every written gradient is rounded once, to its parameter's
   dtype.

Eigenvalues of the normalised Gram matrix at or below ``TAU = 1e-12`` of the largest are dropped.  The constant is documented,
not measured: a Gram matrix in double resolves nothing below about K 2^-52, and the reference's own cut-offs on singular values
(eps for ``gelsy``, P eps for ``pinv``) correspond to eigenvalue ratios of 1e-19 and below, which no Gram matrix can reach; the
two forms differ only for gradients parallel to within about 1e-6 rad.

CPU tensors, and parameter lists with a tensor the kernels do not take (other dtypes than float32 / float64, non-contiguous),
take the ATen form for the WHOLE call: the reference's lines, ``lsqr`` included, in float64.  On the kernels ``lsqr`` has no
effect.  A missing library raises (``_lib.load``).

Graph capture follows ``EMAWeights``: the device tables and the coefficient vector are written eagerly and in place; building
or rebuilding them while the stream is capturing raises (call ``backward`` once eagerly first).  After ``loss.set_coeffs``
between replays, ``sync_coefficients()`` rewrites the vector.  The data-parallel all-reduce is eager only.
"""

from __future__ import annotations

import ctypes
import math
from typing import List, Optional, Tuple

import torch
import torch.distributed as dist

from .. import _lib
from ..utils import ktimer
from ._multi_tensor import _DT, ChunkTables, n_chunks, require_eager

_CLIP = {None: 0, "norm": 1, "value": 2}
MAX_TERMS = 8
TAU = 1e-12
_NO_ACTIVE = ("At least one active loss component is required for training, i.e. at least on component in the loss function "
              "must have `coeff` that is not `None`.")


def _jacobi_eigh(a: List[List[float]]) -> Tuple[List[float], List[List[float]]]:
    """Eigenvalues and eigenvectors (in columns) of a small symmetric matrix by cyclic Jacobi in Python doubles: the rotations
    of ``config_solve`` (csrc/config.hip), one by one.  Unlike LAPACK's ``eigh`` (absolute accuracy, ``2^-53 lambda_max``)
    Jacobi keeps the RELATIVE accuracy of small eigenvalues, which a gradient of norm below ``eps`` produces."""
    k = len(a)
    a = [row[:] for row in a]
    v = [[1.0 if i == j else 0.0 for j in range(k)] for i in range(k)]
    for _ in range(30):
        off = sum(a[i][j] ** 2 for i in range(k) for j in range(i + 1, k))
        if not off > 1.2e-32 * sum(a[i][i] ** 2 for i in range(k)):
            break
        for i in range(k - 1):
            for j in range(i + 1, k):
                if a[i][j] == 0.0:
                    continue
                theta = (a[j][j] - a[i][i]) / (2.0 * a[i][j])
                t = math.copysign(1.0, theta) / (abs(theta) + math.hypot(theta, 1.0)) if math.isfinite(theta) else 0.0
                cs = 1.0 / math.sqrt(t * t + 1.0)
                sn = t * cs
                for r in range(k):
                    a[r][i], a[r][j] = cs * a[r][i] - sn * a[r][j], sn * a[r][i] + cs * a[r][j]
                for r in range(k):
                    a[i][r], a[j][r] = cs * a[i][r] - sn * a[j][r], sn * a[i][r] + cs * a[j][r]
                for r in range(k):
                    v[r][i], v[r][j] = cs * v[r][i] - sn * v[r][j], sn * v[r][i] + cs * v[r][j]
    return [a[i][i] for i in range(k)], v


def gram_weights(gram: torch.Tensor, b: torch.Tensor, eps: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(w, |new_grad|)`` from the Gram matrix ``G_kl = g_k . g_l`` [K, K] and the coefficients ``b`` [K], in float64 ATen (the
    K x K diagonalisation on the host): the arithmetic of ``csrc/config.hip``, ``new_grad = sum_l w_l g_l``."""
    gram, b = gram.double(), b.double()
    n = gram.diagonal().clamp_min(0.0).sqrt().clamp_min(eps)
    gh = gram / (n[:, None] * n[None, :])
    bh = b / b.norm().clamp_min(eps)
    lam, vec = _jacobi_eigh(gh.tolist())
    lam, vec = gram.new_tensor(lam), gram.new_tensor(vec)
    keep = lam > TAU * lam.max()
    inv = torch.where(keep, 1.0 / torch.where(keep, lam, torch.ones_like(lam)), torch.zeros_like(lam))
    c = vec @ (inv * (vec.t() @ bh))
    xi = (c @ gh @ c).clamp_min(0.0).sqrt()
    d = xi.clamp_min(eps)
    s = (gram @ (c / n)).sum() / d
    return s * c / (n * d), s.abs() * xi / d


def solve_host(gram: torch.Tensor, b: torch.Tensor, eps: float, clip_algorithm: Optional[str] = None,
               clip_val: float = 0.0) -> torch.Tensor:
    """The solve of ``nqa_config_gram`` run on the host by the library (the function the kernel runs; for tests without a GPU):
    ``[w_0 .. w_7, |new_grad|, clip factor]`` from a float64 Gram matrix [K, K] and ``b`` [K]."""
    k = gram.shape[0]
    tri = torch.stack([gram[i, j] for i in range(k) for j in range(i, k)]).double().contiguous()
    b = b.double().contiguous()
    out = torch.zeros(MAX_TERMS + 2, dtype=torch.float64)
    rc = _lib.load().nqa_config_solve_host(ctypes.c_void_p(tri.data_ptr()), k, ctypes.c_void_p(b.data_ptr()), float(eps),
                                           _CLIP[clip_algorithm], float(clip_val), ctypes.c_void_p(out.data_ptr()))
    _lib.check(rc, "nqa_config_solve_host")
    return out


class _DeviceTables(ChunkTables):
    """The chunk tables of the gradients (``nqa_ema_tensor``: 4 words each), ``numel_dev = [P]``, the ``[K, row_stride]`` buffer of
    collected gradients (``row_stride``: P rounded up to 4 elements, the pad zero), the partial Gram products, ``b`` and ``out =
    [w_0 .. w_7, |new_grad|, clip factor]``.  Rewritten in place when only the addresses of the gradients change."""

    def __init__(self, device: torch.device, grads: List[torch.Tensor], n_terms: int, buf_dtype: torch.dtype):
        lib = _lib.load()
        chunk, self.gram_chunk = int(lib.nqa_ema_chunk_elems()), int(lib.nqa_config_gram_chunk_elems())
        super().__init__(device, chunk, len(grads), n_chunks([g.numel() for g in grads], chunk), words=4)
        self.n_terms, self.buf_dtype = n_terms, buf_dtype
        self.shapes = [(g.numel(), g.dtype) for g in grads]
        self.numel = sum(g.numel() for g in grads)
        self.row_stride = -(-self.numel // 4) * 4
        self.gram_capacity = -(-self.numel // self.gram_chunk)
        self.numel_dev = torch.tensor([self.numel], dtype=torch.int64, device=device)
        self.buf = torch.zeros(n_terms, max(self.row_stride, 4), dtype=buf_dtype, device=device)
        self.partials = torch.zeros(max(self.gram_capacity, 1) * (MAX_TERMS * (MAX_TERMS + 1) // 2), dtype=torch.float64,
                                    device=device)
        self.b = torch.zeros(MAX_TERMS, dtype=torch.float64, device=device)
        self.out = torch.zeros(MAX_TERMS + 2, dtype=torch.float64, device=device)

    def fits(self, device: torch.device, grads: List[torch.Tensor], n_terms: int, buf_dtype: torch.dtype) -> bool:
        return (device == self.device and n_terms == self.n_terms and buf_dtype == self.buf_dtype
                and [(g.numel(), g.dtype) for g in grads] == self.shapes)

    def write(self, key, grads: List[torch.Tensor]) -> None:
        """(little-endian words: the int32 ``dtype`` is the low half of its word, the pad 0)"""
        esz, rows, start = self.buf.element_size(), [], 0
        for g in grads:
            rows.append([g.data_ptr(), self.buf.data_ptr() + start * esz, g.numel(), _DT[g.dtype]])
            start += g.numel()
        assert start == self.numel
        super().write(key, [g.numel() for g in grads], rows)


class ConFIGGradients:
    """Conflict-free gradients of a loss of several terms (see the module docstring).

    Args:
        model (torch.nn.Module): its parameters with ``requires_grad=True`` take part
        loss (MetricsManager): the terms are its entries with a ``coeff``; the coefficients are ConFIG's ``b``
        norm_eps (float): floor of the three normalisations (default ``1e-8``)
        lsqr (bool): ATen form only: ``torch.linalg.lstsq`` (default) or ``torch.linalg.pinv``; both are the minimum-norm
            solution, which is what the kernels compute
        gradient_clip_val (float, optional): clips the new gradient (default ``None``: no clipping)
        gradient_clip_algorithm (str, optional): ``"norm"`` (the default with a value; ``clip_grad_norm_``'s factor) or ``"value"``
        group: the ``torch.distributed`` process group whose ranks share the model (default: the world)

    Attributes (device tensors; nothing reads them on the host unless the caller does):
        weights: ``[K]`` float64, ``new_grad = sum_l weights[l] g_l`` (clipping by norm included)
        grad_norm: 0-d float64, the norm of the new gradient BEFORE clipping (what ``clip_grad_norm_`` returns)
    """

    def __init__(self, model: torch.nn.Module, loss, norm_eps: float = 1e-8, lsqr: bool = True,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: Optional[str] = None, group=None):
        if gradient_clip_val is None:
            gradient_clip_algorithm = None
        else:
            gradient_clip_algorithm = gradient_clip_algorithm or "norm"
            if gradient_clip_algorithm not in ("norm", "value"):
                raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value', found {gradient_clip_algorithm!r}")
            if not gradient_clip_val >= 0:
                raise ValueError(f"gradient_clip_val must not be negative, found {gradient_clip_val}")
        if not norm_eps >= 0:
            raise ValueError(f"norm_eps must not be negative, found {norm_eps}")
        self.model, self.loss, self.norm_eps, self.lsqr, self.group = model, loss, float(norm_eps), bool(lsqr), group
        self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self.weights: Optional[torch.Tensor] = None
        self.grad_norm: Optional[torch.Tensor] = None
        self._tables: Optional[_DeviceTables] = None
        self._rows: Optional[torch.Tensor] = None  # the ATen form's [K, P]

    # ---- what takes part ---------------------------------------------------------------------------------------------------
    def _active(self) -> List[Tuple[str, float]]:
        return [(name, float(e.coeff)) for name, e in self.loss.entries.items() if e.coeff is not None]

    def _world_size(self) -> int:
        return dist.get_world_size(self.group) if dist.is_available() and dist.is_initialized() else 1

    def component_gradients(self) -> torch.Tensor:
        """The ``[K, P]`` gradients of the terms as collected by the last ``backward`` (after the all-reduce, if any); P runs
        over the participating parameters in ``model.parameters()`` order.  On the kernels a view of their buffer."""
        if self._tables is not None:
            return self._tables.buf[:, :self._tables.numel]
        if self._rows is None:
            raise RuntimeError("ConFIGGradients.component_gradients: no backward with two or more active terms has run")
        return self._rows

    def sync_coefficients(self) -> None:
        """Write the coefficients of ``loss`` to the device vector the kernels read, in place (every eager ``backward`` does
        this; call it after ``loss.set_coeffs`` between the replays of a captured step).  Raises if there is no such vector
        yet, or if the number of active terms is no longer the one the tables (and a captured step) were built for."""
        active = self._active()
        if self._tables is None:
            raise RuntimeError("ConFIGGradients.sync_coefficients: no backward has run on the kernels yet")
        if len(active) != self._tables.n_terms:
            raise RuntimeError(f"ConFIGGradients.sync_coefficients: {len(active)} active loss terms, the device tables were "
                               f"built for {self._tables.n_terms}; call backward eagerly (and capture again)")
        self._tables.b[:len(active)].copy_(torch.tensor([c for _, c in active], dtype=torch.float64))

    def _all_reduce(self, rows: torch.Tensor) -> None:
        if self._world_size() == 1:
            return
        if rows.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ConFIGGradients.backward: the data-parallel all-reduce cannot be captured")
        if dist.get_backend(self.group) == "gloo":
            dist.all_reduce(rows, op=dist.ReduceOp.SUM, group=self.group)
            rows /= dist.get_world_size(self.group)
        else:
            dist.all_reduce(rows, op=dist.ReduceOp.AVG, group=self.group)

    # ---- the method ----------------------------------------------------------------------------------------------------------
    def backward(self, loss_dict, prefix: str = "") -> None:
        """``loss_dict``: what ``loss(out, target, prefix=prefix)`` returned for this step."""
        active = self._active()
        world = self._world_size()
        if len(active) == 0:
            raise RuntimeError(_NO_ACTIVE)
        if len(active) == 1:  # nothing to resolve
            (loss_dict[f"{prefix}weighted_sum"] * world).backward()
            return
        if len(active) > MAX_TERMS:
            raise ValueError(f"ConFIGGradients takes at most {MAX_TERMS} active loss terms, found {len(active)}")
        params = [p for p in self.model.parameters() if p.requires_grad]
        devices = {p.device for p in params}
        if len(devices) > 1:
            raise RuntimeError(f"ConFIGGradients: all parameters must be on one device, found {sorted(map(str, devices))}")
        terms = [loss_dict[f"{prefix}{name}"] * world for name, _ in active]
        on_kernels = bool(params) and all(
            p.is_cuda and p.dtype in _DT and p.is_contiguous()
            and (p.grad is None or (p.grad.dtype == p.dtype and p.grad.is_contiguous() and p.grad.layout == torch.strided))
            for p in params)
        if on_kernels:
            self._native_backward(params, terms, [c for _, c in active], devices.pop())
        else:
            self._aten_backward(params, terms, [c for _, c in active])

    def _device_tables(self, device, params, n_terms: int) -> _DeviceTables:
        hint = ("ConFIGGradients.backward: call backward once eagerly before capturing it (the gradients of the parameters are "
                "allocated and the device tables built, and rebuilt after the gradients moved, eagerly)")
        if any(p.grad is None for p in params):
            require_eager(hint)
            for p in params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
        grads = [p.grad for p in params]
        key = (n_terms,) + tuple((g.data_ptr(), g.numel(), g.dtype) for g in grads)
        tables = self._tables
        if tables is not None and tables.key == key and tables.device == device:
            return tables
        require_eager(hint)
        buf_dtype = torch.float64 if any(g.dtype == torch.float64 for g in grads) else torch.float32
        with torch.cuda.device(device):
            if tables is None or not tables.fits(device, grads, n_terms, buf_dtype):
                tables = _DeviceTables(device, grads, n_terms, buf_dtype)
            tables.write(key, grads)
        self._tables, self._rows = tables, None
        return tables

    def _collect(self, t: _DeviceTables, row: int) -> None:
        """One ``nqa_config_collect`` launch: row ``row`` of the buffer = every ``.grad``, then ``.grad`` = 0 (``row < 0``: only
        the zeros)."""
        nbytes = t.numel * t.buf.element_size()
        with torch.cuda.device(t.device), ktimer.region("config_collect", 3.0 * nbytes):
            rc = _lib.load().nqa_config_collect(_lib.ptr(t.tensors), _lib.ptr(t.chunks), t.capacity, _lib.ptr(t.counts), row,
                                                t.row_stride, _DT[t.buf_dtype], _lib.stream_ptr(t.device))
        _lib.check(rc, "nqa_config_collect")

    def _combine(self, t: _DeviceTables) -> None:
        """``nqa_config_gram`` and ``nqa_config_apply``: from the collected rows to the new gradient in every ``.grad``."""
        lib, k = _lib.load(), t.n_terms
        clip_mode, clip = _CLIP[self.gradient_clip_algorithm], float(self.gradient_clip_val or 0.0)
        nbytes = t.numel * t.buf.element_size()
        with torch.cuda.device(t.device):
            with ktimer.region("config_gram", float(k * nbytes)):
                rc = lib.nqa_config_gram(_lib.ptr(t.buf), _DT[t.buf_dtype], k, t.row_stride, _lib.ptr(t.numel_dev),
                                         t.gram_capacity, _lib.ptr(t.partials), _lib.ptr(t.b), self.norm_eps, clip_mode, clip,
                                         _lib.ptr(t.out), _lib.stream_ptr(t.device))
            _lib.check(rc, "nqa_config_gram")
            with ktimer.region("config_apply", float((k + 1) * nbytes)):
                rc = lib.nqa_config_apply(_lib.ptr(t.tensors), _lib.ptr(t.chunks), t.capacity, _lib.ptr(t.counts), k, t.row_stride,
                                          _DT[t.buf_dtype], _lib.ptr(t.out), clip_mode, clip, _lib.stream_ptr(t.device))
            _lib.check(rc, "nqa_config_apply")

    def _native_backward(self, params, terms, coeffs, device) -> None:
        k = len(terms)
        t = self._device_tables(device, params, k)
        if not torch.cuda.is_current_stream_capturing():
            t.b[:k].copy_(torch.tensor(coeffs, dtype=torch.float64))
        self._collect(t, -1)  # the gradients of the previous step must not leak in
        for i, term in enumerate(terms):
            term.backward(retain_graph=i < k - 1)
            self._collect(t, i)
        self._all_reduce(t.buf)
        self._combine(t)
        torch.autograd.graph.increment_version([p.grad for p in params])
        self.weights, self.grad_norm = t.out[:k], t.out[MAX_TERMS]

    def _aten_backward(self, params, terms, coeffs) -> None:
        """The reference's lines (in float64; clipping as ``clip_grad_norm_`` / ``clip_grad_value_`` apply it afterwards)."""
        self._tables = None
        k, rows = len(terms), []
        for p in params:
            p.grad = None
        for i, term in enumerate(terms):
            term.backward(retain_graph=i < k - 1)
            rows.append(torch.cat([(p.grad if p.grad is not None else torch.zeros_like(p)).flatten() for p in params]))
            for p in params:
                p.grad = None
        a_raw = torch.stack(rows, dim=0)
        self._all_reduce(a_raw)
        self._rows = a_raw
        a_raw = a_raw.double()
        eps = self.norm_eps
        a = torch.nn.functional.normalize(a_raw, dim=1, eps=eps)
        b = torch.nn.functional.normalize(torch.tensor(coeffs, dtype=a.dtype, device=a.device), dim=0, eps=eps)
        x = torch.linalg.lstsq(a, b).solution if self.lsqr else torch.linalg.pinv(a) @ b
        x = torch.nn.functional.normalize(x, dim=0, eps=eps)
        new_grad = torch.sum(a_raw * x) * x
        w, norm = gram_weights(a_raw @ a_raw.t(), b, eps)
        if self.gradient_clip_algorithm == "norm":
            factor = (self.gradient_clip_val / (new_grad.norm() + 1e-6)).clamp(max=1.0)
            new_grad, w = new_grad * factor, w * factor
        self.weights, self.grad_norm = w, norm
        start = 0
        for p in params:
            g = new_grad.narrow(0, start, p.numel()).to(dtype=p.dtype).view(p.shape)
            if self.gradient_clip_algorithm == "value":
                g = g.clamp(min=-self.gradient_clip_val, max=self.gradient_clip_val)
            p.grad = g.clone()
            start += p.numel()
