"""``Adam`` / ``AdamW`` and ``ReduceLROnPlateau``: the optimizer and the scheduler of the reference's default training recipe
(``torch.optim.Adam`` driven by ``torch.optim.lr_scheduler.ReduceLROnPlateau``) on the multi-tensor HIP kernels ``nqa_adam_step`` /
``nqa_adam_grad_norm`` / ``nqa_adam_plateau`` (csrc/adam.hip).

    opt = Adam(model.parameters(), lr=1e-3, gradient_clip_val=1.0)       # AdamW(...): decoupled weight decay, 1e-2
    sched = ReduceLROnPlateau(opt, factor=0.5, patience=5)
    loss.backward(); opt.step(); opt.zero_grad(set_to_none=False)
    sched.step(validation_loss)                                          # a 0-d tensor (device or CPU) or a float

One step of a parameter is torch's ``_single_tensor_adam`` with ``p`` the parameter, ``m = exp_avg``, ``v = exp_avg_sq``::

    g = clip(p.grad);   maximize: g = -g;   s = step + 1;   bc1 = 1 - b1**s;   bc2 = 1 - b2**s
    coupled weight decay: g += wd*p;        decoupled: p *= 1 - lr*wd
    m = lerp(m, g, 1 - b1);   v = b2*v + (1 - b2)*g*g;   amsgrad: max_exp_avg_sq = max(max_exp_avg_sq, v), used for v below
    p -= (lr/bc1) * m/(sqrt(v)/sqrt(bc2) + eps);   step = s

The state names are torch's (``step``, ``exp_avg``, ``exp_avg_sq``, ``max_exp_avg_sq``); ``step`` is a 0-d float32 tensor on the
parameter's device, per parameter (one whose ``.grad`` is ``None`` is skipped and does not count), as torch's capturable and
fused forms keep it.  A state dict written by ``torch.optim.Adam`` / ``AdamW`` loads here and one written here loads there.

Why not torch's own: ``torch.optim.Adam(capturable=True)`` is some 47 launches per step at the train256 parameter set, it writes
the parameters behind the modules' weight-image caches (keyed on ``(data_ptr, _version)``), and its ``ReduceLROnPlateau`` writes a
Python float into ``param_groups`` that a captured step never sees.  Here the hyper-parameters of every group are a record in
device memory that the step reads and the scheduler's one-thread kernel rewrites; a step is one multi-tensor launch and a
one-thread-per-parameter launch that advances the counts (two more launches with clipping by norm), and the version counters of
everything written are bumped (``torch.autograd.graph.increment_version``).  Nothing is read by the host in ``step()`` or
``sched.step(tensor)``.

Gradient clipping (``gradient_clip_val`` / ``gradient_clip_algorithm``, the arguments of ``ConFIGGradients``): ``"norm"`` (the
default with a value) is ``clip_grad_norm_``'s factor ``min(1, clip/(norm + 1e-6))`` over all parameters of all groups that have a
``.grad``, ``"value"`` clamps every gradient element to +-clip (a NaN passes).  A non-finite norm behaves as
``clip_grad_norm_(error_if_nonfinite=False)``.  The clipped gradient is what the step uses; ``.grad`` ITSELF IS NOT MODIFIED -- a
deliberate difference from the trainer's flag, because ``.grad`` is only ever read here (``TrainingStatsMonitor`` and the gradient
all-reduce read it too).  ``opt.grad_norm`` is a 0-d float64 tensor with the norm before clipping.

Capture recipe: run ``step()`` once eagerly (the state tensors and the device tables are built eagerly, and rebuilt eagerly when
a parameter, its state or its ``.grad`` moved), keep the gradient buffers with ``zero_grad(set_to_none=False)``, then capture.
A rebuild under capture raises.

The learning rate has two writers.  Once the device tables exist the device record is the truth: ``state_dict()`` and
``get_last_lr()`` refresh ``param_groups[i]["lr"]`` from it (one copy to the host).  A host assignment
``param_groups[i]["lr"] = x`` that differs from the value last synchronised is written to the record by the next eager
``step()`` (a graph captured earlier then replays with it; under capture it raises); a scheduler step followed by an eager
``step()`` therefore keeps the scheduler's reduction.  Other changed hyper-parameters are written by the next eager ``step()`` too.

CPU tensors, and GPU tensors the kernels do not take (other dtypes than float32 / float64, non-contiguous ones, a ``.grad`` of
another dtype or layout), go through ``_aten_step``: the same equations as ATen ``_foreach`` calls with host scalars.  A mixture of
both kinds works eagerly and is refused under capture.  Sparse gradients and complex parameters raise.  A missing library raises
(``_lib.load``).
"""

from __future__ import annotations

import math
import weakref
from typing import Any, Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch

from .. import _lib
from ..utils import ktimer
from ._multi_tensor import _DT, ChunkTables, n_chunks, require_eager

_GROUP_WORDS = 8  # nqa_adam_group: lr, beta1, beta2, eps, weight_decay, amsgrad | maximize, decoupled | pad, min_lr
_LR, _MIN_LR = 0, 7
_PLATEAU_WORDS = 10  # nqa_adam_plateau_state
_STATE_NAMES = ("exp_avg", "exp_avg_sq", "max_exp_avg_sq")
_TORCH_ONLY_KEYS = ("foreach", "capturable", "differentiable", "fused")

# one table row: (parameter, .grad or None, exp_avg, exp_avg_sq, max_exp_avg_sq or None, step, index of the group)
_Row = Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor, Optional[torch.Tensor], torch.Tensor, int]


def _clip_factor(clip: float, norm: float) -> float:
    """``clip_grad_norm_``'s ``clamp(clip / (norm + 1e-6), max=1)``: a NaN stays."""
    coef = clip / (norm + 1e-6)
    return 1.0 if coef > 1.0 else coef


def _aten_step(rows: List[_Row], group: Dict[str, Any], factor: float, clip_value: Optional[float]) -> None:
    """The step of the rows of one group as ATen ``_foreach`` calls; the step counts are read by the host."""
    ps, gs, ms, vs, xs, steps = ([r[i] for r in rows] for i in range(6))
    lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], group["eps"], group["weight_decay"]
    if factor != 1.0:
        gs = torch._foreach_mul(gs, factor)
    if clip_value is not None:
        gs = [g.clamp(min=-clip_value, max=clip_value) for g in gs]
    if group["maximize"]:
        gs = torch._foreach_neg(gs)
    if wd != 0:
        if group["decoupled_weight_decay"]:
            torch._foreach_mul_(ps, 1.0 - lr * wd)
        else:
            gs = torch._foreach_add(gs, ps, alpha=wd)
    torch._foreach_lerp_(ms, gs, 1.0 - b1)
    torch._foreach_mul_(vs, b2)
    torch._foreach_addcmul_(vs, gs, gs, value=1.0 - b2)
    if group["amsgrad"]:
        torch._foreach_maximum_(xs, vs)
        denom = torch._foreach_sqrt(xs)
    else:
        denom = torch._foreach_sqrt(vs)
    counts = [float(s) + 1.0 for s in steps]
    torch._foreach_div_(denom, [math.sqrt(1.0 - b2 ** s) for s in counts])
    torch._foreach_add_(denom, eps)
    torch._foreach_addcdiv_(ps, ms, denom, [-(lr / (1.0 - b1 ** s)) for s in counts])
    torch._foreach_add_(steps, 1.0)


class _DeviceTables(ChunkTables):
    """The chunk tables of the parameters (``nqa_adam_tensor``: 8 words each), one record per parameter group
    (``nqa_adam_group``), the clipping record (``nqa_adam_clip``) and the partial sums of the norm."""

    def __init__(self, device: torch.device, n_tensors: int, capacity: int, n_groups: int, chunk: int):
        super().__init__(device, chunk, n_tensors, capacity, words=8)
        self.n_groups = n_groups
        self.groups = torch.zeros(n_groups, _GROUP_WORDS, dtype=torch.float64, device=device)
        self.clip = torch.tensor([0.0, 1.0, 0.0, math.inf], dtype=torch.float64, device=device)
        self.partials = torch.zeros(max(capacity, 1), dtype=torch.float64, device=device)
        self.hypers = None
        self.step_bytes = 0.0
        self.norm_bytes = 0.0

    def fits(self, device: torch.device, rows: List[_Row], n_groups: int) -> bool:
        return n_groups == self.n_groups and super().fits(device, [r[0].numel() for r in rows])

    def write(self, key, rows: List[_Row]) -> None:
        """(little-endian words: ``dtype`` is the low half of its word, ``group`` the high half)"""
        super().write(key, [r[0].numel() for r in rows], [
            [p.data_ptr(), 0 if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if x is None else x.data_ptr(),
             s.data_ptr(), p.numel(), _DT[p.dtype] | (gi << 32)] for p, g, m, v, x, s, gi in rows])
        stepped = [r for r in rows if r[1] is not None]
        self.step_bytes = float(sum((7 if r[4] is None else 9) * r[0].numel() * r[0].element_size() for r in stepped))
        self.norm_bytes = float(sum(r[0].numel() * r[0].element_size() for r in stepped))

    def write_hypers(self, param_groups, hypers, clip: Tuple[Optional[float], Optional[str]]) -> None:
        """Everything of the group records but ``lr`` and ``min_lr``, and the clipping record."""
        host = torch.zeros(len(param_groups), 6, dtype=torch.float64)
        words = host.view(torch.int64)
        for i, g in enumerate(param_groups):
            host[i, :4] = torch.tensor([g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"]], dtype=torch.float64)
            words[i, 4] = int(bool(g["amsgrad"])) | (int(bool(g["maximize"])) << 32)
            words[i, 5] = int(bool(g["decoupled_weight_decay"]))
        self.groups[:, 1:7].copy_(host)
        value, algorithm = clip
        self.clip.copy_(torch.tensor([0.0, 1.0, value if algorithm == "norm" else 0.0,
                                      value if algorithm == "value" else math.inf], dtype=torch.float64))
        self.hypers = hypers

    def write_lr(self, i: int, lr: float) -> None:
        self.groups[i, _LR:_LR + 1].copy_(torch.tensor([lr], dtype=torch.float64))


class Adam(torch.optim.Optimizer):
    """Adam on the fused multi-tensor kernels; see the module docstring.

    Args:
        params: parameters or parameter groups; every hyper-parameter up to ``decoupled_weight_decay`` can be set per group
        lr (float): learning rate
        betas (Tuple[float, float]): decay of the first and of the second moment
        eps (float): added to the root of the bias-corrected second moment
        weight_decay (float): coupled (added to the gradient) unless ``decoupled_weight_decay``
        amsgrad (bool): use the running maximum of the second moment
        maximize (bool): ascend
        decoupled_weight_decay (bool): AdamW's decay, ``p *= 1 - lr*weight_decay``
        gradient_clip_val (float, optional): clips the gradient the step uses (default ``None``: no clipping); ``.grad`` is left as it is
        gradient_clip_algorithm (str, optional): ``"norm"`` (the default with a value; ``clip_grad_norm_``'s factor) or ``"value"``
    """

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, amsgrad: bool = False, maximize: bool = False, decoupled_weight_decay: bool = False,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: Optional[str] = None):
        name = type(self).__name__
        if gradient_clip_val is None:
            gradient_clip_algorithm = None
        else:
            gradient_clip_algorithm = gradient_clip_algorithm or "norm"
            if gradient_clip_algorithm not in ("norm", "value"):
                raise ValueError(f"{name}: gradient_clip_algorithm must be 'norm' or 'value', found {gradient_clip_algorithm!r}")
            if not gradient_clip_val >= 0:
                raise ValueError(f"{name}: gradient_clip_val must not be negative, found {gradient_clip_val}")
        self.gradient_clip_val = None if gradient_clip_val is None else float(gradient_clip_val)
        self.gradient_clip_algorithm = gradient_clip_algorithm
        self._tables: Optional[_DeviceTables] = None  # while None `param_groups` holds lr; otherwise the device record does
        self._lr_synced: List[Optional[float]] = []  # lr of every group as last written to / read from the device
        self._schedulers = weakref.WeakSet()  # the ReduceLROnPlateau whose records follow the tables
        self._host_norm: Optional[torch.Tensor] = None
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                        decoupled_weight_decay=decoupled_weight_decay)
        super().__init__(params, defaults)

    # ---- groups ---------------------------------------------------------------------------------------------------------------
    def _hypers_of(self, group: Dict[str, Any]) -> tuple:
        """The validated hyper-parameters of a group without ``lr`` (which has two writers)."""
        lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        if not (lr >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps >= 0.0 and wd >= 0.0):
            raise ValueError(f"{type(self).__name__}: lr, eps, weight_decay >= 0 and betas in [0, 1) are required, got lr={lr}, "
                             f"betas={(b1, b2)}, eps={eps}, weight_decay={wd}")
        return float(b1), float(b2), eps, wd, bool(group["amsgrad"]), bool(group["maximize"]), bool(group["decoupled_weight_decay"])

    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        super().add_param_group(param_group)
        group = self.param_groups[-1]
        unknown = set(group) - set(self.defaults) - {"params"}
        if unknown:
            raise ValueError(f"{type(self).__name__}: unknown parameter-group options {sorted(unknown)}")
        self._hypers_of(group)
        if any(torch.is_complex(p) for p in group["params"]):
            raise ValueError(f"{type(self).__name__} does not support complex parameters")

    def _capturing(self) -> bool:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def _sync_lr(self) -> None:
        """``param_groups[i]["lr"]`` from the device records (one copy), except where a host assignment is pending."""
        if self._tables is None:
            return
        lrs = self._tables.groups[:, _LR].cpu().tolist()  # the one copy to the host
        for i, (group, lr) in enumerate(zip(self.param_groups, lrs)):
            if i < len(self._lr_synced) and self._lr_synced[i] is not None and float(group["lr"]) == self._lr_synced[i]:
                group["lr"] = self._lr_synced[i] = lr

    def _drop_tables(self) -> None:
        if self._tables is not None:
            self._sync_lr()
            for sched in list(self._schedulers):
                sched._leave_device()
            self._tables = None

    def _ensure_state(self) -> None:
        for group in self.param_groups:
            names = _STATE_NAMES if group["amsgrad"] else _STATE_NAMES[:2]
            for p in group["params"]:
                state = self.state[p]
                if "step" in state and all(n in state for n in names):
                    continue
                if self._capturing():
                    raise RuntimeError(f"{type(self).__name__}.step: call step() once eagerly before capturing it (the state "
                                       "tensors are built eagerly)")
                state.setdefault("step", torch.zeros((), dtype=torch.float32, device=p.device))
                for n in names:
                    state.setdefault(n, torch.zeros_like(p, memory_format=torch.preserve_format))

    # ---- which tensors go where ---------------------------------------------------------------------------------------------
    def _rows(self) -> Tuple[List[_Row], List[_Row], Optional[torch.device]]:
        """The parameters split into table rows of the kernels and rows of the ATen form, and the device of the former.  A
        parameter the kernels take whose ``.grad`` they do not take has a table row without ``.grad`` (skipped) and an ATen
        row; parameters without ``.grad`` have no ATen row."""
        native, rest = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                state = self.state[p]
                m, v, s = state["exp_avg"], state["exp_avg_sq"], state["step"]
                x = state["max_exp_avg_sq"] if group["amsgrad"] else None
                g = p.grad
                if g is not None and g.is_sparse:
                    raise RuntimeError(f"{type(self).__name__} does not support sparse gradients")
                on_kernel = (p.is_cuda and p.dtype in _DT and p.is_contiguous() and all(
                    t.device == p.device and t.dtype == p.dtype and t.is_contiguous() for t in (m, v, x) if t is not None)
                    and s.device == p.device and s.dtype == torch.float32 and s.dim() == 0)
                g_on_kernel = g is None or (g.device == p.device and g.dtype == p.dtype and g.is_contiguous())
                if on_kernel:
                    native.append((p, g if g_on_kernel else None, m, v, x, s, gi))
                if g is not None and not (on_kernel and g_on_kernel):
                    rest.append((p, g if g.dtype == p.dtype else g.to(p.dtype), m, v, x, s, gi))
        devices = {r[0].device for r in native}
        if len(devices) > 1:
            raise RuntimeError(f"{type(self).__name__}: the GPU parameters must be on one device, found {sorted(map(str, devices))}")
        return native, rest, (devices.pop() if devices else None)

    def _device_tables(self, device: torch.device, native: List[_Row]) -> _DeviceTables:
        key = tuple((p.data_ptr(), 0 if g is None else g.data_ptr(), m.data_ptr(), v.data_ptr(), 0 if x is None else x.data_ptr(),
                     s.data_ptr(), p.numel(), p.dtype, gi) for p, g, m, v, x, s, gi in native)
        hypers = (tuple(self._hypers_of(g) for g in self.param_groups), self.gradient_clip_val, self.gradient_clip_algorithm)
        n = len(self.param_groups)
        tables = self._tables
        same = tables is not None and tables.device == device and tables.n_groups == n and tables.key == key
        fresh = not same and (tables is None or not tables.fits(device, native, n))
        self._lr_synced = (self._lr_synced + [None] * n)[:n]
        # a host assignment of lr: it differs from the value last synchronised
        pending = [i for i, g in enumerate(self.param_groups) if self._lr_synced[i] != float(g["lr"])]
        if same and tables.hypers == hypers and not pending:
            return tables
        require_eager(f"{type(self).__name__}.step: call step() once eagerly before capturing it (the device tables are built, and "
                      "rewritten after a parameter, its state, its .grad or a hyper-parameter changed, eagerly; keep the gradient "
                      "buffers with zero_grad(set_to_none=False))")
        with torch.cuda.device(device):
            if fresh:
                self._drop_tables()  # (the groups without a pending assignment get the lr of the old records)
                chunk = int(_lib.load().nqa_ema_chunk_elems())
                tables = _DeviceTables(device, len(native), n_chunks([r[0].numel() for r in native], chunk), n, chunk)
                pending = list(range(n))
            if not same:
                tables.write(key, native)
            if tables.hypers != hypers:
                tables.write_hypers(self.param_groups, hypers, (self.gradient_clip_val, self.gradient_clip_algorithm))
            for i in pending:
                lr = float(self.param_groups[i]["lr"])
                tables.write_lr(i, lr)
                self._lr_synced[i] = lr
            if tables is not self._tables:
                self._tables = tables
                for sched in list(self._schedulers):
                    sched._to_device(tables)
        return tables

    # ---- the step -----------------------------------------------------------------------------------------------------------
    @property
    def grad_norm(self) -> Optional[torch.Tensor]:
        """The norm of all gradients before clipping, as of the last ``step()``: a 0-d float64 tensor (on the device of the
        kernels, where they run); ``None`` without clipping by norm."""
        if self.gradient_clip_algorithm != "norm":
            return None
        return self._tables.clip[0] if self._tables is not None else self._host_norm

    def _aten_norm(self, native: List[_Row], rest: List[_Row], device: Optional[torch.device]) -> float:
        grads = [r[1] for r in native if r[1] is not None] + [r[1] for r in rest]
        where = device if device is not None else torch.device("cpu")
        squares = [g.detach().double().square().sum().to(where) for g in grads]
        norm = torch.stack(squares).sum().sqrt() if squares else torch.zeros((), dtype=torch.float64, device=where)
        self._host_norm = norm
        return float(norm)

    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        """One step on every parameter that has a ``.grad`` (which is only read)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        name = type(self).__name__
        self._ensure_state()
        native, rest, device = self._rows()
        by_norm = self.gradient_clip_algorithm == "norm"
        clip_value = self.gradient_clip_val if self.gradient_clip_algorithm == "value" else None
        if not native:
            self._drop_tables()
            for group in self.param_groups:
                self._hypers_of(group)
        else:
            tables = self._device_tables(device, native)
            if rest:
                if self._capturing():
                    raise RuntimeError(f"{name}.step: tensors the kernels do not take (CPU tensors, other dtypes than float32 / "
                                       "float64, non-contiguous ones) cannot be captured: their step scalars are host numbers")
                self._sync_lr()
        factor = 1.0
        if by_norm and (rest or not native):  # the norm covers both kinds: formed by ATen, read by the host
            norm = self._aten_norm(native, rest, device)
            factor = _clip_factor(self.gradient_clip_val, norm)
            if native:
                tables.clip[:2].copy_(torch.tensor([norm, factor], dtype=torch.float64))
        for gi, group in enumerate(self.param_groups):
            rows = [r for r in rest if r[6] == gi]
            if rows:
                _aten_step(rows, group, factor, clip_value)
                torch.autograd.graph.increment_version([t for r in rows for t in (r[0], r[2], r[3], r[4], r[5]) if t is not None])
        if native:
            lib = _lib.load()
            with torch.cuda.device(device):
                if by_norm and not rest:
                    with ktimer.region("adam_grad_norm", tables.norm_bytes):
                        rc = lib.nqa_adam_grad_norm(_lib.ptr(tables.tensors), _lib.ptr(tables.chunks), tables.capacity,
                                                    _lib.ptr(tables.counts), _lib.ptr(tables.partials), _lib.ptr(tables.clip),
                                                    _lib.stream_ptr(device))
                    _lib.check(rc, "nqa_adam_grad_norm")
                with ktimer.region("adam_step", tables.step_bytes):
                    rc = lib.nqa_adam_step(_lib.ptr(tables.tensors), tables.n_tensors, _lib.ptr(tables.chunks), tables.capacity,
                                           _lib.ptr(tables.counts), _lib.ptr(tables.groups), tables.n_groups,
                                           _lib.ptr(tables.clip), _lib.stream_ptr(device))
                _lib.check(rc, "nqa_adam_step")
            torch.autograd.graph.increment_version(
                [t for r in native if r[1] is not None for t in (r[0], r[2], r[3], r[4], r[5]) if t is not None])
        return loss

    # ---- state dicts --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """(refreshes ``lr`` in ``param_groups`` from the device records first: one copy to the host)"""
        self._sync_lr()
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        """Takes a state dict of this class or of ``torch.optim.Adam`` / ``AdamW`` (its ``step`` values may be CPU tensors or
        numbers).  The loaded tensors are copied INTO the state tensors that exist (a captured step keeps its pointers); the
        hyper-parameters, ``lr`` included, reach the device records at the next eager ``step()``."""
        if self._capturing():
            raise RuntimeError(f"{type(self).__name__}.load_state_dict cannot be captured")
        state_dict = dict(state_dict)
        state_dict["param_groups"] = [{k: v for k, v in g.items() if k not in _TORCH_ONLY_KEYS} for g in state_dict["param_groups"]]
        old = {p: dict(s) for p, s in self.state.items()}
        super().load_state_dict(state_dict)
        for group in self.param_groups:
            for key, value in self.defaults.items():
                group.setdefault(key, value)
            self._hypers_of(group)
        for p, state in self.state.items():
            for name in _STATE_NAMES:
                prev, new = old.get(p, {}).get(name), state.get(name)
                if prev is not None and new is not None and prev.shape == new.shape and prev.dtype == new.dtype \
                        and prev.device == new.device:
                    prev.copy_(new)
                    state[name] = prev
                elif new is not None:
                    state[name] = new.clone(memory_format=torch.preserve_format)  # (never the caller's own tensor)
            if "step" in state:
                prev, new = old.get(p, {}).get("step"), state["step"]
                if not (torch.is_tensor(prev) and prev.dtype == torch.float32 and prev.dim() == 0 and prev.device == p.device):
                    prev = torch.zeros((), dtype=torch.float32, device=p.device)
                prev.copy_(new.detach().reshape(()) if torch.is_tensor(new) else torch.tensor(float(new)))
                state["step"] = prev
        self._lr_synced = [None] * len(self.param_groups)  # the loaded lr is a host assignment


class AdamW(Adam):
    """``Adam`` with decoupled weight decay (``torch.optim.AdamW``): ``weight_decay=1e-2`` by default."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 1e-2, amsgrad: bool = False, maximize: bool = False,
                 gradient_clip_val: Optional[float] = None, gradient_clip_algorithm: Optional[str] = None):
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize,
                         decoupled_weight_decay=True, gradient_clip_val=gradient_clip_val,
                         gradient_clip_algorithm=gradient_clip_algorithm)


class ReduceLROnPlateau:
    """``torch.optim.lr_scheduler.ReduceLROnPlateau`` by its rules and its state-dict keys.  With an ``Adam`` / ``AdamW`` of this
    module whose device tables exist, ``step`` is one launch of one thread (``nqa_adam_plateau``) that reads the metric through a
    device pointer and rewrites ``lr`` in the optimizer's device records, so that a captured ``step`` of the optimizer sees the
    reduction; with any other optimizer (or one whose parameters are all on the CPU) it is torch's rules on the host.

    ``step(metric)``: a float32 / float64 tensor of one element on the device of the kernels is read IN PLACE -- under capture it
    must be the same tensor on every replay (write new values into it).  A CPU tensor, another tensor or a float is copied into
    the scheduler's own one-element device buffer: eager only, it raises under capture.  To capture ``step``, construct the
    scheduler and run the optimizer's first eager ``step()`` before the capture (the scheduler's record follows the optimizer's
    tables to the device).

    The attributes ``best``, ``num_bad_epochs``, ``cooldown_counter``, ``last_epoch`` and ``_last_lr`` are current after
    ``state_dict()`` (two copies to the host); ``get_last_lr()`` copies the learning rates from the device once.
    """

    _PRIVATE = ("optimizer", "_record", "_metric", "_attached")

    def __init__(self, optimizer: torch.optim.Optimizer, mode: str = "min", factor: float = 0.1, patience: int = 10,
                 threshold: float = 1e-4, threshold_mode: str = "rel", cooldown: int = 0,
                 min_lr: Union[float, Sequence[float]] = 0, eps: float = 1e-8):
        if factor >= 1.0:
            raise ValueError("Factor should be < 1.0.")
        if not isinstance(optimizer, torch.optim.Optimizer):
            raise TypeError(f"{type(optimizer).__name__} is not an Optimizer")
        if mode not in ("min", "max"):
            raise ValueError("mode " + str(mode) + " is unknown!")
        if threshold_mode not in ("rel", "abs"):
            raise ValueError("threshold mode " + str(threshold_mode) + " is unknown!")
        self.factor = factor
        self.optimizer = optimizer
        if isinstance(min_lr, (list, tuple)):
            if len(min_lr) != len(optimizer.param_groups):
                raise ValueError(f"expected {len(optimizer.param_groups)} min_lrs, got {len(min_lr)}")
            self.default_min_lr = None
            self.min_lrs = list(min_lr)
        else:
            self.default_min_lr = min_lr
            self.min_lrs = [min_lr] * len(optimizer.param_groups)
        self.patience = patience
        self.cooldown = cooldown
        self.eps = eps
        self.last_epoch = 0
        self._last_lr = [g["lr"] for g in optimizer.param_groups]
        self.mode_worse = math.inf if mode == "min" else -math.inf
        self.mode = mode
        self.threshold = threshold
        self.threshold_mode = threshold_mode
        self.best = self.mode_worse
        self.cooldown_counter = 0
        self.num_bad_epochs = 0
        self._record: Optional[torch.Tensor] = None  # nqa_adam_plateau_state on the device; while None the attributes hold it
        self._metric: Optional[torch.Tensor] = None
        self._attached = None  # the optimizer's tables whose records hold min_lr
        schedulers = getattr(optimizer, "_schedulers", None)
        if isinstance(optimizer, Adam) and schedulers is not None:
            schedulers.add(self)
            if optimizer._tables is not None:
                self._to_device(optimizer._tables)

    # ---- host and device ------------------------------------------------------------------------------------------------------
    def _tables(self) -> Optional[_DeviceTables]:
        return self.optimizer._tables if isinstance(self.optimizer, Adam) else None

    def _min_lrs(self, n: int) -> List[float]:
        if len(self.min_lrs) != n:
            if self.default_min_lr is None:
                raise RuntimeError(f"The number of param groups in the `optimizer` ({n}) differs from when `ReduceLROnPlateau` "
                                   f"was initialized ({len(self.min_lrs)}), usually due to a new param group being added to the "
                                   "optimizer. Please modify the `min_lrs` field to match the length of the `optimizer` param "
                                   "groups.")
            self.min_lrs = [self.default_min_lr] * n
        return self.min_lrs

    def _to_device(self, tables: _DeviceTables) -> None:
        if self._record is not None and self._attached is tables:
            return
        require_eager("ReduceLROnPlateau.step: construct the scheduler and run the optimizer's first eager step() before capturing "
                      "(the scheduler's device record is built eagerly)")
        if self._record is not None and self._record.device != tables.device:
            self._sync()
            self._record = None
        if self._record is None:
            host = torch.zeros(_PLATEAU_WORDS, dtype=torch.float64)
            words = host.view(torch.int64)
            host[0], host[4], host[5], host[6] = self.best, self.factor, self.threshold, self.eps
            words[1], words[2], words[3] = int(self.num_bad_epochs), int(self.cooldown_counter), int(self.last_epoch)
            words[7], words[8] = int(self.patience), int(self.cooldown)
            words[9] = int(self.mode == "max") | (int(self.threshold_mode == "abs") << 32)
            self._record = host.to(tables.device)
            self._metric = torch.zeros(1, dtype=torch.float64, device=tables.device)
        min_lrs = self._min_lrs(tables.n_groups)
        tables.groups[:, _MIN_LR].copy_(torch.tensor([float(x) for x in min_lrs], dtype=torch.float64))
        self._attached = tables

    def _sync(self) -> None:
        if self._record is not None:
            host = self._record.cpu()
            words = host.view(torch.int64)
            self.best = float(host[0])
            self.num_bad_epochs, self.cooldown_counter, self.last_epoch = int(words[1]), int(words[2]), int(words[3])

    def _leave_device(self) -> None:
        self._sync()
        self._record = self._metric = self._attached = None

    # ---- the rules --------------------------------------------------------------------------------------------------------------
    def _is_better(self, a: float, best: float) -> bool:
        if self.mode == "min" and self.threshold_mode == "rel":
            return a < best * (1.0 - self.threshold)
        if self.mode == "min":
            return a < best - self.threshold
        if self.threshold_mode == "rel":
            return a > best * (self.threshold + 1.0)
        return a > best + self.threshold

    def _host_step(self, current: float) -> None:
        self.last_epoch += 1
        if self._is_better(current, self.best):
            self.best = current
            self.num_bad_epochs = 0
        else:
            self.num_bad_epochs += 1
        if self.cooldown_counter > 0:
            self.cooldown_counter -= 1
            self.num_bad_epochs = 0
        if self.num_bad_epochs > self.patience:
            groups = self.optimizer.param_groups
            for group, min_lr in zip(groups, self._min_lrs(len(groups))):
                old_lr = float(group["lr"])
                new_lr = max(old_lr * self.factor, min_lr)
                if old_lr - new_lr > self.eps:
                    if torch.is_tensor(group["lr"]):
                        group["lr"].fill_(new_lr)
                    else:
                        group["lr"] = new_lr
            self.cooldown_counter = self.cooldown
            self.num_bad_epochs = 0
        self._last_lr = [g["lr"] for g in self.optimizer.param_groups]

    def step(self, metrics) -> None:
        """One scheduler step on ``metrics``: a 0-d tensor (device or CPU) or a Python float."""
        tables = self._tables()
        if tables is None:
            if self._record is not None:
                self._leave_device()
            self._host_step(float(metrics))
            return
        self._to_device(tables)
        if torch.is_tensor(metrics) and metrics.device == tables.device and metrics.dtype in _DT and metrics.numel() == 1:
            metric = metrics.detach()
        else:
            require_eager("ReduceLROnPlateau.step: a metric that is not a float32 / float64 tensor on the device of the kernels is "
                          "copied by the host and cannot be captured")
            self._metric.copy_(torch.tensor([float(metrics)], dtype=torch.float64))
            metric = self._metric
        with torch.cuda.device(tables.device):
            rc = _lib.load().nqa_adam_plateau(_lib.ptr(metric), _DT[metric.dtype], _lib.ptr(self._record), _lib.ptr(tables.groups),
                                              tables.n_groups, _lib.stream_ptr(tables.device))
        _lib.check(rc, "nqa_adam_plateau")

    def get_last_lr(self) -> List[float]:
        """The learning rate of every group (copied from the device once, where the device holds it)."""
        if isinstance(self.optimizer, Adam):
            self.optimizer._sync_lr()
        self._last_lr = [g["lr"] for g in self.optimizer.param_groups]
        return self._last_lr

    @property
    def in_cooldown(self) -> bool:
        self._sync()
        return self.cooldown_counter > 0

    def state_dict(self) -> Dict[str, Any]:
        """torch's keys and values (everything but the optimizer), current as of this call."""
        self._sync()
        self.get_last_lr()
        return {key: value for key, value in self.__dict__.items() if key not in self._PRIVATE}

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        if torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("ReduceLROnPlateau.load_state_dict cannot be captured")
        self.__dict__.update({k: v for k, v in state_dict.items() if k not in self._PRIVATE})
        if self.mode not in ("min", "max") or self.threshold_mode not in ("rel", "abs"):
            raise ValueError(f"mode {self.mode!r} / threshold mode {self.threshold_mode!r} is unknown!")
        self.mode_worse = math.inf if self.mode == "min" else -math.inf
        attached, self._record, self._attached = self._attached, None, None  # (the record is rebuilt from the attributes)
        if attached is not None and attached is self._tables():
            self._to_device(attached)
