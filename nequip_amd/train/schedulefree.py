"""``AdamWScheduleFree``: schedule-free AdamW (Defazio et al., "The Road Less Scheduled") on the multi-tensor HIP kernels
``nqa_sfree_step`` / ``nqa_sfree_swap`` (csrc/schedulefree.hip), and ``ScheduleFreeHooks``: the hooks of the reference's
``nequip/train/schedulefree.py::ScheduleFreeLightningModule`` without the Lightning dependency.

    opt = AdamWScheduleFree(model.parameters(), lr=2.5e-3, warmup_steps=100)
    opt.train()                                  # the parameters hold y, the point at which gradients are taken
    loss.backward(); opt.step(); opt.zero_grad(set_to_none=False)
    opt.eval()                                   # the parameters hold x, the averaged weights, for validation and saving
    with opt.averaged_parameters(): ...          # the same for a block

One step of a parameter group, with ``y`` the parameter, ``z`` and ``exp_avg_sq`` (``v``) its state::

    sched = (k+1)/warmup_steps if k < warmup_steps else 1;   bc2 = 1 - b2**(k+1);   lr_k = lr*sched  (-> scheduled_lr)
    lr_max = max(lr_k, lr_max);   weight = (k+1)**r * lr_max**weight_lr_power
    weight_sum += weight;   c = weight/weight_sum  (0 if weight_sum == 0)
    v = b2*v + (1-b2)*g*g;   gn = g/(sqrt(v/bc2) + eps) + wd*y
    y = lerp(y, z, c) + lr_k*(b1*(1-c) - 1)*gn;   z = z - lr_k*gn;   k += 1

``eval()`` is ``p = lerp(p, z, 1 - 1/b1)`` and ``train()`` is ``p = lerp(p, z, 1 - b1)``, each a no-op in its own mode.

Why not the published ``schedulefree`` package: its step scalars (``k``, the warm-up, the bias correction, ``weight_sum``,
``c``) are Python numbers, which a hipGraph captured at step ``k`` freezes; one step is about ten ``foreach`` launches per group;
and it writes the parameters behind the modules' weight-image caches, which are keyed on ``(data_ptr, _version)``.  Here
hyper-parameters and group state are a record in device memory from which the kernel forms the scalars, a step is one
multi-tensor launch and a one-thread-per-group launch that advances the state, and the version counters of everything written
are bumped (``torch.autograd.graph.increment_version``).

Capture recipe: run ``step()`` once eagerly (the state tensors and the device tables are built eagerly, and rebuilt eagerly when
a parameter, its state or its ``.grad`` moved), keep the gradient buffers with ``zero_grad(set_to_none=False)``, then capture.
A rebuild under capture raises.  A changed hyper-parameter (``param_groups[i]["lr"] = ...``) is written to the device record,
in place, by the next eager ``step()`` -- a graph captured earlier then replays with the new value; under capture it raises.
``train()`` / ``eval()`` are host state and are refused under capture.

CPU tensors, and GPU tensors the kernels do not take (other dtypes than float32 / float64, non-contiguous ones, a ``.grad`` of
another dtype), go through ``_aten_step``: the same equations as ATen ``_foreach`` calls with host scalars.  A mixture of both
kinds works eagerly (the group state is then read from the device once per step) and is refused under capture.  A missing
library raises (``_lib.load``).

Deliberate differences from the published package:

* ``.grad`` is left untouched (the package overwrites it with the normalised gradient): ``TrainingStatsMonitor`` and the
  gradient all-reduce read it;
* ``z`` and ``exp_avg_sq`` exist for every parameter from the first ``step()`` / ``train()`` on, also for one whose ``.grad`` is
  ``None`` (it is skipped by the step, its state untouched); the first step of a group reads ``z`` as the parameter, as the
  package's lazy initialisation does;
* the group state (``k``, ``weight_sum``, ``lr_max``, ``scheduled_lr``) in ``param_groups`` is current after ``state_dict()``,
  which copies the device records to the host once; nothing else does;
* ``eval()`` with ``beta1 == 0`` raises (the averaged weights cannot be recovered from ``y = z``).

The state-dict keys (``z``, ``exp_avg_sq`` per parameter; ``k``, ``weight_sum``, ``lr_max``, ``scheduled_lr``, ``train_mode`` per
group) are the package's names as far as known; loading a file written by the package itself is not tested (the package is not a
dependency).
"""

from __future__ import annotations

import contextlib
import copy
from typing import Any, Callable, Dict, List, Optional, Tuple

import torch

from .. import _lib
from ..utils import ktimer
from ._multi_tensor import _DT, ChunkTables, n_chunks, require_eager

_GROUP_WORDS = 12  # nqa_sfree_group: lr, beta1, beta2, eps, weight_decay, r, weight_lr_power, warmup_steps | k, weight_sum, lr_max, scheduled_lr
_N_HYPER_WORDS = 8
CHECKPOINT_KEY = "schedulefree_optimizer_state_dict"

# one table row: (parameter, .grad or None, z, exp_avg_sq, index of the group)
_Row = Tuple[torch.Tensor, Optional[torch.Tensor], torch.Tensor, torch.Tensor, int]


def _step_scalars(group: Dict[str, Any]) -> Dict[str, float]:
    """The scalars of the step that follows the state in ``group``, in Python doubles (what the kernel forms on the device)."""
    k, warmup = int(group["k"]), int(group["warmup_steps"])
    b1, b2 = group["betas"]
    sched = (k + 1) / warmup if k < warmup else 1.0
    bc2 = 1.0 - b2 ** (k + 1)
    lr_k = group["lr"] * sched
    lr_max = max(lr_k, group["lr_max"])
    weight = ((k + 1) ** group["r"]) * (lr_max ** group["weight_lr_power"])
    weight_sum = group["weight_sum"] + weight
    c = weight / weight_sum if weight_sum != 0.0 else 0.0
    return {"bc2": bc2, "lr_k": lr_k, "lr_max": lr_max, "weight_sum": weight_sum, "c": c,
            "a": lr_k * (b1 * (1.0 - c) - 1.0)}


def _aten_step(rows: List[_Row], group: Dict[str, Any], s: Dict[str, float]) -> None:
    ys, gs, zs, vs = ([r[i] for r in rows] for i in range(4))
    b2 = group["betas"][1]
    if int(group["k"]) == 0:
        for z, y in zip(zs, ys):
            z.copy_(y)
    torch._foreach_mul_(vs, b2)
    torch._foreach_addcmul_(vs, gs, gs, value=1.0 - b2)
    denom = torch._foreach_div(vs, s["bc2"])
    torch._foreach_sqrt_(denom)
    torch._foreach_add_(denom, group["eps"])
    gn = torch._foreach_div(gs, denom)
    torch._foreach_add_(gn, ys, alpha=group["weight_decay"])
    torch._foreach_lerp_(ys, zs, s["c"])
    torch._foreach_add_(ys, gn, alpha=s["a"])
    torch._foreach_sub_(zs, gn, alpha=s["lr_k"])


def _swap_weight(b1: float, to_eval: bool) -> float:
    return 1.0 - 1.0 / b1 if to_eval else 1.0 - b1


def _strip_grads(key):
    return None if key is None else tuple(row[:1] + row[2:] for row in key)


class _DeviceTables(ChunkTables):
    """The chunk tables of the parameters (``nqa_sfree_tensor``: 6 words each) and one record per parameter group
    (``nqa_sfree_group``), rewritten in place when the hyper-parameters change."""

    def __init__(self, device: torch.device, n_tensors: int, capacity: int, n_groups: int, chunk: int):
        super().__init__(device, chunk, n_tensors, capacity, words=6)
        self.n_groups = n_groups
        self.groups = torch.zeros(n_groups, _GROUP_WORDS, dtype=torch.float64, device=device)
        self.hypers = None
        self.step_bytes = 0.0
        self.swap_bytes = 0.0

    def fits(self, device: torch.device, rows: List[_Row], n_groups: int) -> bool:
        return n_groups == self.n_groups and super().fits(device, [r[0].numel() for r in rows])

    def write(self, key, rows: List[_Row]) -> None:
        """(little-endian words: ``dtype`` is the low half of its word, ``group`` the high half)"""
        super().write(key, [r[0].numel() for r in rows], [
            [p.data_ptr(), 0 if g is None else g.data_ptr(), z.data_ptr(), v.data_ptr(), p.numel(), _DT[p.dtype] | (gi << 32)]
            for p, g, z, v, gi in rows])
        self.step_bytes = 7.0 * sum(p.numel() * p.element_size() for p, g, _, _, _ in rows if g is not None)
        self.swap_bytes = 3.0 * sum(p.numel() * p.element_size() for p, _, _, _, _ in rows)

    @staticmethod
    def _records(param_groups) -> torch.Tensor:
        host = torch.zeros(len(param_groups), _GROUP_WORDS, dtype=torch.float64)
        words = host.view(torch.int64)
        for i, g in enumerate(param_groups):
            host[i, :7] = torch.tensor([g["lr"], g["betas"][0], g["betas"][1], g["eps"], g["weight_decay"], g["r"],
                                        g["weight_lr_power"]], dtype=torch.float64)
            words[i, 7], words[i, 8] = int(g["warmup_steps"]), int(g["k"])
            host[i, 9:] = torch.tensor([g["weight_sum"], g["lr_max"], g["scheduled_lr"]], dtype=torch.float64)
        return host

    def write_hypers(self, param_groups, hypers) -> None:
        self.groups[:, :_N_HYPER_WORDS].copy_(self._records(param_groups)[:, :_N_HYPER_WORDS])
        self.hypers = hypers

    def write_state(self, param_groups) -> None:
        self.groups[:, _N_HYPER_WORDS:].copy_(self._records(param_groups)[:, _N_HYPER_WORDS:])

    def read_state(self, param_groups) -> None:
        host = self.groups.cpu()  # the one copy to the host
        words = host.view(torch.int64)
        for i, g in enumerate(param_groups):
            g["k"] = int(words[i, 8])
            g["weight_sum"], g["lr_max"], g["scheduled_lr"] = (float(x) for x in host[i, 9:])


class AdamWScheduleFree(torch.optim.Optimizer):
    """Schedule-free AdamW.  ``train()`` before training steps, ``eval()`` before validation, saving and packaging.

    Args:
        params: parameters or parameter groups; every hyper-parameter below can be set per group
        lr (float): learning rate
        betas (Tuple[float, float]): interpolation / averaging coefficient ``beta1`` in [0, 1) and the second-moment decay
        eps (float): added to the root of the bias-corrected second moment
        weight_decay (float): decoupled weight decay, taken at ``y``
        warmup_steps (int): steps of linear learning-rate warm-up
        r (float): the averaging weight of step ``k`` carries ``(k+1)**r``
        weight_lr_power (float): ... and ``lr_max**weight_lr_power`` (the warm-up steps then weigh less)
    """

    def __init__(self, params, lr: float = 0.0025, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0, warmup_steps: int = 0, r: float = 0.0, weight_lr_power: float = 2.0):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, warmup_steps=warmup_steps, r=r,
                        weight_lr_power=weight_lr_power, k=0, weight_sum=0.0, lr_max=-1.0, scheduled_lr=0.0, train_mode=False)
        self._tables: Optional[_DeviceTables] = None  # while None `param_groups` holds the group state; otherwise the device does
        super().__init__(params, defaults)

    # ---- groups and their state ---------------------------------------------------------------------------------------------
    @staticmethod
    def _hypers_of(group: Dict[str, Any]) -> tuple:
        lr, (b1, b2), eps, wd = float(group["lr"]), group["betas"], float(group["eps"]), float(group["weight_decay"])
        warmup, r, power = int(group["warmup_steps"]), float(group["r"]), float(group["weight_lr_power"])
        if not (lr >= 0.0 and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0 and eps >= 0.0 and wd >= 0.0 and warmup >= 0):
            raise ValueError(f"AdamWScheduleFree: lr, eps, weight_decay, warmup_steps >= 0 and betas in [0, 1) are required, got "
                             f"lr={lr}, betas={(b1, b2)}, eps={eps}, weight_decay={wd}, warmup_steps={warmup}")
        return lr, float(b1), float(b2), eps, wd, warmup, r, power

    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        super().add_param_group(param_group)
        self._hypers_of(self.param_groups[-1])
        if len(self.param_groups) > 1:  # (a new parameter equals its z: both modes are the same point)
            self.param_groups[-1]["train_mode"] = self.param_groups[0]["train_mode"]

    def _sync_from_device(self) -> None:
        if self._tables is not None:
            self._tables.read_state(self.param_groups)

    def _drop_tables(self) -> None:
        self._sync_from_device()
        self._tables = None

    def _capturing(self) -> bool:
        return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()

    def _ensure_state(self, what: str) -> None:
        for group in self.param_groups:
            for p in group["params"]:
                state = self.state[p]
                if "z" not in state:
                    if self._capturing():
                        raise RuntimeError(f"AdamWScheduleFree.{what}: call step() once eagerly before capturing it (the state "
                                           "tensors are built eagerly)")
                    state["z"] = p.detach().clone(memory_format=torch.preserve_format)
                    state["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)

    # ---- which tensors go where ---------------------------------------------------------------------------------------------
    def _rows(self, for_step: bool) -> Tuple[List[_Row], List[_Row], Optional[torch.device]]:
        """The parameters split into table rows of the kernels and rows of the ATen form, and the device of the former.  For a
        step a parameter the kernels take whose ``.grad`` they do not take has a table row without ``.grad`` (skipped) and an
        ATen row; parameters without ``.grad`` have no ATen row."""
        native, rest = [], []
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                z, v = self.state[p]["z"], self.state[p]["exp_avg_sq"]
                g = p.grad if for_step else None
                if g is not None and g.is_sparse:
                    raise RuntimeError("AdamWScheduleFree does not support sparse gradients")
                on_kernel = (p.is_cuda and p.dtype in _DT and p.is_contiguous() and all(
                    t.device == p.device and t.dtype == p.dtype and t.is_contiguous() for t in (z, v)))
                g_on_kernel = g is None or (g.device == p.device and g.dtype == p.dtype and g.is_contiguous())
                if on_kernel:
                    native.append((p, g if g_on_kernel else None, z, v, gi))
                if g is not None and not (on_kernel and g_on_kernel):
                    rest.append((p, g if g.dtype == p.dtype else g.to(p.dtype), z, v, gi))
                elif not for_step and not on_kernel:
                    rest.append((p, None, z, v, gi))
        devices = {r[0].device for r in native}
        if len(devices) > 1:
            raise RuntimeError(f"AdamWScheduleFree: the GPU parameters must be on one device, found {sorted(map(str, devices))}")
        return native, rest, (devices.pop() if devices else None)

    def _device_tables(self, device: torch.device, native: List[_Row], what: str) -> _DeviceTables:
        key = tuple((p.data_ptr(), 0 if g is None else g.data_ptr(), z.data_ptr(), v.data_ptr(), p.numel(), p.dtype, gi)
                    for p, g, z, v, gi in native)
        hypers = tuple(self._hypers_of(g) for g in self.param_groups)
        tables = self._tables
        same = tables is not None and tables.device == device and tables.n_groups == len(self.param_groups) and (
            tables.key == key or (what != "step" and _strip_grads(tables.key) == _strip_grads(key)))
        if same and tables.hypers == hypers:
            return tables
        require_eager(f"AdamWScheduleFree.{what}: call step() once eagerly before capturing it (the device tables are built, and "
                      "rewritten after a parameter, its .grad or a hyper-parameter changed, eagerly; keep the gradient buffers "
                      "with zero_grad(set_to_none=False))")
        with torch.cuda.device(device):
            if not same:
                if tables is None or not tables.fits(device, native, len(self.param_groups)):
                    self._drop_tables()
                    chunk = int(_lib.load().nqa_ema_chunk_elems())
                    tables = _DeviceTables(device, len(native), n_chunks([r[0].numel() for r in native], chunk),
                                           len(self.param_groups), chunk)
                    tables.write_state(self.param_groups)
                tables.write(key, native)
            if tables.hypers != hypers:
                tables.write_hypers(self.param_groups, hypers)
        self._tables = tables
        return tables

    # ---- the step -----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def step(self, closure: Optional[Callable] = None):
        """One schedule-free AdamW step on every parameter that has a ``.grad`` (which is only read)."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not all(g["train_mode"] for g in self.param_groups):
            raise RuntimeError("AdamWScheduleFree.step: the optimizer is not in train mode; call .train() on it before training "
                               "steps (and .eval() before validation and saving)")
        self._ensure_state("step")
        native, rest, device = self._rows(for_step=True)
        if not native:
            self._drop_tables()
        else:
            tables = self._device_tables(device, native, "step")
            if rest:
                if self._capturing():
                    raise RuntimeError("AdamWScheduleFree.step: tensors the kernels do not take (CPU tensors, other dtypes than "
                                       "float32 / float64, non-contiguous ones) cannot be captured: their step scalars are "
                                       "host numbers")
                self._sync_from_device()
        if rest or not native:
            for gi, group in enumerate(self.param_groups):
                s = _step_scalars(group)
                rows = [r for r in rest if r[4] == gi]
                if rows:
                    _aten_step(rows, group, s)
                if not native:
                    group["k"] = int(group["k"]) + 1
                    group["weight_sum"], group["lr_max"], group["scheduled_lr"] = s["weight_sum"], s["lr_max"], s["lr_k"]
        if native:
            with torch.cuda.device(device), ktimer.region("sfree_step", tables.step_bytes):
                rc = _lib.load().nqa_sfree_step(_lib.ptr(tables.tensors), _lib.ptr(tables.chunks), tables.capacity,
                                                _lib.ptr(tables.counts), _lib.ptr(tables.groups), tables.n_groups,
                                                _lib.stream_ptr(device))
            _lib.check(rc, "nqa_sfree_step")
            torch.autograd.graph.increment_version([t for p, g, z, v, _ in native if g is not None for t in (p, z, v)])
        return loss

    # ---- the two modes ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _switch(self, to_eval: bool) -> None:
        what = "eval" if to_eval else "train"
        pending = [g for g in self.param_groups if bool(g["train_mode"]) == to_eval]
        if not pending:
            return
        if len(pending) != len(self.param_groups):
            raise RuntimeError(f"AdamWScheduleFree.{what}: the parameter groups are in different modes")
        if self._capturing():
            raise RuntimeError(f"AdamWScheduleFree.{what} cannot be captured: the mode is host state")
        if to_eval and any(g["betas"][0] == 0.0 for g in self.param_groups):
            raise ValueError("AdamWScheduleFree.eval: with beta1 == 0 the parameters are z and the averaged weights cannot be "
                             "recovered from them")
        self._ensure_state(what)
        native, rest, device = self._rows(for_step=False)
        if native:
            tables = self._device_tables(device, native, what)
            with torch.cuda.device(device), ktimer.region("sfree_swap", tables.swap_bytes):
                rc = _lib.load().nqa_sfree_swap(_lib.ptr(tables.tensors), _lib.ptr(tables.chunks), tables.capacity,
                                                _lib.ptr(tables.counts), _lib.ptr(tables.groups), tables.n_groups, int(to_eval),
                                                _lib.stream_ptr(device))
            _lib.check(rc, "nqa_sfree_swap")
            torch.autograd.graph.increment_version([r[0] for r in native])
        for gi, group in enumerate(self.param_groups):
            rows = [r for r in rest if r[4] == gi]
            if rows:
                torch._foreach_lerp_([r[0] for r in rows], [r[2] for r in rows], _swap_weight(group["betas"][0], to_eval))
        for g in self.param_groups:
            g["train_mode"] = not to_eval

    def train(self) -> None:
        """The parameters hold ``y``, where the gradients are taken.  A no-op in train mode."""
        self._switch(to_eval=False)

    def eval(self) -> None:
        """The parameters hold ``x``, the averaged weights.  A no-op in eval mode."""
        self._switch(to_eval=True)

    @contextlib.contextmanager
    def averaged_parameters(self):
        """``with opt.averaged_parameters():`` the parameters hold the averaged weights inside the block and what they held
        before afterwards, also when the block raises."""
        was_training = all(g["train_mode"] for g in self.param_groups)
        self.eval()
        try:
            yield self
        finally:
            if was_training:
                self.train()

    # ---- state dicts --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, Any]:
        """(copies the group state from the device into ``param_groups`` first: one copy to the host)"""
        self._sync_from_device()
        return super().state_dict()

    @torch.no_grad()
    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        """The loaded ``z`` / ``exp_avg_sq`` are copied INTO the state tensors that exist (a captured step keeps its pointers),
        the group state is pushed to the device records; hyper-parameters reach them at the next eager ``step()``."""
        old = {p: dict(s) for p, s in self.state.items()}
        super().load_state_dict(state_dict)
        for p, state in self.state.items():
            for name in ("z", "exp_avg_sq"):
                prev, new = old.get(p, {}).get(name), state.get(name)
                if prev is not None and new is not None and prev.shape == new.shape and prev.dtype == new.dtype \
                        and prev.device == new.device:
                    prev.copy_(new)
                    state[name] = prev
        if self._tables is not None:
            self._tables.write_state(self.param_groups)


class ScheduleFreeHooks:
    """The hooks of the reference's ``ScheduleFreeLightningModule`` by name, without Lightning: the trainer calls them with the
    optimizer where the reference asks ``self.optimizers()``.

        hooks = ScheduleFreeHooks()
        hooks.on_train_epoch_start(opt) ... hooks.on_validation_epoch_start(opt) ...
        hooks.on_save_checkpoint(checkpoint, opt)            # checkpoint["schedulefree_optimizer_state_dict"]
        hooks.on_load_checkpoint(checkpoint); model = hooks.evaluation_model(model, make_optimizer)
    """

    def __init__(self):
        self._schedulefree_state_dict: Dict[str, Any] = {}  # restored lazily by `evaluation_model`

    def on_train_epoch_start(self, opt: AdamWScheduleFree) -> None:
        opt.train()

    def on_validation_epoch_start(self, opt: AdamWScheduleFree) -> None:
        opt.eval()

    def on_test_epoch_start(self, opt: AdamWScheduleFree) -> None:
        opt.eval()

    def on_predict_epoch_start(self, opt: AdamWScheduleFree) -> None:
        opt.eval()

    def on_save_checkpoint(self, checkpoint: dict, opt: Optional[AdamWScheduleFree]) -> None:
        if opt is not None:
            checkpoint[CHECKPOINT_KEY] = copy.deepcopy(opt.state_dict())

    def on_load_checkpoint(self, checkpoint: dict) -> None:
        state = checkpoint.get(CHECKPOINT_KEY)
        if state is not None:
            self._schedulefree_state_dict = state

    def evaluation_model(self, model: torch.nn.Module, make_optimizer: Callable[[torch.nn.Module], AdamWScheduleFree]):
        """The model with the averaged weights, for packaging: a fresh optimizer from ``make_optimizer(model)`` gets the state
        stored by ``on_load_checkpoint`` and is put into eval mode (the model must hold the weights of the same checkpoint)."""
        opt = make_optimizer(model)
        if self._schedulefree_state_dict:
            opt.load_state_dict(self._schedulefree_state_dict)
        opt.eval()
        return model
