"""``TrainingStatsMonitor``: per-parameter statistics of the weights, the gradients and the Adam moments every ``log_freq`` steps
(the reference's ``nequip/train/callbacks/training_stats.py::TrainingStatsMonitor`` without the Lightning dependency: the same
logging rule, the same keys, ``compute()`` in place of ``pl_module.log_dict``).

    mon = TrainingStatsMonitor(log_freq=100)
    loss.backward();                             mon.on_after_backward(model)
    mon.on_before_optimizer_step(model, [opt]);  opt.step()
    stats = mon.compute()                        # Dict[str, float] of the last logged step

A step logs when ``step_count % log_freq == 0`` (step 0 logs); ``on_after_backward`` writes the gradient rows,
``on_before_optimizer_step`` the weight and the optimizer rows, and only the latter advances the count, on every call.

On the GPU a hook is the multi-tensor reduction ``nqa_tstats_reduce`` (csrc/training_stats.hip): every tensor is read once and
one row ``[min, max, mean, std, absmin, absmax, rms, count]`` per tensor is left in a float64 table on the device; nothing is
read by the host before ``compute()``, which copies the tables once.  The step count lives on the device and the kernels test
``count % log_freq`` themselves, so hooks captured into a hipGraph keep logging every ``log_freq`` replays.  The kernels take
CUDA tensors of float32 / float64 that are dense (contiguous in some memory format: the statistics do not depend on the element
order beyond rounding).  Everything else -- CPU tensors, other dtypes, strided views -- takes ``_aten_row``: the reference's
lines as ATen calls, stacked into the same row layout without ``.item()``; the count is then kept on the host, and a mixture
of both kinds works eagerly and is refused under capture.  A missing library raises (``_lib.load``).

Deliberate differences from the reference:

* on the GPU the arithmetic is float64 whatever the tensor dtype (the reference reduces in the tensor's dtype), ``sqrt`` of
  ``exp_avg_sq`` included;
* with +-inf and no NaN in a tensor, ``min``, ``max``, ``absmin``, ``absmax`` and ``rms`` are ATen's, ``mean`` and ``std`` are
  only non-finite: Welford forms ``inf - inf = NaN`` where ATen's sum may give ``inf``.  One NaN makes all statistics NaN, as
  in ATen;
* tensors without elements get no rows (the reference raises on them);
* the count lives on the device, so a captured step keeps logging every ``log_freq`` replays.

The device tables are keyed on the data pointers of what they describe, allocated once for the most the model can need and
rewritten in place when a key changed (``.grad`` reallocated by ``zero_grad(set_to_none=True)``, optimizer state appearing,
``.to()``); when the LIST of tensors changed, the rows move with their tensors and a tensor that is new to the list has no keys
until the next logged step.
"""

from __future__ import annotations

import math
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from .. import _lib
from ..utils import ktimer
from ._multi_tensor import _DT, ChunkTables, n_chunks, require_eager

_PREFIX = "training_stats"
COLUMNS = {"min": 0, "max": 1, "mean": 2, "std": 3, "absmin": 4, "absmax": 5, "rms": 6, "count": 7}
_IDENTITY, _SQRT = 0, 1  # nqa_tstats_transform
_WEIGHT_STATS = ("min", "max", "mean", "std", "absmin", "absmax")
_GRADIENT_STATS = ("absmax", "rms")
_EXP_AVG_STATS = ("absmax", "rms")
_SQRT_EXP_AVG_SQ_STATS = ("min", "max", "mean")


class _Entry(NamedTuple):
    """One tensor, one table row: the keys are ``training_stats.{head}.{stat}/{name}``."""
    head: str
    name: str
    stats: Tuple[str, ...]
    tensor: torch.Tensor
    transform: int

    def keys(self) -> List[Tuple[str, int]]:
        return [(f"{_PREFIX}.{self.head}.{s}/{self.name}", COLUMNS[s]) for s in self.stats]


def _is_dense(t: torch.Tensor) -> bool:
    return t.is_contiguous() or torch._prims_common.is_non_overlapping_and_dense(t)


def _on_kernel(t: torch.Tensor) -> bool:
    return t.is_cuda and t.dtype in _DT and _is_dense(t)


def _aten_row(t: torch.Tensor, stats: Sequence[str], transform: int) -> torch.Tensor:
    """The reference's lines for one tensor, in the tensor's dtype, as a float64 row (the columns not asked for are NaN)."""
    x = t.detach()
    if transform == _SQRT:
        x = torch.sqrt(x)
    nan = torch.full((), math.nan, dtype=torch.float64, device=x.device)
    row = [nan] * 7 + [torch.full((), float(x.numel()), dtype=torch.float64, device=x.device)]
    ax = x.abs() if ("absmin" in stats or "absmax" in stats) else None
    for s in stats:
        if s == "min":
            v = x.min()
        elif s == "max":
            v = x.max()
        elif s == "mean":
            v = x.mean()
        elif s == "std":
            v = x.std() if x.numel() > 1 else nan  # (torch.std of one element: NaN, with a warning)
        elif s == "absmin":
            v = ax.min()
        elif s == "absmax":
            v = ax.max()
        else:
            v = torch.sqrt(torch.mean(x ** 2))
        row[COLUMNS[s]] = v.to(torch.float64)
    return torch.stack(row)


class _DeviceTables(ChunkTables):
    """What the kernels read and write for one hook on one device: the chunk tables of the tensors (``nqa_tstats_tensor``: 4 words
    each), the workspace of chunk rows and ``out``: one row per tensor and a last row whose first word is the step (int64) at
    which the rows were written."""

    def __init__(self, device: torch.device, n_tensors: int, capacity: int, chunk: int):
        super().__init__(device, chunk, n_tensors, max(capacity, 1), words=4)
        self.workspace = torch.zeros(self.capacity, 8, dtype=torch.float64, device=device)
        self.out = torch.zeros(self.n_tensors + 1, 8, dtype=torch.float64, device=device)
        self.stamp = self.out[self.n_tensors].view(torch.int64)[:1]
        self.stamp.fill_(-1)
        self.names: Optional[tuple] = None
        self.nbytes = 0

    def write(self, key, entries: List[_Entry]) -> None:
        """(little-endian words: ``dtype`` and ``chunk0`` are the low halves of their words, ``transform`` a high half)"""
        tensors = [e.tensor for e in entries]
        super().write(key, [t.numel() for t in tensors], with_chunk0=True, rows=[
            [t.data_ptr(), t.numel(), _DT[t.dtype] | (e.transform << 32)] for t, e in zip(tensors, entries)])
        names = tuple((e.head, e.name) for e in entries)
        if names != self.names:  # the rows move with their tensors; those of new tensors hold nothing (count 0) until a step logs
            old = {name: i for i, name in enumerate(self.names or ())}
            kept = [(i, old[name]) for i, name in enumerate(names) if name in old]
            moved = torch.zeros_like(self.out[:self.n_tensors])
            if kept:
                moved[[i for i, _ in kept]] = self.out[[j for _, j in kept]]
            self.out[:self.n_tensors].copy_(moved)
        self.names = names
        self.nbytes = sum(t.numel() * t.element_size() for t in tensors)


class _Section:
    """The rows of one hook: ``layout`` says where the row of an entry of the last written list lies (device table or ATen)."""

    def __init__(self, what: str):
        self.what = what
        self.tables: Optional[_DeviceTables] = None
        self.layout: List[Tuple[_Entry, str, int]] = []  # (entry without its tensor, "hip" | "aten", row)
        self.aten_rows: List[torch.Tensor] = []


class TrainingStatsMonitor:
    """Monitor detailed training statistics: weights, gradients and the internal states of Adam / AdamW optimizers.

    Args:
        log_freq (int): frequency (in optimizer steps) at which statistics are written
        log_weights (bool): whether to log weight statistics
        log_gradients (bool): whether to log gradient statistics
        log_optimizer_states (bool): whether to log ``exp_avg`` / ``exp_avg_sq`` statistics (Adam / AdamW only)
        name_prefix (str): prepended to every parameter name of ``model.named_parameters()``
    """

    def __init__(self, log_freq: int = 100, log_weights: bool = True, log_gradients: bool = True,
                 log_optimizer_states: bool = True, name_prefix: str = ""):
        assert int(log_freq) >= 1, f"log_freq must be >= 1, got {log_freq}"
        self.log_freq = int(log_freq)
        self.log_weights = log_weights
        self.log_gradients = log_gradients
        self.log_optimizer_states = log_optimizer_states
        self.name_prefix = name_prefix
        self._step_count = 0  # the truth while `_counter` is None; otherwise `_counter` on the device is
        self._counter: Optional[torch.Tensor] = None
        self._host_logged_step = -1  # of the ATen form
        self._gradients = _Section("on_after_backward")
        self._step = _Section("on_before_optimizer_step")

    # ---- the count ---------------------------------------------------------------------------------------------------------
    @property
    def step_count(self) -> int:
        """Number of ``on_before_optimizer_step`` calls.  After a GPU hook this copies the device counter to the host."""
        if self._counter is not None:
            return int(self._counter.item())
        return self._step_count

    @property
    def logged_step(self) -> Optional[int]:
        """The last step whose statistics were written; ``None`` before the first one."""
        stamps = [s.tables.stamp for s in (self._gradients, self._step) if s.tables is not None]
        last = self._host_logged_step
        if stamps:
            last = max([last] + torch.cat([s.to(stamps[0].device) for s in stamps]).tolist())
        return None if last < 0 else int(last)

    def _device_counter(self, device: torch.device, what: str) -> torch.Tensor:
        if self._counter is None or self._counter.device != device:
            require_eager(f"TrainingStatsMonitor.{what}: run the hooks once eagerly before capturing them (the device tables and "
                          "the step counter are built eagerly)")
            self._counter = torch.tensor([self.step_count], dtype=torch.int64, device=device)
        return self._counter

    # ---- which tensors ---------------------------------------------------------------------------------------------------------
    def _gradient_entries(self, model: torch.nn.Module) -> List[_Entry]:
        out = []
        for name, p in model.named_parameters():
            if p.requires_grad and p.grad is not None and p.grad.numel() > 0:
                out.append(_Entry("gradients", self.name_prefix + name, _GRADIENT_STATS, p.grad.detach(), _IDENTITY))
        return out

    def _weight_entries(self, model: torch.nn.Module) -> List[_Entry]:
        out = []
        for name, p in model.named_parameters():
            if p.requires_grad and p.numel() > 0:
                out.append(_Entry("weights", self.name_prefix + name, _WEIGHT_STATS, p.detach(), _IDENTITY))
        return out

    def _optimizer_entries(self, model: torch.nn.Module, optimizers) -> List[_Entry]:
        names = {id(p): self.name_prefix + name for name, p in model.named_parameters()}
        out = []
        for i, opt in enumerate(optimizers):
            suffix = f"_{i}" if len(optimizers) > 1 else ""
            for p, state in opt.state.items():
                if id(p) not in names or "exp_avg" not in state or "exp_avg_sq" not in state:
                    continue
                m, v = state["exp_avg"], state["exp_avg_sq"]
                if isinstance(m, torch.Tensor) and m.numel() > 0:
                    out.append(_Entry(f"optimizer{suffix}.exp_avg", names[id(p)], _EXP_AVG_STATS, m.detach(), _IDENTITY))
                if isinstance(v, torch.Tensor) and v.numel() > 0:
                    out.append(_Entry(f"optimizer{suffix}.sqrt_exp_avg_sq", names[id(p)], _SQRT_EXP_AVG_SQ_STATS, v.detach(),
                                      _SQRT))
        return out

    def _most(self, section: _Section, model: torch.nn.Module, optimizers, chunk: int) -> Tuple[int, int]:
        """(tensors, chunks): the most a hook can need for this model and these optimizers."""
        def size(ps):
            ps = [p for p in ps if p.numel() > 0]
            return len(ps), n_chunks([p.numel() for p in ps], chunk)

        trainable = size(p for p in model.parameters() if p.requires_grad)
        if section is self._gradients:
            return trainable
        known = {id(p) for p in model.parameters()}
        n, c = trainable if self.log_weights else (0, 0)
        if self.log_optimizer_states:
            for opt in optimizers:
                k, m = size(p for g in opt.param_groups for p in g["params"] if id(p) in known)
                n, c = n + 2 * k, c + 2 * m
        return n, c

    # ---- one hook ----------------------------------------------------------------------------------------------------------
    def _device_tables(self, section: _Section, device: torch.device, native: List[_Entry], model, optimizers) -> _DeviceTables:
        key = tuple((e.head, e.name, e.tensor.data_ptr(), e.tensor.numel(), e.tensor.dtype, e.transform) for e in native)
        tables = section.tables
        if tables is not None and tables.key == key and tables.device == device:
            return tables
        require_eager(f"TrainingStatsMonitor.{section.what}: run the hooks once eagerly before capturing them (the device tables "
                      "are built, and rebuilt after a tensor moved or appeared, eagerly)")
        with torch.cuda.device(device):
            numels = [e.tensor.numel() for e in native]
            if tables is None or not tables.fits(device, numels):
                chunk = int(_lib.load().nqa_tstats_chunk_elems())
                n, c = self._most(section, model, optimizers, chunk)
                tables = _DeviceTables(device, max(n, len(native)), max(c, n_chunks(numels, chunk)), chunk)
            tables.write(key, native)
        section.tables = tables
        return tables

    @torch.no_grad()
    def _write(self, section: _Section, entries: List[_Entry], model, optimizers) -> None:
        native = [e for e in entries if _on_kernel(e.tensor)]
        rest = [e for e in entries if not _on_kernel(e.tensor)]
        devices = {e.tensor.device for e in native}
        if len(devices) > 1:
            raise RuntimeError(f"TrainingStatsMonitor: the GPU tensors of one hook must be on one device, found "
                               f"{sorted(map(str, devices))}")
        if rest or not native:  # the ATen form decides on the host
            if rest and any(e.tensor.is_cuda for e in rest) and torch.cuda.is_current_stream_capturing():
                raise RuntimeError(f"TrainingStatsMonitor.{section.what}: tensors the kernels do not take (other dtypes than "
                                   "float32 / float64, strided views) cannot be captured: the step count is then host state")
            count = self.step_count
            if count % self.log_freq != 0:
                return
            self._host_logged_step = count
        if native:
            device = devices.pop()
            counter = self._device_counter(device, section.what)
            tables = self._device_tables(section, device, native, model, optimizers)
            with torch.cuda.device(device), ktimer.region(f"training_stats_{section.what}", float(tables.nbytes)):
                rc = _lib.load().nqa_tstats_reduce(_lib.ptr(tables.tensors), tables.n_tensors, _lib.ptr(tables.chunks),
                                                   tables.capacity, _lib.ptr(tables.counts), _lib.ptr(counter), self.log_freq,
                                                   _lib.ptr(tables.workspace), _lib.ptr(tables.out), _lib.ptr(tables.stamp),
                                                   _lib.stream_ptr(device))
            _lib.check(rc, "nqa_tstats_reduce")
        if not rest and section.layout and all(kind == "hip" for _, kind, _ in section.layout) \
                and tuple((e.head, e.name) for e, _, _ in section.layout) == tuple((e.head, e.name) for e in native):
            return  # the same list as before: a non-logging step leaves the layout, like the rows, alone
        rows = {id(e): ("hip", i) for i, e in enumerate(native)}
        section.aten_rows = [_aten_row(e.tensor, e.stats, e.transform) for e in rest]
        rows.update({id(e): ("aten", i) for i, e in enumerate(rest)})
        section.layout = [(e._replace(tensor=None), *rows[id(e)]) for e in entries]

    def on_after_backward(self, model: torch.nn.Module) -> None:
        """After ``loss.backward()``: the gradient rows of a logging step."""
        if not self.log_gradients:
            return
        entries = self._gradient_entries(model)
        if entries:
            self._write(self._gradients, entries, model, ())

    def on_before_optimizer_step(self, model: torch.nn.Module, optimizers=()) -> None:
        """Before ``opt.step()``: the weight and the optimizer rows of a logging step; then the count advances."""
        if isinstance(optimizers, torch.optim.Optimizer):
            optimizers = [optimizers]
        optimizers = list(optimizers or ())
        entries = self._weight_entries(model) if self.log_weights else []
        if self.log_optimizer_states:
            entries += self._optimizer_entries(model, optimizers)
        if entries:
            self._write(self._step, entries, model, optimizers)
        if self._counter is not None:
            device = self._counter.device
            with torch.cuda.device(device):
                rc = _lib.load().nqa_tstats_advance(_lib.ptr(self._counter), _lib.stream_ptr(device))
            _lib.check(rc, "nqa_tstats_advance")
        else:
            self._step_count += 1

    # ---- reading -----------------------------------------------------------------------------------------------------------
    def compute(self, group=None) -> Dict[str, float]:
        """The statistics of the last logged step (``{}`` before the first one), gradients, weights, optimizer states in the
        reference's key order.  The device tables come to the host in one copy.  Under ``torch.distributed`` every value is
        averaged over the ranks of ``group`` in one all-reduce (what ``log_dict(..., sync_dist=True)`` does)."""
        sections = (self._gradients, self._step)
        used = [s.tables.out[:s.tables.n_tensors] for s in sections if s.tables is not None]
        host = torch.cat([u.to(used[0].device) for u in used]).tolist() if used else None
        out: Dict[str, float] = {}
        offset = 0
        for s in sections:
            aten = torch.stack([r.to("cpu") for r in s.aten_rows]).tolist() if s.aten_rows else None
            for e, kind, i in s.layout:
                row = host[offset + i] if kind == "hip" else aten[i]
                if row[COLUMNS["count"]] == 0:  # a tensor that appeared after the last logged step
                    continue
                for key, col in e.keys():
                    out[key] = row[col]
            if s.tables is not None:
                offset += s.tables.n_tensors
        import torch.distributed as dist

        if out and dist.is_available() and dist.is_initialized() and dist.get_world_size(group) > 1:
            device = used[0].device if used and dist.get_backend(group) != "gloo" else torch.device("cpu")
            flat = torch.tensor(list(out.values()), dtype=torch.float64, device=device)
            dist.all_reduce(flat, op=dist.ReduceOp.SUM, group=group)
            flat /= dist.get_world_size(group)
            out = dict(zip(out.keys(), flat.tolist()))
        return out
