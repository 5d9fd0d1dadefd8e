"""``EMAWeights``: the exponential moving average of a model's parameters (the reference's ``nequip/train/ema.py::EMAWeights``:
same constructor, buffers ``ema_weight_{idx}``, extra state and methods, so state dicts load in both directions).

On the GPU the update and the swap are the multi-tensor HIP kernels ``nqa_ema_update`` / ``nqa_ema_swap`` (csrc/ema.hip), for
two reasons that belong to this code base:

* the decay of a step, ``min(decay, (1 + n) / (10 + n))``, depends on the number of updates ``n``.  As a Python scalar it is
  frozen when the training step is captured into a hipGraph; the kernel reads ``n`` from a device counter, so every replay
  advances the warm-up.  ``num_updates`` stays readable as a Python int: reading it (or ``get_extra_state``) copies the
  counter to the host once, nothing else does;
* the modules cache derived weight images keyed on ``(data_ptr, _version)``.  The kernels write through raw pointers, so the
  version counters of everything they wrote are bumped here (``torch.autograd.graph.increment_version``).

CPU tensors, and GPU tensors the kernels do not take (other dtypes than float32 / float64, non-contiguous ones), go through
``_aten_update`` / ``_aten_swap``: the reference's arithmetic as ATen calls.  A missing library raises (``_lib.load``).
"""

from __future__ import annotations

import contextlib
import warnings
from typing import Dict, List, Optional, Tuple

import torch

from .. import _lib
from ..utils import ktimer
from ._multi_tensor import _DT, ChunkTables, n_chunks, require_eager


def _decay_at(decay: float, n: int) -> float:
    """The decay of update ``n`` (``n`` updates done before it): small early on, so that the first weights fade quickly."""
    return min(decay, (1 + n) / (10 + n))


def _aten_update(emas: List[torch.Tensor], params: List[torch.Tensor], n: int, decay: float) -> None:
    if n == 0:
        for e, p in zip(emas, params):
            e.copy_(p)
        return
    d = _decay_at(decay, n)
    by_dtype: Dict[torch.dtype, Tuple[List[torch.Tensor], List[torch.Tensor]]] = {}
    for e, p in zip(emas, params):
        if (e.is_floating_point() or e.is_complex()) and e.dtype == p.dtype:
            es, ps = by_dtype.setdefault(e.dtype, ([], []))
            es.append(e)
            ps.append(p)
        else:  # (_foreach_lerp_ takes floating and complex tensors only)
            e.copy_(e * d + p * (1 - d))
    for es, ps in by_dtype.values():
        torch._foreach_lerp_(es, ps, 1 - d)


def _aten_swap(emas: List[torch.Tensor], params: List[torch.Tensor]) -> None:
    for e, p in zip(emas, params):
        tmp = e.clone()
        e.copy_(p)
        p.copy_(tmp)


class _DeviceTables(ChunkTables):
    """The chunk tables of the EMA buffers (``nqa_ema_tensor``: 4 words each) and ``state = [num_updates]``.  Allocated once for
    the most the EMA buffers can need."""

    def __init__(self, device: torch.device, emas: List[torch.Tensor], num_updates: int):
        chunk = int(_lib.load().nqa_ema_chunk_elems())
        super().__init__(device, chunk, len(emas), n_chunks([e.numel() for e in emas], chunk), words=4)
        self.state = torch.tensor([num_updates], dtype=torch.int64, device=device)
        self.nbytes = 0

    def write(self, key, pairs: List[Tuple[torch.Tensor, torch.Tensor]]) -> None:
        """(little-endian words: the int32 ``dtype`` is the low half of its word, the pad 0)"""
        super().write(key, [e.numel() for e, _ in pairs], [[e.data_ptr(), p.data_ptr(), e.numel(), _DT[e.dtype]] for e, p in pairs])
        self.nbytes = sum(e.numel() * e.element_size() for e, _ in pairs)


class EMAWeights(torch.nn.Module):
    """Exponential moving average (EMA) of the parameters of a base model.

    The averages are buffers ``ema_weight_{idx}`` in ``model.parameters()`` order; buffers of the model are not tracked.  All
    parameters and EMA buffers must be on one device.

    Args:
        model (torch.nn.Module): base model (this module makes copies of its weights)
        decay (float): the EMA decay factor
    """

    def __init__(self, model: torch.nn.Module, decay: float):
        super().__init__()
        if decay < 0.0 or decay > 1.0:
            raise ValueError(f"Invalid decay value {decay} provided. Please provide a value in [0,1] range.")
        self.decay = decay
        count = 0
        for idx, p in enumerate(model.parameters()):
            self.register_buffer(f"ema_weight_{idx}", torch.empty_like(p))
            count = idx + 1
        self.num_ema_weights = count
        self._num_updates = 0  # the truth while `_tables` is None; otherwise `_tables.state[0]` on the device is
        self._tables: Optional[_DeviceTables] = None
        # False between `swap_parameters` and the swap back: the buffers then hold the raw weights
        self.is_holding_ema_weights = True

    @property
    def ema_weights(self) -> List[torch.Tensor]:
        return [getattr(self, f"ema_weight_{idx}") for idx in range(self.num_ema_weights)]

    @property
    def num_updates(self) -> int:
        """Number of updates done.  After a GPU update this copies the device counter to the host (a synchronisation)."""
        if self._tables is not None:
            return int(self._tables.state[0].item())
        return self._num_updates

    @num_updates.setter
    def num_updates(self, value: int) -> None:
        self._num_updates = int(value)
        if self._tables is not None:
            self._tables.state[:1].copy_(torch.tensor([int(value)], dtype=torch.int64))

    def forward(self, *args, **kwargs):
        raise RuntimeError("This module only carries EMA weights, but not a model forward implementation.")

    def _apply(self, fn, *args, **kwargs):
        # `.to()` / `.cuda()` / `.cpu()`: the device tables stay behind (they are rebuilt at the next GPU call), the count comes along
        self._num_updates = self.num_updates
        self._tables = None
        return super()._apply(fn, *args, **kwargs)

    # ---- which tensors go where -------------------------------------------------------------------------------------------
    def _pairs(self, model: torch.nn.Module):
        """(EMA buffer, detached parameter) pairs split into those the kernels take and the rest, and the device."""
        emas, params = self.ema_weights, [p.detach() for p in model.parameters()]
        if len(params) != len(emas):
            raise ValueError(f"the model has {len(params)} parameters, this EMAWeights was built for {len(emas)}")
        devices = {t.device for t in emas} | {t.device for t in params}
        if len(devices) > 1:
            raise RuntimeError(f"EMAWeights: all parameters and EMA buffers must be on one device, found {sorted(map(str, devices))}")
        native, rest = [], []
        for e, p in zip(emas, params):
            if e.shape != p.shape:
                raise ValueError(f"EMA buffer of shape {tuple(e.shape)} against a parameter of shape {tuple(p.shape)}")
            on_kernel = e.is_cuda and e.dtype in _DT and p.dtype == e.dtype and e.is_contiguous() and p.is_contiguous()
            (native if on_kernel else rest).append((e, p))
        return native, rest, (devices.pop() if devices else None)

    def _device_tables(self, device: torch.device, native, what: str) -> _DeviceTables:
        key = tuple((e.data_ptr(), p.data_ptr(), e.numel(), e.dtype) for e, p in native)
        tables = self._tables
        if tables is not None and tables.key == key and tables.device == device:
            return tables
        require_eager(f"EMAWeights.{what}: call update_parameters once eagerly before capturing it (the device tables of the "
                      "parameters are built, and rebuilt after the parameters moved, eagerly)")
        with torch.cuda.device(device):
            if tables is None or not tables.fits(device, [e.numel() for e in self.ema_weights]):
                tables = _DeviceTables(device, self.ema_weights, self.num_updates)
            tables.write(key, native)
        self._tables = tables
        return tables

    # ---- the reference's methods -------------------------------------------------------------------------------------------
    @torch.no_grad()
    def update_parameters(self, model: torch.nn.Module) -> None:
        """One EMA step towards the parameters of ``model``; the first one copies them."""
        assert self.is_holding_ema_weights, (
            "EMA module is not holding EMA weights. If using `nequip-train` from a checkpoint, the checkpoint is likely "
            "corrupted. Otherwise, there is something wrong and a GitHub issue should be reported.")
        native, rest, device = self._pairs(model)
        if not native:
            n = self.num_updates
            _aten_update([e for e, _ in rest], [p for _, p in rest], n, self.decay)
            self.num_updates = n + 1
            return
        tables = self._device_tables(device, native, "update_parameters")
        if rest:  # (needs the count on the host: such a mixture is not capturable)
            _aten_update([e for e, _ in rest], [p for _, p in rest], self.num_updates, self.decay)
        with torch.cuda.device(device), ktimer.region("ema_update", 3.0 * tables.nbytes):
            rc = _lib.load().nqa_ema_update(_lib.ptr(tables.tensors), _lib.ptr(tables.chunks), tables.capacity,
                                            _lib.ptr(tables.counts), float(self.decay), _lib.ptr(tables.state),
                                            _lib.stream_ptr(device))
        _lib.check(rc, "nqa_ema_update")
        torch.autograd.graph.increment_version([e for e, _ in native])

    @torch.no_grad()
    def swap_parameters(self, model: torch.nn.Module) -> None:
        """Exchange the EMA buffers with the parameters of ``model`` (before and after validation: the model, with whatever
        its modules have prepared, then evaluates with the averaged weights)."""
        native, rest, device = self._pairs(model)
        if device is not None and device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("EMAWeights.swap_parameters cannot be captured: which side holds the EMA weights is host state")
        if native:
            tables = self._device_tables(device, native, "swap_parameters")
            with torch.cuda.device(device), ktimer.region("ema_swap", 4.0 * tables.nbytes):
                rc = _lib.load().nqa_ema_swap(_lib.ptr(tables.tensors), _lib.ptr(tables.chunks), tables.capacity,
                                              _lib.ptr(tables.counts), _lib.stream_ptr(device))
            _lib.check(rc, "nqa_ema_swap")
            torch.autograd.graph.increment_version([t for pair in native for t in pair])
        _aten_swap([e for e, _ in rest], [p for _, p in rest])
        self.is_holding_ema_weights = not self.is_holding_ema_weights

    @contextlib.contextmanager
    def average_parameters(self, model: torch.nn.Module):
        """``with ema.average_parameters(model):`` the model carries the averaged weights inside the block and its own again
        afterwards, also when the block raises (what the reference does between validation start and end)."""
        if not self.is_holding_ema_weights:
            raise RuntimeError("EMAWeights.average_parameters: the model already carries the averaged weights")
        self.swap_parameters(model)
        try:
            yield model
        finally:
            self.swap_parameters(model)

    def set_extra_state(self, state) -> None:
        self.num_updates = state["num_updates"]
        self.is_holding_ema_weights = state["is_holding_ema_weights"]
        assert self.is_holding_ema_weights, (
            "EMA module loaded in a state where it does not contain EMA weights -- the checkpoint file is likely corrupted.")
        loaded = state["decay"]
        if self.decay != loaded:
            warnings.warn(
                f"EMA decay parameter loaded from state dict ({loaded}) is different from EMA decay parameter set "
                f"({self.decay}) -- make sure this is intended (e.g. you have intentionally overriden `ema_decay` in a "
                f"restart). The current decay value ({self.decay}) will be used.")

    def get_extra_state(self):
        return {"decay": self.decay, "num_updates": self.num_updates, "is_holding_ema_weights": self.is_holding_ema_weights}
