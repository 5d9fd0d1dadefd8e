"""What the host drivers of the STREAM / TERM / SLOT reductions share (csrc/slot_reduce.h; ``train/_metrics_ops.py::FusedPlan``,
``data/_stats_ops.py::StatsPlan``): the term table ordered by stream with contiguous slots, its cached ctypes form, and per device
the workspace of partial rows and the running state ``[planes, slots]`` -- allocated once --, plus the canonical form of a
stream's tensors and the membership mask of the ATen forms."""

from __future__ import annotations

import math
from typing import Dict, Optional

import torch

from .. import _lib


class SlotPlan:
    """Terms in the caller's order; the table handed to the kernels is ordered by stream.  A subclass gives ``MAX_STREAMS`` /
    ``MAX_TERMS`` with their messages (``TOO_MANY_*``, formatted with ``n`` and ``max``), ``TERM_STRUCT`` and ``fill_row``
    (one row of the ctypes table), ``WORKSPACE_BYTES`` (the name of the library's size function) and ``PLANES``: (name, dtype,
    initial value) of every 8-byte plane of the state.  Its ``check_terms()`` runs before the slots are assigned: it may raise
    and must leave ``n_groups`` on every term; its ``device_buffers(bufs, device)`` adds what else a GPU needs."""

    MAX_SLOTS: Optional[int] = None

    def __init__(self, terms, n_streams: int):
        if n_streams > self.MAX_STREAMS:
            raise ValueError(self.TOO_MANY_STREAMS.format(n=n_streams, max=self.MAX_STREAMS))
        if len(terms) > self.MAX_TERMS:
            raise ValueError(self.TOO_MANY_TERMS.format(n=len(terms), max=self.MAX_TERMS))
        self.terms, self.n_streams = list(terms), n_streams
        self.check_terms()
        self.table_order = sorted(range(len(self.terms)), key=lambda i: self.terms[i].stream)  # (stable)
        slot = 0
        for i in self.table_order:
            self.terms[i].slot0 = slot
            slot += self.terms[i].n_groups
        if self.MAX_SLOTS is not None and slot > self.MAX_SLOTS:
            raise ValueError(self.TOO_MANY_SLOTS.format(n=slot, max=self.MAX_SLOTS))
        self.n_slots = slot
        self._dev: Dict[torch.device, dict] = {}
        self._host_table = None

    def __getstate__(self):  # (device buffers and the ctypes table are rebuilt on demand; a copy starts with an empty state)
        d = dict(self.__dict__)
        d["_dev"], d["_host_table"] = {}, None
        return d

    def host_table(self):
        if self._host_table is None:
            arr = (self.TERM_STRUCT * len(self.terms))()
            for row, i in enumerate(self.table_order):
                self.fill_row(arr[row], self.terms[i])
            self._host_table = arr
        return self._host_table

    def buffers(self, device: torch.device) -> dict:
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        bufs = self._dev.get(device)
        if bufs is None:
            S = self.n_slots
            state = torch.zeros(len(self.PLANES) * S, dtype=torch.int64, device=device)  # [planes, S], 8 bytes each
            bufs = {"state": state}
            for j, (name, dtype, init) in enumerate(self.PLANES):
                bufs[name] = state[j * S:(j + 1) * S].view(dtype)
                bufs[name].fill_(init)
            if device.type == "cuda":
                nbytes = int(getattr(_lib.load(), self.WORKSPACE_BYTES)(S))
                bufs["workspace"] = torch.empty(nbytes // 8, dtype=torch.float64, device=device)
                bufs["workspace_bytes"] = nbytes
                self.device_buffers(bufs, device)
            self._dev[device] = bufs
        return bufs

    def reset(self) -> None:
        for bufs in self._dev.values():
            for name, _, init in self.PLANES:
                bufs[name].fill_(init)


def canonical_rows(x: torch.Tensor, keep=(torch.float32, torch.float64), integers=torch.float64) -> torch.Tensor:
    """``[rows, cols]`` contiguous (a scalar is one row, the trailing dimensions one row's columns, no row still has a column)
    in a dtype of ``keep``: float16 / bfloat16 become float32, other floating types float64, anything else ``integers``."""
    if x.dtype not in keep:
        half = x.dtype in (torch.float16, torch.bfloat16)
        x = x.to(torch.float32 if half else (torch.float64 if x.is_floating_point() else integers))
    rows = x.shape[0] if x.dim() > 0 else 1
    cols = math.prod(x.shape[1:])
    return x.reshape(rows, cols if rows > 0 else max(1, cols)).contiguous()


def canonical_row_scale(scale: Optional[torch.Tensor], rows: int, device) -> Optional[torch.Tensor]:
    if scale is not None:
        scale = scale.detach().to(device=device, dtype=torch.float64).reshape(-1).contiguous()
        assert scale.numel() == rows, "one scale per row"
    return scale


def membership(group: Optional[torch.Tensor], n_groups: int, contrib: torch.Tensor) -> torch.Tensor:
    """``[n_groups, rows, cols]``: element (r, c) contributes (``contrib``) and row r is of group g; ``group`` None: one group."""
    if group is None:
        return contrib[None]
    return (group[None, :] == torch.arange(n_groups, device=group.device)[:, None])[:, :, None] & contrib[None]
