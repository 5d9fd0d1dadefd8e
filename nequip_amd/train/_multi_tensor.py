"""Host side of the multi-tensor chunk layout (``csrc/multi_tensor.h``, "multi-tensor chunk layout" in ``include/nequip_amd.h``)
that ``EMAWeights``, ``ConFIGGradients``, ``AdamWScheduleFree`` and ``TrainingStatsMonitor`` launch over: a device table of
tensor records, a device map of chunks and the counts in use, allocated once and rewritten IN PLACE when the tensors change, so
that a captured launch keeps reading the same buffers."""

from __future__ import annotations

from typing import List, Sequence, Tuple

import torch

from .. import _lib

_DT = {torch.float32: _lib.NQA_F32, torch.float64: _lib.NQA_F64}


def n_chunks(numels: Sequence[int], chunk: int) -> int:
    return sum(-(-n // chunk) for n in numels)


def chunk_map(numels: Sequence[int], chunk: int) -> Tuple[torch.Tensor, List[int]]:
    """The chunk map of tensors of ``numels`` elements, ``chunk`` elements per chunk: the ``[offset, tensor]`` rows (int64, on the
    CPU; little-endian words: the int32 ``tensor`` is the low half of its word, the pad 0) and the index of every tensor's first
    chunk.  A tensor without elements has an entry and no chunk."""
    offsets = [torch.arange(0, n, chunk, dtype=torch.int64) for n in numels]
    rows = torch.cat([torch.stack([o, torch.full_like(o, i)], dim=1) for i, o in enumerate(offsets)]
                     + [torch.zeros(0, 2, dtype=torch.int64)])
    chunk0, total = [], 0
    for o in offsets:
        chunk0.append(total)
        total += len(o)
    return rows, chunk0


def require_eager(message: str) -> None:
    """The device tables are built, and rebuilt, eagerly: ``message`` says what to call once before capturing."""
    if torch.cuda.is_current_stream_capturing():
        raise RuntimeError(message)


class ChunkTables:
    """``tensors [n_tensors, words]`` and ``chunks [capacity, 2]`` (int64) on one device, and ``counts = [chunks in use, tensors in
    use]``.  ``capacity`` is what the kernels take as their grid; ``key`` is whatever the owner keyed the last ``write`` on."""

    def __init__(self, device: torch.device, chunk: int, n_tensors: int, capacity: int, words: int):
        self.device, self.chunk = device, chunk
        self.n_tensors, self.capacity = max(n_tensors, 1), capacity
        self.tensors = torch.zeros(self.n_tensors, words, dtype=torch.int64, device=device)
        self.chunks = torch.zeros(max(capacity, 1), 2, dtype=torch.int64, device=device)
        self.counts = torch.zeros(2, dtype=torch.int64, device=device)
        self.key = None

    def fits(self, device: torch.device, numels: Sequence[int]) -> bool:
        return device == self.device and len(numels) <= self.n_tensors and n_chunks(numels, self.chunk) <= self.capacity

    def write(self, key, numels: Sequence[int], rows: List[List[int]], with_chunk0: bool = False) -> None:
        """``rows``: the words of the record of every tensor; ``with_chunk0`` appends the index of the tensor's first chunk."""
        chunk_rows, chunk0 = chunk_map(numels, self.chunk)
        if with_chunk0:
            rows = [r + [c] for r, c in zip(rows, chunk0)]
        assert len(rows) <= self.n_tensors and len(chunk_rows) <= self.capacity
        if rows:
            self.tensors[:len(rows)].copy_(torch.tensor(rows, dtype=torch.int64))
        if len(chunk_rows):
            self.chunks[:len(chunk_rows)].copy_(chunk_rows)
        self.counts.copy_(torch.tensor([len(chunk_rows), len(rows)], dtype=torch.int64))
        self.key = key
