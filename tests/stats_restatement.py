"""A plain-torch float64 restatement of the reference's dataset statistics (nequip/data/stats_manager.py, nequip/data/stats.py,
nequip/data/modifier.py::PerAtomModifier / NumNeighbors / EdgeLengths), the yardstick of ``tests/test_data_statistics*.py``.

The reference itself cannot be imported here (it needs ``torchmetrics``).  This file restates its semantics the slow, obvious
way: one running object per entry and per type (pair), fed with tensors selected by boolean indexing, NaNs removed by another
boolean selection, and the reference's update formulas --

* means (``mean``, ``mean_abs``, ``rms``): ``new_mean = mean + (batch_mean - mean) * batch_count / new_count``, kept as
  ``sum = new_mean * new_count``; value ``sum / count``;
* ``std`` / ``var``: batch mean, batch ``M2`` about it, ``delta = batch_mean - mean``, ``mean += delta * batch_count /
  new_count``, ``M2 += batch_M2 + delta * (delta * batch_count / new_count) * count``; value ``M2 / (count - 1)`` (unbiased);
* ``max`` / ``min``: ``torch.maximum`` / ``torch.minimum`` with the batch's ``max()`` / ``min()`` (NaN propagates);
* ``count``: ``numel``;
* an empty selection updates nothing.

It carries this project's two deliberate deviations from the reference: ``num_neighbors`` gives atom ``i`` its own count (the
reference misaligns the counts when an atom in the middle of the index range is isolated), and a per-type edge entry names the
pair (centre c, neighbour n) that it accumulated at ``c * T + n`` (the reference reads ``c + T * n`` back).  Every value is
promoted to float64 before anything else (``PerAtomModifier`` divides in float64).

Entries: ``{"name", "field", "kind", "per_type", "ignore_nan"}`` with ``field`` a key of the batch or one of
``"per_atom:<key>"``, ``"num_neighbors"``, ``"edge_lengths"`` and ``kind`` one of ``mean, mean_abs, rms, std, var, std_biased, max, absmax, min,
absmin, count``.
"""
import math

import torch

F64 = torch.float64
NODE_FIELDS = {"forces"}  # per-atom fields (a test that uses another one adds it)


class _RunningMean:
    def __init__(self, modifier):
        self.modifier, self.sum, self.count = modifier, torch.tensor(0.0, dtype=F64), 0

    def update(self, x):
        if x.numel() == 0:
            return
        current = self.sum / self.count if self.count != 0 else 0.0
        batch_mean = self.modifier(x).mean().cpu()  # (the running arithmetic is done on 0-dim host tensors)
        new_count = self.count + x.numel()
        new_mean = current + (batch_mean - current) * x.numel() / new_count
        self.count, self.sum = new_count, new_mean * new_count

    def compute(self):
        return self.sum / self.count if self.count != 0 else torch.tensor(math.nan, dtype=F64)  # (0 / 0)


class _RootMeanSquare(_RunningMean):
    def compute(self):
        return super().compute().sqrt()


class _Std:
    def __init__(self, squared, unbiased):
        self.squared, self.unbiased = squared, unbiased
        self.m2, self.mean, self.count = torch.tensor(0.0, dtype=F64), torch.tensor(0.0, dtype=F64), 0

    def update(self, x):
        if x.numel() == 0:
            return
        batch_mean = x.mean()
        batch_m2 = (x - batch_mean).square().sum().cpu()
        batch_mean = batch_mean.cpu()
        delta = batch_mean - self.mean
        new_count = self.count + x.numel()
        change = delta * x.numel() / new_count
        self.mean = self.mean + change
        self.m2 = self.m2 + batch_m2 + delta * change * self.count
        self.count = new_count

    def compute(self):
        denom = torch.tensor(float(self.count - 1 if self.unbiased else self.count), dtype=F64)
        var = self.m2 / denom
        return var if self.squared else var.sqrt()


class _Extreme:
    def __init__(self, largest, absolute):
        self.largest, self.absolute = largest, absolute
        self.value = torch.tensor(-math.inf if largest else math.inf, dtype=F64)

    def update(self, x):
        if x.numel() == 0:
            return
        x = x.abs() if self.absolute else x
        self.value = (torch.maximum(self.value, x.max().cpu()) if self.largest
                      else torch.minimum(self.value, x.min().cpu()))

    def compute(self):
        return self.value


class _Count:
    def __init__(self):
        self.count = 0

    def update(self, x):
        self.count += x.numel()

    def compute(self):
        return torch.tensor(float(self.count), dtype=F64)


def make(kind):
    return {"mean": lambda: _RunningMean(lambda x: x), "mean_abs": lambda: _RunningMean(torch.abs),
            "rms": lambda: _RootMeanSquare(torch.square), "std": lambda: _Std(False, True), "var": lambda: _Std(True, True),
            "std_biased": lambda: _Std(False, False), "max": lambda: _Extreme(True, False),
            "absmax": lambda: _Extreme(True, True), "min": lambda: _Extreme(False, False),
            "absmin": lambda: _Extreme(False, True), "count": _Count}[kind]()


def edge_lengths(data):
    pos, ei = data["pos"].to(F64), data["edge_index"]
    vec = pos[ei[1]] - pos[ei[0]]
    if "cell" in data:
        cell = data["cell"].to(F64).reshape(-1, 3, 3)
        frame = data["batch"][ei[0]] if "batch" in data else torch.zeros_like(ei[0])
        vec = vec + torch.einsum("ei,eij->ej", data["edge_cell_shift"].to(F64), cell[frame])
    return vec.square().sum(1, keepdim=True).sqrt()


def num_neighbors(data):
    counts = [0] * data["pos"].shape[0]
    for c in data["edge_index"][0].tolist():  # atom i gets its OWN count
        counts[c] += 1
    return torch.tensor(counts, dtype=F64, device=data["pos"].device)


def field_of(field, data):
    """(tensor in float64, "graph" | "node" | "edge")"""
    if field == "num_neighbors":
        return num_neighbors(data), "node"
    if field == "edge_lengths":
        return edge_lengths(data), "edge"
    if field.startswith("per_atom:"):
        x = data[field[len("per_atom:"):]].to(F64)
        inv = 1.0 / data["num_atoms"].reshape(-1).to(F64)
        return x * inv.reshape((-1,) + (1,) * (x.dim() - 1)), "graph"
    return data[field].to(F64), "node" if field in NODE_FIELDS else "graph"


def evaluate(entries, batches, type_names):
    """``compute()`` of the reference's manager (with the two deviations) after the batches, values as Python floats."""
    T = len(type_names)
    running = []
    for e in entries:
        n = 1
        if e.get("per_type"):
            n = T * T if e["field"] == "edge_lengths" else T
        running.append([make(e["kind"]) for _ in range(n)])
    for data in batches:
        for e, objs in zip(entries, running):
            x, ftype = field_of(e["field"], data)
            if e.get("per_type"):
                types = data["atom_types"].reshape(-1)
                if ftype == "node":
                    group = types
                else:
                    ei = data["edge_index"]
                    group = types[ei[0]] * T + types[ei[1]]
                for g, obj in enumerate(objs):
                    sel = x[group == g]
                    if e.get("ignore_nan"):
                        sel = sel[~torch.isnan(sel)]
                    obj.update(sel.reshape(-1))
            else:
                sel = x.reshape(-1)
                if e.get("ignore_nan"):
                    sel = sel[~torch.isnan(sel)]
                objs[0].update(sel)
    out = {}
    for e, objs in zip(entries, running):
        name = e["name"]
        if not e.get("per_type"):
            out[name] = float(objs[0].compute())
            continue
        per = {}
        if e["field"] == "edge_lengths":
            for c, cn in enumerate(type_names):
                for n, nn in enumerate(type_names):
                    v = float(objs[c * T + n].compute())  # accumulated AND named at c * T + n
                    per[f"{cn}_{nn}"] = v
                    out[f"{name}_{cn}{nn}"] = v
        else:
            for g, tn in enumerate(type_names):
                v = float(objs[g].compute())
                per[tn] = v
                out[f"{name}_{tn}"] = v
        out[name] = per
    return out
