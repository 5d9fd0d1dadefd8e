"""Entries and batches shared by ``tests/test_data_statistics.py`` (CPU) and ``tests/test_data_statistics_gpu.py``: the
entries in the form of ``tests/stats_restatement.py`` and as ``DataStatisticsManager`` dictionaries, and seeded batches with the
fields both sides read (``pos``, ``cell``, ``edge_cell_shift``, ``batch``, ``edge_index``, ``atom_types``, ``num_atoms``,
``total_energy``, ``forces``, ``charges`` [N, 1], ``fnan`` [N, 3] with a quarter of NaNs)."""
import math
from fractions import Fraction

import torch

import stats_restatement as sr
from nequip_amd.data import (Count, DataStatisticsManager, EdgeLengths, Max, Mean, MeanAbsolute, Min, NumNeighbors,
                             PerAtomModifier, RootMeanSquare, StandardDeviation, register_fields)

TYPES = ["H", "O", "Cs"]
KINDS = ["mean", "mean_abs", "rms", "std", "var", "std_biased", "max", "absmax", "min", "absmin", "count"]
register_fields(node_fields=["fnan"])  # (``charges`` is a per-atom field already)
sr.NODE_FIELDS.update({"fnan", "charges"})


def metric_of(kind):
    return {"mean": Mean, "mean_abs": MeanAbsolute, "rms": RootMeanSquare, "std": StandardDeviation,
            "var": lambda: StandardDeviation(squared=True), "std_biased": lambda: StandardDeviation(unbiased=False),
            "max": Max, "absmax": lambda: Max(abs=True), "min": Min, "absmin": lambda: Min(abs=True), "count": Count}[kind]()


def field_of(field):
    if field == "num_neighbors":
        return NumNeighbors()
    if field == "edge_lengths":
        return EdgeLengths()
    if field.startswith("per_atom:"):
        return PerAtomModifier(field[len("per_atom:"):])
    return field


def to_dicts(entries):
    """The ``DataStatisticsManager`` entries of restatement entries."""
    return [{"name": e["name"], "field": field_of(e["field"]), "metric": metric_of(e["kind"]),
             "per_type": bool(e.get("per_type", False)), "ignore_nan": bool(e.get("ignore_nan", False))} for e in entries]


def entries_for(fields, per_type=True, kinds=KINDS, ignore_nan=(False,)):
    """Every kind, plain (and per type), on every field."""
    out = []
    for f in fields:
        for k in kinds:
            for pt in ((False, True) if per_type else (False,)):
                for ig in ignore_nan:
                    out.append({"name": f"{f}|{k}|{'pt' if pt else 'all'}|{'drop' if ig else 'keep'}", "field": f, "kind": k,
                                "per_type": pt, "ignore_nan": ig})
    return out


def make_batch(sizes, seed, dtype=torch.float64, num_edges=None, type_choices=(0, 1), device="cpu"):
    """One batch of ``len(sizes)`` frames.  Random edges in any order (never a self edge); the LAST atom is isolated (the
    centre of no edge); types drawn from ``type_choices`` with the first atom of the first choice."""
    g = torch.Generator().manual_seed(seed)
    n, b = sum(sizes), len(sizes)
    e = (4 * n if num_edges is None else num_edges) if n > 1 else 0
    types = torch.tensor(type_choices)[torch.randint(0, len(type_choices), (n,), generator=g)] if n else torch.zeros(0).long()
    if n:
        types[0] = type_choices[0]
    center = torch.randint(0, max(n - 1, 1), (e,), generator=g)
    neighbor = (center + 1 + torch.randint(0, max(n - 1, 1), (e,), generator=g)) % max(n, 1)
    fnan = torch.randn(n, 3, generator=g, dtype=dtype)
    fnan[torch.rand(n, 3, generator=g) < 0.25] = math.nan
    data = {
        "pos": 3.0 * torch.randn(n, 3, generator=g, dtype=torch.float64),
        "cell": 10.0 * torch.eye(3, dtype=torch.float64).repeat(b, 1, 1)
        + torch.randn(b, 3, 3, generator=g, dtype=torch.float64),
        "edge_cell_shift": torch.randint(-1, 2, (e, 3), generator=g).to(torch.float64),
        "batch": torch.repeat_interleave(torch.arange(b), torch.tensor(sizes, dtype=torch.long)) if n else types.long(),
        "edge_index": torch.stack([center, neighbor]).long(),
        "atom_types": types.long(),
        "num_atoms": torch.tensor(sizes, dtype=torch.long),
        "total_energy": (-50.0 * torch.tensor(sizes, dtype=torch.float64)[:, None]
                         + torch.randn(b, 1, generator=g, dtype=torch.float64)).to(dtype),
        "forces": torch.randn(n, 3, generator=g, dtype=dtype),
        "charges": (0.5 + torch.randn(n, 1, generator=g, dtype=torch.float64)).to(dtype),
        "fnan": fnan,
    }
    return {k: v.to(device) for k, v in data.items()}


def three_batches(dtype=torch.float64, device="cpu"):
    """Unequal sizes with an empty batch in between; ``O`` is absent from the second batch and ``Cs`` from all of them."""
    return [make_batch([3, 5], 1, dtype, device=device), make_batch([], 2, dtype, device=device),
            make_batch([4], 3, dtype, type_choices=(0,), device=device), make_batch([2, 6, 1], 4, dtype, device=device)]


def assert_stats_close(got, ref, rtol=1e-10):
    """Same keys in the same order; floats at ``rtol`` (atol 0, NaN equals NaN), nested per-type dictionaries likewise."""
    assert list(got) == list(ref), (list(got), list(ref))
    for k in ref:
        if isinstance(ref[k], dict):
            assert_stats_close(got[k], ref[k], rtol)
            continue
        assert isinstance(got[k], float), (k, type(got[k]))
        torch.testing.assert_close(torch.tensor(got[k], dtype=torch.float64), torch.tensor(ref[k], dtype=torch.float64),
                                   rtol=rtol, atol=0.0, equal_nan=True, msg=lambda m, k=k: f"{k}: {m}")


# ---- cancellation ------------------------------------------------------------------------------------------------------------
def cancellation_case():
    """1000 values ``1e6 + 1e-2 randn`` in three batches, and their exact mean and standard deviation (rational arithmetic
    on the same float64 inputs)."""
    x = 1e6 + 1e-2 * torch.randn(1000, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    fr = [Fraction(v) for v in x.tolist()]
    mean = sum(fr) / len(fr)
    var = sum((f - mean) ** 2 for f in fr) / (len(fr) - 1)
    # sqrt of a rational: through float64 of the variance (one rounding, 1e-16) -- far below the errors compared
    return [x[:300], x[300:730], x[730:]], float(mean), math.sqrt(float(var))


def cancellation_errors(batches_of, device="cpu"):
    """(e_ref, e_new) per quantity: relative errors of the restatement and of the manager against the exact values."""
    parts, mean, std = cancellation_case()
    entries = [{"name": k, "field": "total_energy", "kind": k} for k in ("std", "mean")]
    batches = [{"total_energy": p.reshape(-1, 1)} for p in parts]
    ref = sr.evaluate(entries, batches, [])
    got = DataStatisticsManager(to_dicts(entries)).get_statistics(batches_of(batches))
    out = {}
    for name, exact in (("std", std), ("mean", mean)):
        out[name] = (abs(ref[name] - exact) / exact, abs(got[name] - exact) / exact)
        print(f"[cancellation, {device}] {name}: e_ref = {out[name][0]:.3e}, e_new = {out[name][1]:.3e}")
    return out
