"""A plain-torch float64 restatement of the loss / metric semantics of nequip's ``MetricsManager``
(nequip/train/metrics_manager.py:283-411, nequip/train/metrics.py, nequip/data/stats.py::_MeanX,
nequip/data/modifier.py::PerAtomModifier), written from their definitions in this project's own words: loops over types,
boolean indexing, and -- this project's one deliberate difference -- promotion to float64 BEFORE the subtraction.
Differentiable by autograd w.r.t. the predictions; runs on any device.

An ENTRY is a dict: ``name``, ``field`` (key of both data dicts), ``kind`` ("mse", "mae", "rmse", "max_ae", "huber",
"stratified huber"), and optionally ``per_atom`` (divide both sides by ``num_atoms``; ``factor``), ``coeff`` (raw; normalised
here), ``per_type``, ``per_type_coeffs`` (list in type order), ``ignore_nan``, ``delta``, ``delta_dict``, ``reduction``.
"""
import math

import torch


def element_loss(kind, d, target, delta=1.0, delta_dict=None):
    """The modifier of the difference ``d`` ([R, C] float64), element by element."""
    if kind in ("mse", "rmse"):
        return d.square()
    if kind in ("mae", "max_ae"):
        return d.abs()
    if kind == "huber":
        return torch.where(d.abs() < delta, 0.5 * d.square(), delta * (d.abs() - 0.5 * delta))
    assert kind == "stratified huber"
    if min(delta_dict) > 0:
        delta_dict = {0: math.inf, **delta_dict}
    bounds, deltas = list(delta_dict.keys()), list(delta_dict.values())
    norm = target.square().sum(-1).sqrt()
    out = torch.zeros_like(d)
    for i, dl in enumerate(deltas):  # rows with bound_i <= |target row|, and not bound_{i+1} <= |target row|
        rows = norm >= bounds[i]
        if i + 1 < len(bounds):
            rows = rows & ~(norm >= bounds[i + 1])
        x = d[rows]
        out[rows] = 0.5 * x.square() if math.isinf(dl) else torch.where(x.abs() < dl, 0.5 * x.square(),
                                                                         dl * (x.abs() - 0.5 * dl))
    return out


def sums(kind, pred, target, scale=None, ignore_nan=False, **kw):
    """(sum of the modifier, number of contributing elements, max |d|) of one set of rows."""
    cols = max(1, math.prod(pred.shape[1:]))
    p, t = pred.to(torch.float64).reshape(-1, cols), target.to(torch.float64).reshape(-1, cols)
    if scale is not None:
        p, t = p * scale[:, None], t * scale[:, None]
    if ignore_nan:  # masked on the target, BEFORE anything is computed from the pair (masked elements: zero gradient)
        assert kind != "stratified huber", "needs whole rows"
        keep = ~torch.isnan(t)
        p, t = p[keep][:, None], t[keep][:, None]
    v = element_loss(kind, p - t, t, **kw)
    mx = v.detach().max() if (kind == "max_ae" and v.numel() > 0) else torch.tensor(-math.inf, dtype=torch.float64)
    return v.sum(), v.numel(), mx


def value(kind, s, n, mx, reduction="mean"):
    if kind == "max_ae":
        return mx
    if kind in ("huber", "stratified huber") and reduction == "sum":
        return s
    mean = s / n if n > 0 else torch.tensor(math.nan, dtype=torch.float64)
    return mean.sqrt() if kind == "rmse" else mean


def _loss_kw(e):
    return {k: e[k] for k in ("delta", "delta_dict") if k in e}


def _inputs(e, preds, target):
    scale = None
    if e.get("per_atom"):
        scale = preds["num_atoms"].reshape(-1).to(torch.float64).reciprocal() * (e.get("factor") or 1.0)
    return preds[e["field"]], target[e["field"]], scale


def normalised_coeffs(entries):
    tot = sum(e["coeff"] for e in entries if e.get("coeff") is not None)
    return {e["name"]: (e["coeff"] / tot if e.get("coeff") is not None and tot > 0 else None) for e in entries}


def evaluate(entries, batches, type_names=None, epoch=False):
    """``{name: value}`` as ``MetricsManager`` returns it.  ``batches``: list of ``(preds, target)`` dict pairs.
    ``epoch=False``: the value of the single batch given (types without a value are left out of the aggregate);
    ``epoch=True``: the accumulated value over all batches (every type enters, NaN propagates)."""
    assert epoch or len(batches) == 1
    coeffs = normalised_coeffs(entries)
    out, ws = {}, 0.0
    for e in entries:
        kind, red = e["kind"], e.get("reduction", "mean")
        groups = range(len(type_names)) if e.get("per_type") else [None]
        vals = []
        for g in groups:
            s, n, mx = 0.0, 0, torch.tensor(-math.inf, dtype=torch.float64)
            for preds, target in batches:
                p, t, scale = _inputs(e, preds, target)
                if g is not None:
                    rows = preds["atom_types"].reshape(-1) == g
                    p, t = p[rows], t[rows]
                s_b, n_b, mx_b = sums(kind, p, t, scale, e.get("ignore_nan", False), **_loss_kw(e))
                s, n, mx = s + s_b, n + n_b, torch.maximum(mx, mx_b.to(mx.device))
            vals.append(value(kind, s, n, mx, red))
        if e.get("per_type"):
            for tn, v in zip(type_names, vals):
                out[f"{e['name']}_{tn}"] = v
            c = e.get("per_type_coeffs") or [1.0] * len(vals)
            use = [i for i, v in enumerate(vals) if epoch or not torch.isnan(v)]
            num = sum(c[i] * vals[i] for i in use)
            den = sum(c[i] for i in use)
            m = num / den if use else torch.tensor(math.nan, dtype=torch.float64)
        else:
            m = vals[0]
        out[e["name"]] = m
        if coeffs[e["name"]] is not None:
            ws = ws + m * coeffs[e["name"]]
    if any(c is not None for c in coeffs.values()):
        out["weighted_sum"] = ws
    return out
