"""``MetricsManager``: losses and monitored error metrics on ``AtomicDataDict`` pairs (interface and semantics of
``nequip/train/metrics_manager.py``), evaluated as ONE fused reduction.

``metrics`` is a list of dicts with the keys

``metric`` (required)   a metric object (``MeanSquaredError()``, ``HuberLoss(delta=...)``, ...; ``nequip_amd.train.metrics``)
``field``               a field name, a ``BaseModifier`` (e.g. ``PerAtomModifier("total_energy")``), or ``None``: the metric is
                        then a custom module called with the two data dicts, outside the fused launch (no ``per_type`` /
                        ``ignore_nan`` for it)
``coeff``               weight in ``weighted_sum``; the coefficients are normalised to sum to 1, entries without one are reported
                        but left out of ``weighted_sum``, which exists only if some coefficient is set (a reserved name)
``name``                defaults to ``"<field>_<metric>"`` with the abbreviations of ``_key_registry.ABBREV``; must be unique
``per_type``            per-atom fields only, needs ``type_names``: one value per atom type (``"<name>_<type>"``) and their
                        aggregate.  Per batch a type without contributing element is NaN and left out of the aggregate; per
                        epoch (``compute``) every configured type enters and NaN propagates
``per_type_coeffs``     ``{type name: positive float}`` for every type: the aggregate becomes ``sum(c_i m_i) / sum(c_i)``
``ignore_nan``          elements whose TARGET is NaN contribute nothing (partial labels)

``manager(preds, target, prefix, suffix)`` returns the values of the batch and accumulates them; ``compute(prefix, suffix)``
returns the accumulated values (all-reducing the state first under an initialised ``torch.distributed``); ``reset()`` clears
them.  Every distinct (prediction, target) pair is read once; all terms, per-type groups, NaN masks, ``weighted_sum`` and the
running state are computed on the device (``csrc/metrics.hip``: two launches forward, one backward) and nothing is read by
the host, so a step with its loss captures into a hipGraph.  The returned values are 0-dim views of one device vector;
``metrics_values_step`` / ``metrics_values_epoch`` copy that vector to the host once, when first looked at.

Differences from the reference, both deliberate: predictions and targets are promoted to float64 before they are subtracted;
a per-type batch in which NO type contributes gives NaN instead of a ``ZeroDivisionError`` (raising would need a host read).
"""

from __future__ import annotations

import dataclasses
from collections.abc import Mapping
from typing import Any, Dict, Final, Iterator, List, Optional

import torch

from ..data import AtomicDataDict, BaseModifier, MappedFieldModifier, PerAtomModifier
from . import _metrics_ops as _ops
from .metrics import MaximumAbsoluteError, MeanAbsoluteError, MeanSquaredError, RootMeanSquaredError, _FusedMetric


@dataclasses.dataclass
class MetricEntry:
    field: Optional[BaseModifier]
    coeff: Optional[float]
    ignore_nan: bool
    per_type: bool
    per_type_coeffs: Optional[List[float]]


_METRICS_MANAGER_INPUT_KEYS: Final[frozenset] = frozenset({f.name for f in dataclasses.fields(MetricEntry)} | {"metric", "name"})


class _LazyValues(Mapping):
    """``{entry name: float}``, in entry order, over a device vector that is copied to the host once, when a value is first
    looked at (``extra``: the values of the custom ``field=None`` entries, which are not in the vector)."""

    def __init__(self, names: List[str], vector: Optional[torch.Tensor], index: Dict[str, int], extra: Dict[str, Any]):
        self._names, self._vector, self._index, self._extra, self._host = names, vector, index, extra, None

    def __getitem__(self, key: str) -> float:
        if key in self._extra:
            v = self._extra[key]
            return v.item() if isinstance(v, torch.Tensor) else v
        if self._host is None:
            self._host = self._vector.detach().cpu().tolist()
        return self._host[self._index[key]]

    def __iter__(self) -> Iterator[str]:
        return iter(self._names)

    def __len__(self) -> int:
        return len(self._names)


def _stream_key(field: BaseModifier):
    """Entries with equal keys share one stream: the same tensors, read once."""
    if type(field) is BaseModifier:
        return ("field", field.field)
    if type(field) is PerAtomModifier:
        return ("per_atom", field.field, field._factor)
    if type(field) is MappedFieldModifier:
        return ("mapped", field.pred_field, field.target_field)
    return ("custom", id(field))


class MetricsManager(torch.nn.ModuleDict):
    def __init__(self, metrics: List[Dict[str, Any]], type_names: Optional[List[str]] = None):
        super().__init__()
        if any(m.get("per_type", False) for m in metrics):
            assert type_names is not None, "`type_names` must be provided if any `per_type=True`"
            self.type_names = type_names

        self.entries: Dict[str, MetricEntry] = {}
        for metric_dict in metrics:
            name, entry, module = self.parse_entry(metric_dict, type_names)
            assert name not in self.entries, (
                f"Repeated names found ({name}) -- names must be unique. It is recommended to give custom names instead of "
                "relying on the automatic naming.")
            self.entries[name] = entry
            self.update({name: module})

        # the fused plan: one stream per distinct field modifier, one term per entry with a field
        self._stream_fields: List[BaseModifier] = []
        self._stream_grouped: List[bool] = []
        keys: Dict[Any, int] = {}
        self._term_of: Dict[str, int] = {}
        terms = []
        for name, entry in self.entries.items():
            if entry.field is None:
                continue
            module = self[name]
            if not isinstance(module, _FusedMetric):
                raise TypeError(f"the metric of `{name}` is a {type(module).__name__}: entries with a `field` take the metric "
                                "classes of nequip_amd.train (custom modules go with `field: None`)")
            key = _stream_key(entry.field)
            if key not in keys:
                keys[key] = len(self._stream_fields)
                self._stream_fields.append(entry.field)
                self._stream_grouped.append(False)
            s = keys[key]
            self._stream_grouped[s] = self._stream_grouped[s] or entry.per_type
            self._term_of[name] = len(terms)
            terms.append(module.term_spec(s, n_groups=len(type_names) if entry.per_type else 1, ignore_nan=entry.ignore_nan,
                                          group_coeffs=entry.per_type_coeffs))
        self.__dict__["_plan"] = _ops.FusedPlan(terms, len(self._stream_fields)) if terms else None

        self.do_weighted_sum = False
        self.set_coeffs({k: v.coeff for k, v in self.entries.items()})
        self.metrics_values_step = {k: None for k in self.entries}
        self.metrics_values_epoch = {k: None for k in self.entries}

    @staticmethod
    def parse_entry(metric_dict: Dict[str, Any], type_names: Optional[List[str]]):
        """One metric dict -> ``(name, MetricEntry, metric module)``, with the reference's checks and exception types."""
        for key in metric_dict:
            assert key in _METRICS_MANAGER_INPUT_KEYS, f"unrecognized key `{key}` found as input in `MetricsManager`"
        assert "metric" in metric_dict, "each dictionary in `MetricsManager`'s `metrics` argument must contain a `metric` key"

        field = metric_dict.get("field", None)
        if isinstance(field, str):
            field = BaseModifier(field)
        assert field is None or isinstance(field, BaseModifier)
        metric = metric_dict["metric"]

        name = metric_dict.get("name", None)
        if name is None:
            name = str(metric) if field is None else f"{field}_{metric}"
        assert name != "weighted_sum", "`weighted_sum` is a specially reserved metric name that should not be configured."

        if field is None:
            for key in ("ignore_nan", "per_type"):
                assert key not in metric_dict, f"When field is not provided or `field: None`, `{key}` should not be provided."

        ignore_nan = metric_dict.get("ignore_nan", False)
        assert isinstance(ignore_nan, bool), f"`ignore_nan` should be a bool, but found {ignore_nan} of type {type(ignore_nan)}"

        per_type = bool(metric_dict.get("per_type", False))
        if per_type:
            assert type_names is not None, "`type_names` must be provided if any `per_type=True`"
            if field.type != "node":
                raise RuntimeError(f"`per_type` metrics only supported for node fields, but {field.type} field found for {name}.")

        per_type_coeffs = None
        raw = metric_dict.get("per_type_coeffs", None)
        if raw is not None:
            if not per_type:
                raise ValueError(f"`per_type_coeffs` provided for `{name}` but `per_type` is not True; per-type coefficients "
                                 "require `per_type: true`.")
            if not isinstance(raw, Mapping):
                raise TypeError("`per_type_coeffs` must be a dict mapping type name to positive float, got "
                                f"{type(raw).__name__}.")
            unknown, missing = set(raw) - set(type_names), set(type_names) - set(raw)
            if unknown:
                raise ValueError(f"`per_type_coeffs` for `{name}` contains type names {sorted(unknown)} not in `type_names` "
                                 f"{type_names}.")
            if missing:
                raise ValueError(f"`per_type_coeffs` for `{name}` must specify a positive coefficient for every type in "
                                 f"`type_names`; missing: {sorted(missing)}.")
            per_type_coeffs = [float(raw[tn]) for tn in type_names]
            for tn, c in zip(type_names, per_type_coeffs):
                if c <= 0:
                    raise ValueError(f"`per_type_coeffs` entry for `{tn}` must be positive (got {c}).")

        entry = MetricEntry(field=field, coeff=metric_dict.get("coeff", None), ignore_nan=ignore_nan, per_type=per_type,
                            per_type_coeffs=per_type_coeffs)
        return name, entry, metric

    # ---- evaluation ------------------------------------------------------------------------------------------------------
    def _streams(self, preds, target):
        out = []
        for field, grouped in zip(self._stream_fields, self._stream_grouped):
            if type(field) is PerAtomModifier:
                p, t, scale = preds[field.field], target[field.field], field.row_scale(preds)
            else:
                (p, t), scale = field(preds, target), None
            group = preds[AtomicDataDict.ATOM_TYPE_KEY] if grouped else None
            out.append((p, t, scale, group))
        return out

    def _named(self, vector: Optional[torch.Tensor], custom: Dict[str, torch.Tensor], prefix: str, suffix: str):
        """The result dict in entry order (per-type values before their aggregate), ``weighted_sum`` last."""
        plan = self.__dict__["_plan"]
        out, ws = {}, None
        for name, entry in self.entries.items():
            if entry.field is None:
                value = custom[name]
            else:
                t = plan.terms[self._term_of[name]]
                if entry.per_type:
                    for g, tn in enumerate(self.type_names):
                        out[f"{prefix}{name}_{tn}{suffix}"] = vector[t.out0 + g]
                value = vector[t.value_index]
            out[f"{prefix}{name}{suffix}"] = value
            if self.do_weighted_sum and entry.field is None and entry.coeff is not None:
                ws = value * entry.coeff if ws is None else ws + value * entry.coeff
        if self.do_weighted_sum:
            fused = vector[plan.ws_index] if plan is not None and any(t.coeff is not None for t in plan.terms) else None
            out[f"{prefix}weighted_sum{suffix}"] = fused if ws is None else (ws if fused is None else fused + ws)
        return out

    def _lazy(self, vector, custom):
        plan = self.__dict__["_plan"]
        index = {name: plan.terms[i].value_index for name, i in self._term_of.items()}
        return _LazyValues(list(self.entries), None if vector is None else vector.detach(), index,
                           {k: v.detach() for k, v in custom.items()})

    def forward(self, preds: AtomicDataDict.Type, target: AtomicDataDict.Type, prefix: str = "", suffix: str = ""):
        """Values of this batch (differentiable w.r.t. the predictions); the batch is also accumulated."""
        plan = self.__dict__["_plan"]
        vector = plan.evaluate(self._streams(preds, target)) if plan is not None else None
        custom = {name: self[name](preds, target) for name, e in self.entries.items() if e.field is None}
        self.metrics_values_step = self._lazy(vector, custom)
        return self._named(vector, custom, prefix, suffix)

    def compute(self, prefix: str = "", suffix: str = ""):
        """Accumulated values (intended for the end of an epoch).  Unlike a step this synchronises with the host: the state
        (three small vectors) is copied to the CPU and the dozen scalar operations are done there."""
        plan = self.__dict__["_plan"]
        vector = None
        if plan is not None:
            state = plan.state()
            if torch.distributed.is_available() and torch.distributed.is_initialized():
                torch.distributed.all_reduce(state[0], op=torch.distributed.ReduceOp.SUM)
                torch.distributed.all_reduce(state[1], op=torch.distributed.ReduceOp.SUM)
                torch.distributed.all_reduce(state[2], op=torch.distributed.ReduceOp.MAX)
            vector = plan.epoch_values(state)
        custom = {name: self[name].compute() for name, e in self.entries.items() if e.field is None}
        self.metrics_values_epoch = self._lazy(vector, custom)
        return self._named(vector, custom, prefix, suffix)

    def reset(self):
        if self.__dict__["_plan"] is not None:
            self.__dict__["_plan"].reset()
        for name, entry in self.entries.items():
            if entry.field is None and hasattr(self[name], "reset"):
                self[name].reset()

    # ---- coefficients and checkpoint state ---------------------------------------------------------------------------------
    def set_coeffs(self, coeff_dict: Dict[str, Optional[float]]) -> None:
        """Normalise the coefficients to sum to 1 and set them; names that are missing get ``None``.  The device table is
        rewritten in place, so a captured graph sees the new coefficients at its next replay.  Call it between steps: a
        backward whose forward ran under the previous coefficients is refused."""
        coeffs = {k: coeff_dict.get(k) for k in self.entries}
        tot = sum(v for v in coeffs.values() if v is not None)
        self.do_weighted_sum = tot > 0
        plan = self.__dict__["_plan"]
        for name, entry in self.entries.items():
            c = coeffs[name]
            entry.coeff = (c / tot) if (c is not None and self.do_weighted_sum) else None
            if name in self._term_of:
                plan.terms[self._term_of[name]].coeff = entry.coeff
        if plan is not None:
            plan.coeffs_changed()  # (in place: a captured graph sees the new coefficients)

    def get_extra_state(self) -> Dict[str, Any]:
        return {
            "coeff_dict": {k: v.coeff for k, v in self.entries.items()},
            "metrics_values_step": dict(self.metrics_values_step),
            "metrics_values_epoch": dict(self.metrics_values_epoch),
        }

    def set_extra_state(self, state: Dict) -> None:
        self.set_coeffs(state["coeff_dict"])
        self.metrics_values_step = state["metrics_values_step"]
        self.metrics_values_epoch = state["metrics_values_epoch"]


# ---- builders -----------------------------------------------------------------------------------------------------------------
_E, _F, _S = AtomicDataDict.TOTAL_ENERGY_KEY, AtomicDataDict.FORCE_KEY, AtomicDataDict.STRESS_KEY


def _energy_field(per_atom: bool):
    return PerAtomModifier(_E) if per_atom else _E


def _loss(fields, coeffs, per_atom_energy, per_type_forces_coeffs, ignore_nan, type_names, extra_metrics):
    """MSE terms of a loss: ``per_atom_energy_mse`` or ``total_energy_mse``, ``forces_mse``, ``stress_mse``."""
    ignore_nan = {} if ignore_nan is None else ignore_nan
    metrics = []
    for f in fields:
        if f == _E:
            entry = {"name": "per_atom_energy_mse" if per_atom_energy else "total_energy_mse",
                     "field": _energy_field(per_atom_energy)}
        else:
            entry = {"name": f"{f}_mse", "field": f}
        entry.update(coeff=coeffs[f], metric=MeanSquaredError())
        entry["ignore_nan"] = ignore_nan.get(f, False)
        if f == _F and per_type_forces_coeffs is not None:
            entry.update(per_type=True, per_type_coeffs=per_type_forces_coeffs)
        metrics.append(entry)
    return MetricsManager(metrics + list(extra_metrics or []), type_names=type_names)


def EnergyForceLoss(coeffs: Dict[str, float] = {_E: 1.0, _F: 1.0}, per_atom_energy: bool = True,
                    per_type_forces_coeffs: Optional[Dict[str, float]] = None, type_names: Optional[List[str]] = None,
                    extra_metrics: Optional[List[Dict[str, Any]]] = None):
    """Loss of energy and force mean squared errors.  Terms: ``per_atom_energy_mse`` (or ``total_energy_mse`` with
    ``per_atom_energy=False``) and ``forces_mse`` -- the names to use with ``set_coeffs``.  ``per_type_forces_coeffs`` makes
    the force term a per-type weighted mean (see ``per_type_coeffs``)."""
    return _loss([_E, _F], coeffs, per_atom_energy, per_type_forces_coeffs, None, type_names, extra_metrics)


def EnergyForceStressLoss(coeffs: Dict[str, float] = {_E: 1.0, _F: 1.0, _S: 1.0}, per_atom_energy: bool = True,
                          per_type_forces_coeffs: Optional[Dict[str, float]] = None, type_names: Optional[List[str]] = None,
                          ignore_nan: Optional[Dict[str, bool]] = None, extra_metrics: Optional[List[Dict[str, Any]]] = None):
    """``EnergyForceLoss`` plus ``stress_mse``; ``ignore_nan={"stress": True}`` for frames without stress labels (NaN)."""
    return _loss([_E, _F, _S], coeffs, per_atom_energy, per_type_forces_coeffs, ignore_nan, type_names, extra_metrics)


def EnergyOnlyLoss(per_atom_energy: bool = True, type_names: Optional[List[str]] = None,
                   extra_metrics: Optional[List[Dict[str, Any]]] = None):
    """Loss of the energy mean squared error alone (``per_atom_energy_mse`` or ``total_energy_mse``, coefficient 1)."""
    return _loss([_E], {_E: 1.0}, per_atom_energy, None, None, type_names, extra_metrics)


_KINDS = (("rmse", RootMeanSquaredError), ("mae", MeanAbsoluteError), ("maxabserr", MaximumAbsoluteError))


def _metrics(quantities, default_on, coeffs, ignore_nan, type_names, extra_metrics):
    """rmse / mae / maxabserr of each quantity, in the reference's order: rmse and mae quantity by quantity, then the maxima."""
    keys = [f"{q}_{k}" for k, _ in _KINDS for q in quantities]
    if coeffs is None:
        coeffs = {k: (1.0 if k in default_on else None) for k in keys}
    assert all(k in keys for k in coeffs), f"Unrecognized key found in `coeffs`, only the following are recognized: {keys}"
    ignore_nan = {} if ignore_nan is None else ignore_nan
    field_of = {"total_energy": (_E, _E), "per_atom_energy": (lambda: PerAtomModifier(_E), _E), "forces": (_F, _F),
                "stress": (_S, _S)}

    def entry(q, kind, cls):
        field, raw = field_of[q]
        return {"name": f"{q}_{kind}", "field": field() if callable(field) else field, "metric": cls(),
                "coeff": coeffs.get(f"{q}_{kind}", None), "ignore_nan": ignore_nan.get(raw, False)}

    metrics = [entry(q, k, c) for q in quantities for k, c in _KINDS[:2]] + [entry(q, *_KINDS[2]) for q in quantities]
    return MetricsManager(metrics + list(extra_metrics or []), type_names=type_names)


def EnergyForceMetrics(coeffs: Optional[Dict[str, Optional[float]]] = None, type_names: Optional[List[str]] = None,
                       extra_metrics: Optional[List[Dict[str, Any]]] = None):
    """rmse, mae and maxabserr of ``total_energy``, ``per_atom_energy`` and ``forces`` (names ``"<quantity>_<kind>"``);
    ``coeffs`` weights them in ``weighted_sum`` (default: ``total_energy_rmse`` and ``forces_rmse`` at 1)."""
    return _metrics(["total_energy", "per_atom_energy", "forces"], ("total_energy_rmse", "forces_rmse"), coeffs, None,
                    type_names, extra_metrics)


def EnergyForceStressMetrics(coeffs: Optional[Dict[str, Optional[float]]] = None, type_names: Optional[List[str]] = None,
                             ignore_nan: Optional[Dict[str, bool]] = None,
                             extra_metrics: Optional[List[Dict[str, Any]]] = None):
    """``EnergyForceMetrics`` plus the three ``stress`` metrics (default also ``stress_rmse`` at 1); ``ignore_nan`` per field
    (``total_energy``, ``forces``, ``stress``)."""
    return _metrics(["total_energy", "per_atom_energy", "forces", "stress"],
                    ("total_energy_rmse", "forces_rmse", "stress_rmse"), coeffs, ignore_nan, type_names, extra_metrics)


def EnergyOnlyMetrics(coeffs: Optional[Dict[str, Optional[float]]] = None, type_names: Optional[List[str]] = None,
                      extra_metrics: Optional[List[Dict[str, Any]]] = None):
    """rmse, mae and maxabserr of ``total_energy`` and ``per_atom_energy`` (default: ``total_energy_rmse`` at 1)."""
    return _metrics(["total_energy", "per_atom_energy"], ("total_energy_rmse",), coeffs, None, type_names, extra_metrics)
