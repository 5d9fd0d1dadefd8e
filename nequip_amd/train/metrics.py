"""The metric classes of ``MetricsManager`` (interface of ``nequip/train/metrics.py``; running mean as in
``nequip/data/stats.py::_MeanX``: a float64 sum and an integer count).

A metric object here is a DESCRIPTION -- kind, ``delta``, ``reduction``, strata -- that ``MetricsManager`` compiles into one
term of its fused reduction (``_metrics_ops.FusedPlan``); the arithmetic is in ``csrc/metrics.hip`` (GPU tensors) or
``_metrics_ops._aten_forward`` (CPU tensors).  Used on its own, ``metric(preds, target)`` returns the batch value and
accumulates, ``compute()`` returns the accumulated value, ``reset()`` clears it -- through a one-term plan of its own.

Predictions and targets are promoted to float64 BEFORE they are subtracted (the reference subtracts in their own dtype).
``MaximumAbsoluteError`` is a metric, not a loss: it is computed detached and receives no gradient.
"""

from __future__ import annotations

import copy
from typing import Dict

import torch

from . import _metrics_ops as _ops


class _FusedMetric(torch.nn.Module):
    kind: int = -1
    _name: str = ""

    def __init__(self):
        super().__init__()
        self.__dict__["_plan"] = None

    # what MetricsManager compiles
    def term_spec(self, stream: int, **kw) -> _ops.TermSpec:
        return _ops.TermSpec(stream=stream, kind=self.kind, **kw)

    # stand-alone use
    def _own_plan(self) -> _ops.FusedPlan:
        if self.__dict__.get("_plan") is None:
            self.__dict__["_plan"] = _ops.FusedPlan([self.term_spec(0)], 1)
        return self.__dict__["_plan"]

    def forward(self, preds: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        """The value of this batch (differentiable w.r.t. ``preds``); the batch is also added to the running state."""
        return self._own_plan().evaluate([(preds, target, None, None)])[0]

    def update(self, preds: torch.Tensor, target: torch.Tensor) -> None:
        self.forward(preds.detach(), target)

    def compute(self) -> torch.Tensor:
        plan = self._own_plan()
        return plan.epoch_values(plan.state())[0]

    def reset(self) -> None:
        if self.__dict__.get("_plan") is not None:
            self.__dict__["_plan"].reset()

    def clone(self):
        return copy.deepcopy(self)

    def __str__(self) -> str:
        return self._name


class MeanSquaredError(_FusedMetric):
    """Mean squared error."""

    kind, _name = _ops.MSE, "mse"


class MeanAbsoluteError(_FusedMetric):
    """Mean absolute error."""

    kind, _name = _ops.MAE, "mae"


class RootMeanSquaredError(_FusedMetric):
    """Root mean squared error: the root is taken of the accumulated mean."""

    kind, _name = _ops.RMSE, "rmse"


class MaximumAbsoluteError(_FusedMetric):
    """Maximum absolute error (``-inf`` before the first element).  Computed detached: no gradient."""

    kind, _name = _ops.MAXABS, "max_ae"


class HuberLoss(_FusedMetric):
    """Huber loss: ``x^2 / 2`` for ``|x| < delta`` (strictly), ``delta (|x| - delta / 2)`` otherwise; ``delta`` has the units of
    the tensors.  ``reduction``: ``"mean"`` or ``"sum"``."""

    kind, _name = _ops.HUBER, "huber"

    def __init__(self, reduction: str = "mean", delta: float = 1.0):
        assert reduction in ["mean", "sum"]
        super().__init__()
        self.reduction, self.delta = reduction, float(delta)

    def term_spec(self, stream: int, **kw) -> _ops.TermSpec:
        return _ops.TermSpec(stream=stream, kind=self.kind, delta=self.delta, reduce_sum=self.reduction == "sum", **kw)


class StratifiedHuberForceLoss(_FusedMetric):
    """Huber loss on vectors (forces) whose ``delta`` depends on the magnitude of the TARGET vector: ``delta_dict`` maps a
    lower bound of ``|target row|`` to the ``delta`` used from there up to the next lower bound.  If the first lower bound is
    above 0, rows below it get half the squared error (an implicit ``{0: inf}`` stratum).  At least two strata."""

    kind, _name = _ops.STRATIFIED_HUBER, "stratified huber"

    def __init__(self, delta_dict: Dict[float, float], reduction: str = "mean"):
        if min(delta_dict.keys()) > 0:
            delta_dict = {0: float("inf"), **delta_dict}
        assert reduction in ["mean", "sum"]
        assert len(delta_dict) >= 2, "At least two delta values are required, otherwise use standard HuberLoss instead."
        super().__init__()
        self.delta_dict, self.reduction = dict(delta_dict), reduction

    def term_spec(self, stream: int, **kw) -> _ops.TermSpec:
        if kw.get("ignore_nan"):
            # masked_select flattens the rows in the reference, after which "row norm" means nothing
            raise ValueError("StratifiedHuberForceLoss needs whole target rows: `ignore_nan` is not supported for it")
        strata = [(float(b), float(d)) for b, d in self.delta_dict.items()]
        return _ops.TermSpec(stream=stream, kind=self.kind, strata=strata, reduce_sum=self.reduction == "sum", **kw)
