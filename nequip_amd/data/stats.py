"""Dataset statistics: what an entry of ``DataStatisticsManager`` computes (the classes of ``nequip/data/stats.py``).

The reference's classes are ``torchmetrics.Metric`` objects that hold their own running state and are updated tensor by tensor.
Here a class only DESCRIBES a term of the fused reduction (``_stats_ops.StatsPlan``): every slot of every term keeps the same
running state -- ``count``, ``mean`` (in two words), ``M2 = sum (y - mean)^2``, ``min``, ``max`` of ``y = m(x)`` -- and a class
says which element modifier ``m`` it needs (identity, ``abs``, ``square``) and what ``compute()`` forms from that state
(``value``).  The objects are ``nn.Module``s without parameters, buffers or state: the running state lives in the manager's plan
and, like the reference's non-persistent ``add_state``, is part of no ``state_dict``.
"""

from __future__ import annotations

import torch

IDENTITY, ABS, SQUARE = "identity", "abs", "square"


class _Statistic(torch.nn.Module):
    """``modifier``: the element modifier; ``value(count, mean, m2, mn, mx)``: float64 tensors [slots] -> float64 [slots]."""

    modifier = IDENTITY

    def value(self, count, mean, m2, mn, mx) -> torch.Tensor:
        raise NotImplementedError


def _mean_or_nan(count, mean):
    # (the reference divides the running sum by the running count: 0 / 0 = NaN for a slot without elements)
    return torch.where(count > 0, mean, torch.full_like(mean, float("nan")))


class Mean(_Statistic):
    """Mean, kept as a running mean (never as a running sum)."""

    def value(self, count, mean, m2, mn, mx):
        return _mean_or_nan(count, mean)

    def __str__(self) -> str:
        return "mean"


class MeanAbsolute(Mean):
    """Mean of the absolute values."""

    modifier = ABS

    def __str__(self) -> str:
        return "mean_abs"


class RootMeanSquare(Mean):
    """Square root of the mean of the squares."""

    modifier = SQUARE

    def value(self, count, mean, m2, mn, mx):
        return torch.sqrt(_mean_or_nan(count, mean))

    def __str__(self) -> str:
        return "rms"


class StandardDeviation(_Statistic):
    """Standard deviation (``squared=True``: variance) from Welford / Chan updates; ``unbiased`` divides by ``count - 1``."""

    def __init__(self, squared: bool = False, unbiased: bool = True):
        super().__init__()
        self.squared, self.unbiased = bool(squared), bool(unbiased)

    def value(self, count, mean, m2, mn, mx):
        denom = (count - 1) if self.unbiased else count
        variance = m2 / denom.to(torch.float64)  # (0 / 0 = NaN: a single element, or none with unbiased=False)
        return variance if self.squared else torch.sqrt(variance)

    def __str__(self) -> str:
        return "var" if self.squared else "std"


class Max(_Statistic):
    """Largest element (``abs=True``: largest absolute value); ``-inf`` without elements; a NaN element gives NaN."""

    def __init__(self, abs: bool = False):
        super().__init__()
        self.abs = bool(abs)

    @property
    def modifier(self):
        return ABS if self.abs else IDENTITY

    def value(self, count, mean, m2, mn, mx):
        return mx

    def __str__(self) -> str:
        return "absmax" if self.abs else "max"


class Min(Max):
    """Smallest element (``abs=True``: smallest absolute value); ``+inf`` without elements; a NaN element gives NaN."""

    def value(self, count, mean, m2, mn, mx):
        return mn

    def __str__(self) -> str:
        return "absmin" if self.abs else "min"


class Count(_Statistic):
    """Number of elements."""

    def value(self, count, mean, m2, mn, mx):
        return count.to(torch.float64)

    def __str__(self) -> str:
        return "count"
