from . import AtomicDataDict  # noqa: F401
from ._key_registry import register_fields  # noqa: F401
from .modifier import BaseModifier, EdgeLengths, MappedFieldModifier, NumNeighbors, PerAtomModifier  # noqa: F401
from .stats import Count, Max, Mean, MeanAbsolute, Min, RootMeanSquare, StandardDeviation  # noqa: F401
from .stats_manager import (CommonDataStatisticsManager, DataStatisticsManager,  # noqa: F401
                            EnergyOnlyDataStatisticsManager)
