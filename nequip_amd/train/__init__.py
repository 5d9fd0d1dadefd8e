from .simple_ddp import SimpleDDPStrategy, all_reduce_gradients, broadcast_parameters  # noqa: F401
from .ema import EMAWeights  # noqa: F401
from .config import ConFIGGradients  # noqa: F401
from .training_stats import TrainingStatsMonitor  # noqa: F401
from .schedulefree import AdamWScheduleFree, ScheduleFreeHooks  # noqa: F401
from .adam import Adam, AdamW, ReduceLROnPlateau  # noqa: F401
from .metrics import (  # noqa: F401
    HuberLoss,
    MaximumAbsoluteError,
    MeanAbsoluteError,
    MeanSquaredError,
    RootMeanSquaredError,
    StratifiedHuberForceLoss,
)
from .metrics_manager import (  # noqa: F401
    EnergyForceLoss,
    EnergyForceMetrics,
    EnergyForceStressLoss,
    EnergyForceStressMetrics,
    EnergyOnlyLoss,
    EnergyOnlyMetrics,
    MetricsManager,
)
