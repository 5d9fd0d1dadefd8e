"""Float64 restatement of ``TrainingStatsMonitor``'s statistics from Python floats and ``math.fsum`` (exactly rounded sums; two
passes for ``std``), the expected key list of a module, and the layout of ``tests/golden/ref_training_stats.npz``.

The fixture (``tests/golden/make_training_stats_golden.py``, the reference's own class): a module with the parameters ``SHAPES``
(float32, ``randn * 0.5 + 0.1``; ``frozen`` does not require a gradient, ``nograd`` never receives one), ``LOG_FREQ = 2`` and one
``torch.optim.Adam``.  Recorded: weights and gradients at step 0 (``w0_*``, ``g0_*``), weights, gradients and the Adam moments
after two optimizer steps (``w2_*``, ``g2_*``, ``m2_*``, ``v2_*``), and the reference's keys and values at steps 0 and 2
(``keys_0``, ``values_0``, ``keys_2``, ``values_2``) in the order of its ``log_dict`` calls.
"""
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_training_stats.npz")
LOG_FREQ = 2
SHAPES = {"lin.weight": (37, 5), "lin.bias": (2053,), "one": (1,), "frozen": (3,), "nograd": (7,), "pair": (2,)}
TRAINED = ("lin.weight", "lin.bias", "one", "pair")  # the parameters that receive gradients
PREFIX = "training_stats"
WEIGHT_STATS = ("min", "max", "mean", "std", "absmin", "absmax")
GRADIENT_STATS = ("absmax", "rms")
EXP_AVG_STATS = ("absmax", "rms")
SQRT_EXP_AVG_SQ_STATS = ("min", "max", "mean")
NAN = float("nan")


def stats(values, sqrt=False):
    """All seven statistics of a flat list of Python floats (of ``sqrt(v)`` element by element with ``sqrt``).  One NaN makes
    them all NaN; with an infinity and no NaN, ``mean`` and ``std`` are reported as NaN (only "non-finite" is specified)."""
    x = [math.sqrt(v) if (sqrt and v >= 0.0) else (NAN if sqrt else v) for v in values]
    n = len(x)
    if any(v != v for v in x):
        return dict.fromkeys(("min", "max", "mean", "std", "absmin", "absmax", "rms"), NAN)
    ax = [abs(v) for v in x]
    out = {"min": min(x), "max": max(x), "absmin": min(ax), "absmax": max(ax)}
    if any(math.isinf(v) for v in x):
        out.update(mean=NAN, std=NAN, rms=math.inf)
        return out
    mean = math.fsum(x) / n
    out["mean"] = mean
    out["std"] = math.sqrt(math.fsum((v - mean) ** 2 for v in x) / (n - 1)) if n > 1 else NAN
    out["rms"] = math.sqrt(math.fsum(v * v for v in x) / n)
    return out


def tensor_stats(t, sqrt=False):
    return stats(t.detach().to("cpu", torch.float64).reshape(-1).tolist(), sqrt)


def expected(model, optimizers=(), log_weights=True, log_gradients=True, log_optimizer_states=True, name_prefix=""):
    """``{key: value}`` of a logging step, in the order of the reference's three ``log_dict`` calls (gradients after the
    backward, then weights and optimizer states before the optimizer step).  Tensors without elements have no keys."""
    out = {}
    named = [(name_prefix + n, p) for n, p in model.named_parameters()]
    if log_gradients:
        for name, p in named:
            if p.requires_grad and p.grad is not None and p.grad.numel():
                s = tensor_stats(p.grad)
                out.update({f"{PREFIX}.gradients.{k}/{name}": s[k] for k in GRADIENT_STATS})
    if log_weights:
        for name, p in named:
            if p.requires_grad and p.numel():
                s = tensor_stats(p)
                out.update({f"{PREFIX}.weights.{k}/{name}": s[k] for k in WEIGHT_STATS})
    if log_optimizer_states:
        names = {id(p): name for name, p in named}
        for i, opt in enumerate(optimizers):
            suffix = f"_{i}" if len(optimizers) > 1 else ""
            for p, state in opt.state.items():
                if id(p) not in names or "exp_avg" not in state or "exp_avg_sq" not in state or not p.numel():
                    continue
                s = tensor_stats(state["exp_avg"])
                out.update({f"{PREFIX}.optimizer{suffix}.exp_avg.{k}/{names[id(p)]}": s[k] for k in EXP_AVG_STATS})
                s = tensor_stats(state["exp_avg_sq"], sqrt=True)
                out.update({f"{PREFIX}.optimizer{suffix}.sqrt_exp_avg_sq.{k}/{names[id(p)]}": s[k]
                            for k in SQRT_EXP_AVG_SQ_STATS})
    return out


# ---- the fixture ------------------------------------------------------------------------------------------------------------
class FixtureModule(torch.nn.Module):
    def __init__(self, weights):
        super().__init__()
        self.lin = torch.nn.Module()
        self.lin.weight = torch.nn.Parameter(weights["lin.weight"].clone())
        self.lin.bias = torch.nn.Parameter(weights["lin.bias"].clone())
        self.one = torch.nn.Parameter(weights["one"].clone())
        self.frozen = torch.nn.Parameter(weights["frozen"].clone(), requires_grad=False)
        self.nograd = torch.nn.Parameter(weights["nograd"].clone())
        self.pair = torch.nn.Parameter(weights["pair"].clone())


def fixture_optimizer(model):
    return torch.optim.Adam([p for p in model.parameters() if p.requires_grad], lr=1e-2)


def set_state(model, tensors, tag):
    """Weights and gradients ``w{tag}_*`` / ``g{tag}_*`` into the module (``nograd`` keeps ``.grad = None``)."""
    with torch.no_grad():
        for name, p in model.named_parameters():
            if f"w{tag}_{name}" in tensors:
                p.copy_(tensors[f"w{tag}_{name}"])
            if name in TRAINED:
                p.grad = tensors[f"g{tag}_{name}"].clone().to(p.device)


def load_fixture():
    z = np.load(GOLDEN)
    tensors = {k: torch.from_numpy(z[k]) for k in z.files if k[0] in "wgmv" and k[1] in "02" and k[2] == "_"}
    logged = {step: dict(zip([str(k) for k in z[f"keys_{step}"]], z[f"values_{step}"].tolist())) for step in (0, LOG_FREQ)}
    return tensors, logged
