#!/usr/bin/env python3
"""Golden values of the training statistics, produced by the REFERENCE's own ``TrainingStatsMonitor``
(``nequip/train/callbacks/training_stats.py``).

``import nequip.train.callbacks`` pulls in the training stack; the class is loaded from its one file instead, with the stand-ins
of ``make_reference_golden.py`` for ``lightning`` and a stub ``nequip.train`` (``NequIPLightningModule = object``).  The callback
is driven by hand: a stand-in ``pl_module`` whose ``log_dict`` collects the dictionaries, a stand-in trainer that carries the
optimizers.

The module, the shapes and the layout of the file are described in ``tests/training_stats_restatement.py``.  Inputs are seeded
``randn * 0.5 + 0.1`` in float32 (``|mean|`` below the spread: the float32 bounds of ``tests/test_training_stats.py`` are
conditions on this choice).  With ``log_freq = 2`` the reference logs at step 0 (no optimizer state yet) and at step 2 (Adam
state after two steps).

    python tests/golden/make_training_stats_golden.py     # needs the reference tree; rewrites ref_training_stats.npz
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_reference_golden as mrg  # noqa: E402

import training_stats_restatement as tr  # noqa: E402


def reference_class():
    sys.meta_path.insert(0, mrg._Finder())
    for name in ("nequip", "nequip.train"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    sys.modules["nequip.train"].NequIPLightningModule = object
    path = os.path.join(mrg.REFERENCE, "nequip", "train", "callbacks", "training_stats.py")
    spec = importlib.util.spec_from_file_location("nequip.train.callbacks.training_stats", path)
    module = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = module
    spec.loader.exec_module(module)
    return module.TrainingStatsMonitor


class Collecting(tr.FixtureModule):
    """The stand-in ``pl_module``: ``log_dict`` collects what the callback logs."""

    def __init__(self, weights):
        super().__init__(weights)
        self.logged = {}

    def log_dict(self, values, sync_dist=False):
        assert sync_dist
        self.logged.update(values)


class Trainer:
    def __init__(self, optimizers):
        self.optimizers = optimizers


def draw(gen, shape):
    return (torch.randn(shape, generator=gen) * 0.5 + 0.1).float()


def main():
    Monitor = reference_class()
    gen = torch.Generator().manual_seed(20261019)
    tensors = {f"w0_{n}": draw(gen, s) for n, s in tr.SHAPES.items()}
    for step in range(tr.LOG_FREQ + 1):
        tensors.update({f"g{step}_{n}": draw(gen, tr.SHAPES[n]) for n in tr.TRAINED})
    module = Collecting({n: tensors[f"w0_{n}"] for n in tr.SHAPES})
    opt = tr.fixture_optimizer(module)
    trainer = Trainer([opt])
    mon = Monitor(log_freq=tr.LOG_FREQ)
    out = {}
    for step in range(tr.LOG_FREQ + 1):
        tr.set_state(module, tensors, step)
        module.logged = {}
        mon.on_after_backward(trainer, module)
        mon.on_before_optimizer_step(trainer, module, opt)
        assert bool(module.logged) == (step % tr.LOG_FREQ == 0)
        if module.logged:
            out[f"keys_{step}"] = np.array(list(module.logged.keys()))
            out[f"values_{step}"] = np.array(list(module.logged.values()), dtype=np.float64)
            for name, p in module.named_parameters():
                out[f"w{step}_{name}"] = p.detach().numpy().copy()
                if name in tr.TRAINED:
                    out[f"g{step}_{name}"] = p.grad.numpy().copy()
                if p in opt.state:
                    out[f"m{step}_{name}"] = opt.state[p]["exp_avg"].numpy().copy()
                    out[f"v{step}_{name}"] = opt.state[p]["exp_avg_sq"].numpy().copy()
        opt.step()
    assert mon.step_count == tr.LOG_FREQ + 1
    path = os.path.join(HERE, "ref_training_stats.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", {k: len(out[k]) for k in out if k.startswith("keys_")})


if __name__ == "__main__":
    main()
