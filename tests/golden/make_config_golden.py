#!/usr/bin/env python3
"""Golden vectors of the conflict-free gradients, produced by the REFERENCE's own method
(``nequip/train/config.py::ConFIGLightningModule._ConFIG_backwards``).

``import nequip.train.config`` pulls in Lightning and the training stack; the class is loaded from its one file instead, with
the stand-ins of ``make_reference_golden.py`` for ``lightning`` and stub modules for ``nequip.train.lightning``
(an empty ``NequIPLightningModule``), ``nequip.train.ema`` (an empty ``EMALightningModule``), ``nequip.data`` and
``nequip.utils.versions``.  The unbound method is then called on a bare object that carries what the method reads: the model
(``tests/config_restatement.py::GoldenMLP``), a loss with ``entries`` / ``keys()``, the parameter bookkeeping its ``__init__``
would have made, ``world_size = 1``, ``manual_backward = Tensor.backward``.

Recorded per model (``mixed``: one float64 parameter among float32 ones; ``f32``) and number of terms (2, 3): the per-term
gradients ``rows_{model}_{K}`` ([K, P], by ``torch.autograd.grad`` here, in the promoted dtype) and the final ``.grad``s laid
end to end, ``grad_{model}_{K}_{lstsq|pinv}``, each in float64 (the values are those of the parameters' dtypes).  The model's
parameters and inputs are regenerated from seeds by the tests.

    python tests/golden/make_config_golden.py     # needs the reference tree; rewrites ref_config.npz
"""
import importlib.util
import os
import sys
import types
from itertools import accumulate

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_reference_golden as mrg  # noqa: E402

import config_restatement as cr  # noqa: E402


def reference_method():
    sys.meta_path.insert(0, mrg._Finder())
    for name in ("nequip", "nequip.train", "nequip.utils", "nequip.data", "nequip.utils.versions", "nequip.train.lightning",
                 "nequip.train.ema"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    sys.modules["nequip.data"].AtomicDataDict = types.SimpleNamespace(Type=dict)
    sys.modules["nequip.utils.versions"]._TORCH_GE_2_6 = True
    base = type("NequIPLightningModule", (), {})  # (the file also derives a class from both: they must be two classes)
    sys.modules["nequip.train.lightning"].NequIPLightningModule = base
    sys.modules["nequip.train.ema"].EMALightningModule = type("EMALightningModule", (base,), {})
    spec = importlib.util.spec_from_file_location("nequip.train.config", os.path.join(mrg.REFERENCE, "nequip", "train", "config.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules["nequip.train.config"] = module
    spec.loader.exec_module(module)
    return module.ConFIGLightningModule._ConFIG_backwards


class _Loss(dict):
    """``keys()`` in entry order and ``entries[name].coeff``: what the method reads of a MetricsManager."""

    def __init__(self, names, coeffs):
        super().__init__({n: None for n in names})
        self.entries = {n: types.SimpleNamespace(coeff=c) for n, c in zip(names, coeffs)}


def bare_module(model, n_terms, lsqr):
    names = cr.GOLDEN_NAMES[:n_terms]
    params = dict(model.named_parameters())
    self = types.SimpleNamespace()
    self.model, self.loss = model, _Loss(names, cr.GOLDEN_COEFFS[n_terms])
    self.logging_delimiter, self.world_size = "/", 1
    self.manual_backward = lambda loss, **kw: loss.backward(**kw)
    self.ConFIG_model_param_names = list(params)
    self.ConFIG_param_numel_list = [p.numel() for p in params.values()]
    self.ConFIG_param_batch_list = [0] + list(accumulate(self.ConFIG_param_numel_list))
    self.ConFIG_param_shape_list = [p.shape for p in params.values()]
    self.ConFIG_loss_component_keys = {n: f"train_loss_step/{n}" for n in names}
    self.ConFIG_eps, self.ConFIG_lsqr = cr.EPS, lsqr
    return self


def main():
    method = reference_method()
    x, target = cr.golden_inputs()
    out = {}
    for kind in cr.GOLDEN_MODELS:
        for n_terms in (2, 3):
            model = cr.GoldenMLP(kind)
            params = list(model.parameters())
            terms = cr.golden_terms(model(x), target, n_terms)
            rows = []
            for name in cr.GOLDEN_NAMES[:n_terms]:
                gs = torch.autograd.grad(terms[name], params, retain_graph=True)
                rows.append(torch.cat([g.flatten() for g in gs]))
            out[f"rows_{kind}_{n_terms}"] = torch.stack(rows).double().numpy()
            for lsqr in (True, False):
                model = cr.GoldenMLP(kind)
                loss_dict = cr.golden_terms(model(x), target, n_terms, prefix="train_loss_step/")
                method(bare_module(model, n_terms, lsqr), loss_dict)
                for p in model.parameters():
                    assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
                flat = torch.cat([p.grad.double().flatten() for p in model.parameters()])
                out[f"grad_{kind}_{n_terms}_{'lstsq' if lsqr else 'pinv'}"] = flat.numpy()
    path = os.path.join(HERE, "ref_config.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
