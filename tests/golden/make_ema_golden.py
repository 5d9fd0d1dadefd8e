#!/usr/bin/env python3
"""Golden vectors of the weight averaging, produced by the REFERENCE's own ``EMAWeights`` (``nequip/train/ema.py:105-245``).

``import nequip.train.ema`` pulls in the training stack; the class is loaded from its one file instead, with the stand-ins of
``make_reference_golden.py`` for ``lightning`` and stub modules for ``nequip.train.lightning`` (``NequIPLightningModule =
object``) and ``nequip.utils`` (``RankedLogger``).

The parameter list and the layout of the file are described in ``tests/ema_restatement.py``; the chunk length comes from the
built library (``nqa_ema_chunk_elems``).  Recorded: the float32 parameters before each of 12 updates, the EMA buffers after
updates 1, 2, 3, 8, 9, 10, 11, 12 with ``decay=0.5`` (the warm-up ends exactly at n = 8: both regimes and the crossover; 8 and
11 are the states before updates 9 and 12) and after updates 1 and 2 with ``decay=0.999``, the state-dict keys and the extra
state.  The buffers are filled with NaN before the first update.

    python tests/golden/make_ema_golden.py     # needs the reference tree and the built library; rewrites ref_ema.npz
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

import ema_restatement as er  # noqa: E402


def reference_class():
    sys.meta_path.insert(0, mrg._Finder())
    for name in ("nequip", "nequip.train", "nequip.utils"):
        mod = types.ModuleType(name)
        mod.__path__ = []
        sys.modules[name] = mod
    sys.modules["nequip.utils"].RankedLogger = lambda *a, **k: None
    stub = types.ModuleType("nequip.train.lightning")
    stub.NequIPLightningModule = object
    sys.modules["nequip.train.lightning"] = stub
    spec = importlib.util.spec_from_file_location("nequip.train.ema", os.path.join(mrg.REFERENCE, "nequip", "train", "ema.py"))
    module = importlib.util.module_from_spec(spec)
    sys.modules["nequip.train.ema"] = module
    spec.loader.exec_module(module)
    return module.EMAWeights


def parameters32(chunk, k, gen):
    """Float32 parameters before update ``k``: a drifting centre plus noise, the long tensor a tiling of one period."""
    out = []
    for shape in er.shapes(chunk):
        n = int(np.prod(shape, dtype=np.int64))
        m = er.PERIOD if n == 2 * chunk + 3 else n
        v = (torch.randn(m, generator=gen) * (0.5 + 0.25 * k) + 0.1 * k).float()
        out.append(torch.from_numpy(np.resize(v.numpy(), n).copy()).reshape(shape))
    return out


def main():
    from nequip_amd import _lib

    EMAWeights = reference_class()
    chunk = int(_lib.load().nqa_ema_chunk_elems())
    gen = torch.Generator().manual_seed(20261018)
    p32 = {k: parameters32(chunk, k, gen) for k in range(1, er.N_STEPS + 1)}
    out = {"chunk": np.array(chunk), "period": np.array(er.PERIOD)}
    for k, ps in p32.items():
        out[f"p32_{k}"] = er.condense(ps, chunk)
    for decay, kept in er.RECORDED.items():
        model = torch.nn.Module()
        model.p = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in p32[1] + er.params64(p32[1], p32[2])])
        ema = EMAWeights(model, decay=decay)
        for b in ema.ema_weights:
            b.fill_(float("nan"))
        for k in range(1, max(kept) + 1):
            values = p32[k] + er.params64(p32[k], p32[k % er.N_STEPS + 1])
            with torch.no_grad():
                for p, v in zip(model.parameters(), values):
                    p.copy_(v)
            ema.update_parameters(model)
            if k in kept:
                bufs = ema.ema_weights
                out[f"ema32_{er.tag(decay)}_{k}"] = er.condense(bufs[:7], chunk)
                out[f"ema64_{er.tag(decay)}_{k}"] = er.condense(bufs[7:], chunk)
        if decay == 0.5:
            out["state_keys"] = np.array(list(ema.state_dict().keys()))
            for name, v in ema.get_extra_state().items():
                out[f"extra_{name}"] = np.array(v)
    path = os.path.join(HERE, "ref_ema.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
