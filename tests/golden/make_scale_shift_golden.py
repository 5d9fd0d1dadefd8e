#!/usr/bin/env python3
"""Golden vectors of ``PerTypeScaleShift`` with constant and trainable tables, produced by the REFERENCE's own module
(``nequip/nn/atomwise.py:116-356``), imported with the stand-ins of ``make_reference_golden.py``.

Three types, 40 atoms, the third type absent from the frame.  For every combination of ``scales_trainable`` /
``shifts_trainable`` and for single-valued and per-type initial values: the state-dict keys, which of them are Parameters,
their shapes and values, ``repr``, the output for a float32 input, and the gradients of a weighted sum of the output w.r.t.
the input and the trainable tables.  Then ``modify_PerTypeScaleShift`` with a partial ``shifts`` dict and a single ``scales``
number on the per-type module: the tables of the replaced module and which of them are Parameters.

    python tests/golden/make_scale_shift_golden.py     # needs the reference tree; rewrites tests/golden/ref_scale_shift.npz
"""

import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_golden as mrg  # noqa: E402

TYPE_NAMES = ["A", "B", "C"]
N_ATOMS = 40
INITIAL = {
    "single": dict(scales=1.7, shifts=-0.4),
    "pertype": dict(scales={"A": 1.3, "B": 0.7, "C": 2.1}, shifts={"A": -1.0, "B": 2.0, "C": 0.25}),
}
MODIFY = dict(scales=0.9, shifts={"B": 7.5}, scales_trainable=False, shifts_trainable=True)


def inputs():
    g = torch.Generator().manual_seed(20261017)
    types = torch.randint(0, 2, (N_ATOMS,), generator=g)  # type C (index 2) has no atom
    x = torch.randn(N_ATOMS, 1, generator=g, dtype=torch.float32)
    w = torch.rand(N_ATOMS, 1, generator=g, dtype=torch.float64) + 0.5
    return types, x, w


def main():
    K = mrg._import_reference()[0]
    from nequip.nn.atomwise import PerTypeScaleShift

    field = K.PER_ATOM_ENERGY_KEY
    types, x, w = inputs()
    out = dict(type_names=np.array(TYPE_NAMES), atom_types=types.numpy(), x=x.numpy(), weights=w.numpy())
    for (init, kw), s_tr, h_tr in itertools.product(INITIAL.items(), (False, True), (False, True)):
        tag = f"{init}_s{int(s_tr)}_h{int(h_tr)}"
        mod = PerTypeScaleShift(type_names=TYPE_NAMES, field=field, out_field=field, scales_trainable=s_tr,
                                shifts_trainable=h_tr, irreps_in={field: "0e"}, **kw)
        sd = mod.state_dict()
        params = dict(mod.named_parameters())
        out[f"{tag}_state_keys"] = np.array(list(sd.keys()))
        out[f"{tag}_param_keys"] = np.array(list(params.keys()), dtype=str)
        out[f"{tag}_repr"] = np.array(repr(mod))
        out[f"{tag}_shortcuts"] = np.array([mod.scales_shortcut, mod.shifts_shortcut])
        for k, v in sd.items():
            out[f"{tag}_state_{k}"] = v.detach().numpy()
            out[f"{tag}_dtype_{k}"] = np.array(str(v.dtype))
        xin = x.clone().requires_grad_(True)
        y = mod({field: xin, K.ATOM_TYPE_KEY: types})[field]
        wrt = [xin] + list(params.values())
        grads = torch.autograd.grad((y * w).sum(), wrt)
        out[f"{tag}_out"] = y.detach().numpy()
        out[f"{tag}_g_x"] = grads[0].numpy()
        for name, g in zip(params.keys(), grads[1:]):
            out[f"{tag}_g_{name}"] = g.numpy()
    # the fine-tuning modifier on the per-type module with constant tables
    model = torch.nn.ModuleDict({"per_type_energy_scale_shift": PerTypeScaleShift(
        type_names=TYPE_NAMES, field=field, out_field=field, irreps_in={field: "0e"}, **INITIAL["pertype"])})
    model = PerTypeScaleShift.modify_PerTypeScaleShift(model, **MODIFY)
    new = model["per_type_energy_scale_shift"]
    out["modify_scales"] = new.scales.detach().numpy()
    out["modify_shifts"] = new.shifts.detach().numpy()
    out["modify_param_keys"] = np.array([k for k, _ in new.named_parameters()], dtype=str)
    out["modify_repr"] = np.array(repr(new))
    np.savez_compressed(os.path.join(HERE, "ref_scale_shift.npz"), **out)
    print("wrote", os.path.join(HERE, "ref_scale_shift.npz"))


if __name__ == "__main__":
    main()
