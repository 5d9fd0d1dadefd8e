"""Trainable per-type energy scales / shifts (``PerTypeScaleShift(scales_trainable, shifts_trainable)``), the builder
arguments, the ``modify_PerTypeScaleShift`` modifier and the conversion of a reference module, against recordings of the
reference's own module (``tests/golden/make_scale_shift_golden.py`` -> ``ref_scale_shift.npz``)."""
import itertools
import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIELD = "atomic_energy"
INITIAL = {
    "single": dict(scales=1.7, shifts=-0.4),
    "pertype": dict(scales={"A": 1.3, "B": 0.7, "C": 2.1}, shifts={"A": -1.0, "B": 2.0, "C": 0.25}),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "ref_scale_shift.npz"))


def _module(init, s_tr, h_tr, names=("A", "B", "C")):
    from nequip_amd.nn import PerTypeScaleShift

    return PerTypeScaleShift(type_names=list(names), field=FIELD, out_field=FIELD, scales_trainable=s_tr,
                             shifts_trainable=h_tr, irreps_in={FIELD: "0e"}, **INITIAL[init])


@pytest.mark.parametrize("init,s_tr,h_tr", list(itertools.product(INITIAL, (False, True), (False, True))))
def test_module_matches_the_reference_recording(golden, init, s_tr, h_tr):
    from nequip_amd.data import AtomicDataDict

    assert FIELD == AtomicDataDict.PER_ATOM_ENERGY_KEY
    g, tag = golden, f"{init}_s{int(s_tr)}_h{int(h_tr)}"
    mod = _module(init, s_tr, h_tr)
    sd, params = mod.state_dict(), dict(mod.named_parameters())
    assert list(sd.keys()) == list(g[f"{tag}_state_keys"])
    assert list(params.keys()) == list(g[f"{tag}_param_keys"])
    assert isinstance(mod.scales, torch.nn.Parameter) == s_tr and isinstance(mod.shifts, torch.nn.Parameter) == h_tr
    assert [mod.scales_shortcut, mod.shifts_shortcut] == list(g[f"{tag}_shortcuts"])
    assert repr(mod) == str(g[f"{tag}_repr"])
    for k, v in sd.items():
        ref = torch.from_numpy(g[f"{tag}_state_{k}"])
        assert tuple(v.shape) == tuple(ref.shape) and str(v.dtype) == str(g[f"{tag}_dtype_{k}"])
        assert torch.equal(v, ref), k
    types = torch.from_numpy(g["atom_types"])
    x = torch.from_numpy(g["x"]).requires_grad_(True)
    w = torch.from_numpy(g["weights"])
    y = mod({FIELD: x, AtomicDataDict.ATOM_TYPE_KEY: types})[FIELD]
    assert y.dtype == torch.float64
    grads = torch.autograd.grad((y * w).sum(), [x] + list(params.values()))
    torch.testing.assert_close(y.detach(), torch.from_numpy(g[f"{tag}_out"]), rtol=1e-12, atol=0)
    torch.testing.assert_close(grads[0], torch.from_numpy(g[f"{tag}_g_x"]), rtol=1e-12, atol=0)
    assert 2 not in types.tolist()
    for name, gr in zip(params.keys(), grads[1:]):
        ref = torch.from_numpy(g[f"{tag}_g_{name}"])
        assert gr.shape == ref.shape == (3, 1)
        torch.testing.assert_close(gr, ref, rtol=1e-12, atol=0)
        assert float(gr[2].abs()) == 0.0 and float(ref[2].abs()) == 0.0  # the type without an atom
        assert float(gr[:2].abs().min()) > 0.0


def test_constant_tables_are_what_they_were():
    """Both flags off: buffers, single values kept as one entry (the shortcut), no parameters."""
    mod = _module("single", False, False)
    assert list(mod.state_dict()) == ["scales", "shifts"] and not list(mod.parameters())
    assert mod.scales.shape == (1, 1) and mod.shifts.shape == (1, 1) and mod.scales_shortcut and mod.shifts_shortcut
    mod = _module("single", True, False)
    assert mod.scales.shape == (3, 1) and not mod.scales_shortcut and mod.shifts.shape == (1, 1)
    assert torch.equal(mod.scales.detach(), torch.full((3, 1), 1.7, dtype=torch.float64))


def test_lists_are_rejected():
    from nequip_amd.nn import PerTypeScaleShift

    for kw in (dict(scales=[1.0, 2.0, 3.0]), dict(shifts=[1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            PerTypeScaleShift(type_names=["A", "B", "C"], field=FIELD, irreps_in={FIELD: "0e"}, **kw)


# ---- builders ------------------------------------------------------------------------------------------------------------
def _model(**kw):
    from nequip_amd.model import NequIPGNNModel

    args = dict(seed=3, model_dtype="float32", r_max=4.0, type_names=["H", "O"], num_layers=2, l_max=1, parity=False,
                num_features=8, radial_mlp_depth=1, radial_mlp_width=16, avg_num_neighbors=20.0,
                per_type_energy_scales={"H": 1.3, "O": 0.7}, per_type_energy_shifts=-0.5)
    args.update(kw)
    return NequIPGNNModel(**args)


def _tail(model, data):
    """The energy tail of a built model on given last-layer scalars (the convolution stack itself runs on the GPU only)."""
    func = model.model.func
    data = dict(data)
    for name in ("per_atom_energy_readout", "per_type_energy_scale_shift", "total_energy_sum"):
        data = getattr(func, name)(data)
    return data


def _tail_data(n=24, d=8):
    g = torch.Generator().manual_seed(11)
    return {"node_features": torch.randn(n, d, generator=g), "atom_types": torch.randint(0, 2, (n,), generator=g)}


def test_builder_makes_the_tables_parameters():
    model = _model(per_type_energy_scales_trainable=True, per_type_energy_shifts_trainable=True, learnable_shift=True)
    ss = model.model.func.per_type_energy_scale_shift
    assert isinstance(ss.scales, torch.nn.Parameter) and isinstance(ss.shifts, torch.nn.Parameter)
    assert ss.scales.shape == (2, 1) and ss.shifts.shape == (2, 1) and ss.shifts.dtype == torch.float64
    names = dict(model.named_parameters())
    assert "model.func.per_type_energy_scale_shift.scales" in names
    assert "model.func.per_type_energy_scale_shift.shifts" in names
    # learnable_shift: the first layer is built like the others, with its self-connection
    layer0 = model.model.func.layer0_convnet
    assert layer0.conv.use_sc and layer0.conv.sc is not None and "model.func.layer0_convnet.conv.sc.weight" in names
    assert _model().model.func.layer0_convnet.conv.sc is None
    _tail(model, _tail_data())["total_energy"].square().sum().backward()
    assert float(ss.scales.grad.abs().min()) > 0 and float(ss.shifts.grad.abs().min()) > 0


def test_learnable_shift_with_resnet_only_and_without_skip_connections():
    model = _model(learnable_shift=True, convnet_sc=False, convnet_resnet=True)
    assert model.model.func.layer0_convnet.conv.sc is None
    with pytest.raises(AssertionError):
        _model(learnable_shift=True, convnet_sc=False, convnet_resnet=False)


def test_builder_defaults_change_nothing():
    a = _model().state_dict()
    b = _model(per_type_energy_scales_trainable=False, per_type_energy_shifts_trainable=False,
               learnable_shift=False).state_dict()
    assert list(a) == list(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert not any("scale_shift" in k for k, _ in _model().named_parameters())


def test_preset_builder_forwards_the_arguments():
    from nequip_amd.model.nequip_models import PresetNequIPGNNModel

    model = PresetNequIPGNNModel("S", seed=0, r_max=4.0, type_names=["H", "O"], avg_num_neighbors=20.0,
                                 per_type_energy_shifts={"H": 1.0, "O": 2.0}, per_type_energy_shifts_trainable=True, learnable_shift=True)
    assert isinstance(model.model.func.per_type_energy_scale_shift.shifts, torch.nn.Parameter)
    assert model.model.func.layer0_convnet.conv.sc is not None


# ---- modifier ------------------------------------------------------------------------------------------------------------
def test_modifier_matches_the_reference_recording(golden):
    from nequip_amd.nn import PerTypeScaleShift

    model = torch.nn.ModuleDict({"per_type_energy_scale_shift": _module("pertype", False, False)})
    model = PerTypeScaleShift.modify_PerTypeScaleShift(model, scales=0.9, shifts={"B": 7.5}, scales_trainable=False,
                                                       shifts_trainable=True)
    new = model["per_type_energy_scale_shift"]
    assert torch.equal(new.scales.detach(), torch.from_numpy(golden["modify_scales"]))
    assert torch.equal(new.shifts.detach(), torch.from_numpy(golden["modify_shifts"]))
    assert [k for k, _ in new.named_parameters()] == list(golden["modify_param_keys"]) == ["shifts"]
    assert repr(new) == str(golden["modify_repr"])


def test_modifier_on_a_built_model():
    from nequip_amd.model.modify_utils import get_all_modifiers, modify
    from nequip_amd.nn.model_modifier_utils import _MODEL_MODIFIER_PERSISTENT_ATTR_NAME, _MODEL_MODIFIER_PRIVATE_ATTR_NAME

    model = _model()
    fn = get_all_modifiers(model)["modify_PerTypeScaleShift"]
    assert getattr(fn, _MODEL_MODIFIER_PERSISTENT_ATTR_NAME) is True
    assert getattr(fn, _MODEL_MODIFIER_PRIVATE_ATTR_NAME) is False
    data = _tail_data()
    e0 = _tail(model, data)["atomic_energy"].detach()
    old = model.model.func.per_type_energy_scale_shift
    readout = model.model.func.per_atom_energy_readout
    assert readout.__dict__["_scale_shift"][0] is old
    # a partial dict changes the named type only (the single-valued shift is spread over the types first)
    model = modify(model, [dict(modifier="modify_PerTypeScaleShift", shifts={"O": 2.0})])
    new = model.model.func.per_type_energy_scale_shift
    assert new is not old and not list(new.parameters())
    assert new.shifts.view(-1).tolist() == [-0.5, 2.0] and new.scales.view(-1).tolist() == [1.3, 0.7]
    # the cross-module plan points at the module that is in the chain now, and a forward pass of the tail works (the whole
    # model on the GPU, where the fused head reads that plan: tests/test_energy_head_train.py)
    assert readout.__dict__["_scale_shift"][0] is new
    e1 = _tail(model, data)["atomic_energy"].detach()
    is_o = data["atom_types"].view(-1) == 1
    torch.testing.assert_close(e1[is_o], e0[is_o] + 2.5, rtol=1e-12, atol=1e-12)
    assert torch.equal(e1[~is_o], e0[~is_o])
    # one number applies to every type; the trainable flags take effect
    model = modify(model, [dict(modifier="modify_PerTypeScaleShift", scales=2.0, scales_trainable=True,
                                shifts_trainable=True)])
    new = model.model.func.per_type_energy_scale_shift
    assert new.scales.view(-1).tolist() == [2.0, 2.0] and new.shifts.view(-1).tolist() == [-0.5, 2.0]
    assert isinstance(new.scales, torch.nn.Parameter) and isinstance(new.shifts, torch.nn.Parameter)
    assert readout.__dict__["_scale_shift"][0] is new
    _tail(model, data)["total_energy"].sum().backward()
    assert new.shifts.grad is not None and new.scales.grad is not None
    with pytest.raises(AssertionError):
        modify(model, [dict(modifier="modify_PerTypeScaleShift", shifts={"Xe": 1.0})])


# ---- conversion of a reference module -------------------------------------------------------------------------------------
def _reference_shaped(golden, tag):
    """A module shaped like the reference's ``PerTypeScaleShift`` (class name and ``nequip.`` module, the attributes the
    conversion reads), its tables taken from the recording of the reference module."""

    class PerTypeScaleShift(torch.nn.Module):
        pass

    PerTypeScaleShift.__module__ = "nequip.nn.atomwise"
    old = PerTypeScaleShift()
    old.type_names, old.field, old.out_field, old.irreps_in = ["A", "B", "C"], FIELD, FIELD, {FIELD: "0e"}
    old.has_scales = old.has_shifts = True
    params = set(golden[f"{tag}_param_keys"].tolist())
    for name in ("scales", "shifts"):
        table = torch.from_numpy(golden[f"{tag}_state_{name}"]).clone()
        if name in params:
            setattr(old, name, torch.nn.Parameter(table))
        else:
            old.register_buffer(name, table)
    return old


@pytest.mark.parametrize("tag", ["pertype_s1_h1", "single_s0_h1", "pertype_s0_h0", "single_s0_h0"])
def test_conversion_keeps_parameter_tables(golden, tag):
    from nequip_amd import nn as ann
    from nequip_amd.integrations import nequip_full

    old = _reference_shaped(golden, tag)
    model = torch.nn.ModuleDict({"per_type_energy_scale_shift": old})
    keys = list(model.state_dict())
    model = nequip_full.convert(model)
    new = model["per_type_energy_scale_shift"]
    assert type(new) is ann.PerTypeScaleShift and list(model.state_dict()) == keys
    for name in ("scales", "shifts"):
        a, b = getattr(old, name), getattr(new, name)
        assert isinstance(b, torch.nn.Parameter) == isinstance(a, torch.nn.Parameter), name
        assert b.dtype == torch.float64 and torch.equal(a.detach(), b.detach()), name
    assert [k for k, _ in new.named_parameters()] == [k for k, _ in old.named_parameters()]
