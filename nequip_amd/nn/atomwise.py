"""Per-atom readout helpers (mirror of ``nequip/nn/atomwise.py:62-378``): ``AtomwiseReduce`` (per-frame energy sum)
and ``PerTypeScaleShift`` (float64 scale/shift, constant or trainable tables, ``modify_PerTypeScaleShift``).  O(N) elementwise work, outside the hot kernels."""

from typing import Dict, List, Optional, Union

import torch

from ..data import AtomicDataDict
from ._graph_mixin import GraphModuleMixin
from .model_modifier_utils import model_modifier, replace_submodules
from .utils import scatter

_GLOBAL_DTYPE = torch.float64


class AtomwiseReduce(GraphModuleMixin, torch.nn.Module):
    def __init__(self, field: str, out_field: Optional[str] = None, reduce="sum", irreps_in={}):
        super().__init__()
        assert reduce == "sum"
        self.reduce = reduce
        self.field = field
        self.out_field = f"{reduce}_{field}" if out_field is None else out_field
        self._init_irreps(
            irreps_in=irreps_in,
            irreps_out=({self.out_field: irreps_in[self.field]} if self.field in irreps_in else {}),
        )

    def forward(self, data: AtomicDataDict.Type) -> AtomicDataDict.Type:
        field = data[self.field]
        if AtomicDataDict.BATCH_KEY in data:
            result = scatter(field, data[AtomicDataDict.BATCH_KEY], dim=0, dim_size=AtomicDataDict.num_frames(data))
        else:
            result = field.sum(dim=0, keepdim=True)
        data[self.out_field] = result
        return data


class PerTypeScaleShift(GraphModuleMixin, torch.nn.Module):
    """``E_atom = shift[type] + scale[type] * E_atom`` in float64.  A single value takes a shortcut (no per-atom lookup); a
    trainable table (``scales_trainable`` / ``shifts_trainable``) is an ``nn.Parameter`` with one entry per type, a single
    initial value repeated for every type (``nequip/nn/atomwise.py:116-234``)."""

    def __init__(self, type_names: List[str], field: str, out_field: Optional[str] = None,
                 scales: Optional[Union[float, Dict[str, float]]] = None,
                 shifts: Optional[Union[float, Dict[str, float]]] = None, scales_trainable: bool = False,
                 shifts_trainable: bool = False, irreps_in={}):
        super().__init__()
        self.type_names = type_names
        self.num_types = len(type_names)
        self.field = field
        self.out_field = field if out_field is None else out_field
        self._init_irreps(irreps_in=irreps_in, my_irreps_in={self.field: "0e"},
                          irreps_out={self.out_field: irreps_in[self.field]})
        self.out_dtype = _GLOBAL_DTYPE
        if isinstance(scales, list) or isinstance(shifts, list):
            raise ValueError("per-type scales / shifts as lists are not supported: give one number, or a dict keyed by the "
                             "model's type names, e.g. per_type_energy_shifts: {C: 1.0, H: 2.0, O: 3.0}")

        def prep(v, trainable: bool):
            if v is None:
                return None
            if isinstance(v, (float, int)):
                v = [v]
            elif isinstance(v, dict):
                assert set(self.type_names) == set(v.keys())
                v = [v[name] for name in self.type_names]
            else:
                raise ValueError("per-type scales/shifts must be a float or a dict keyed by type name")
            t = torch.as_tensor(v, dtype=self.out_dtype)
            if trainable and t.numel() == 1:
                t = torch.ones(self.num_types, dtype=t.dtype) * t  # one trainable entry per type
            assert t.shape == (self.num_types,) or t.numel() == 1
            return t.reshape(-1, 1)

        self.scales_trainable, self.shifts_trainable = scales_trainable, shifts_trainable
        for name, table, trainable in (("scales", prep(scales, scales_trainable), scales_trainable),
                                       ("shifts", prep(shifts, shifts_trainable), shifts_trainable)):
            if table is None:
                self.register_buffer(name, torch.Tensor())
            elif trainable:
                setattr(self, name, torch.nn.Parameter(table))
            else:
                self.register_buffer(name, table)
        self.has_scales = scales is not None
        self.has_shifts = shifts is not None
        self.scales_shortcut = self.scales.numel() == 1
        self.shifts_shortcut = self.shifts.numel() == 1

    def forward(self, data: AtomicDataDict.Type) -> AtomicDataDict.Type:
        scaled_by = data.pop("_nqa_energy_scaled", None)
        if scaled_by is not None and scaled_by != id(self):
            raise RuntimeError("the fused energy head applied the scales / shifts of a PerTypeScaleShift module that is no "
                               "longer the one in the model (module replaced after the model was built): rebuild the model "
                               "or set NQA_NO_ENERGY_HEAD=1")
        if scaled_by is not None:
            # the fused energy head (nn/_energy_head.py) has produced `field` in float64 with this module's scales and
            # shifts applied
            if self.out_field != self.field:
                data[self.out_field] = data[self.field]
            return data
        if not (self.has_scales or self.has_shifts):
            data[self.out_field] = data[self.field].to(self.out_dtype)
            return data
        in_field = data[self.field]
        types = data[AtomicDataDict.ATOM_TYPE_KEY].view(-1)[: in_field.size(0)]
        scales = shifts = None
        if self.has_scales:
            scales = self.scales if self.scales_shortcut else torch.nn.functional.embedding(types, self.scales)
        if self.has_shifts:
            shifts = self.shifts if self.shifts_shortcut else torch.nn.functional.embedding(types, self.shifts)
        in_field = in_field.to(self.out_dtype)
        if self.has_scales and self.has_shifts:
            in_field = torch.addcmul(shifts, scales, in_field)
        else:
            if self.has_scales:
                in_field = scales * in_field
            if self.has_shifts:
                in_field = shifts + in_field
        data[self.out_field] = in_field
        return data

    @model_modifier(persistent=True, private=False)
    @classmethod
    def modify_PerTypeScaleShift(cls, model, scales: Optional[Union[float, Dict[str, float]]] = None,
                                 shifts: Optional[Union[float, Dict[str, float]]] = None, scales_trainable: bool = False,
                                 shifts_trainable: bool = False):
        """New per-type scales / shifts for a built model, e.g. the isolated-atom energies of a fine-tuning dataset
        (``nequip/nn/atomwise.py:286-353``).  A dict may name some of the model's types only: the other types keep their
        values; one number applies to every type; ``None`` keeps the table.  ``*_trainable`` says whether the new tables
        are parameters."""

        def merged(new, vname, old):
            cur = getattr(old, vname).detach().cpu().reshape(-1).tolist()
            if len(cur) != len(old.type_names):
                assert len(cur) == 1
                cur = cur * len(old.type_names)
            table = dict(zip(old.type_names, cur))
            if new is not None:
                if isinstance(new, (float, int)):
                    new = {name: new for name in old.type_names}
                assert isinstance(new, dict)
                assert all(k in old.type_names for k in new), (
                    f"`{vname}` names {list(new)}, the model's types are {list(old.type_names)}")
                table.update(new)
            return table

        def factory(old):
            return cls(type_names=old.type_names, field=old.field, out_field=old.out_field,
                       scales=merged(scales, "scales", old), shifts=merged(shifts, "shifts", old),
                       scales_trainable=scales_trainable, shifts_trainable=shifts_trainable, irreps_in=old.irreps_in)

        model = replace_submodules(model, cls, factory)
        # a readout planned to run the fused energy head holds its scale / shift module in a plain list
        # (model/nequip_models.py::_plan_fusions): point it at the module that is in the chain now
        for parent in model.modules():
            kids = list(parent._modules.values())
            for a, b in zip(kids, kids[1:]):
                if isinstance(b, cls) and "_scale_shift" in getattr(a, "__dict__", {}):
                    a.__dict__["_scale_shift"] = [b]
        return model

    def __repr__(self) -> str:
        return (f"{self.__class__.__name__} \n  scales: {_format_type_vals(self.scales.reshape(-1).tolist(), self.type_names)}"
                f"\n  shifts: {_format_type_vals(self.shifts.reshape(-1).tolist(), self.type_names)}")


def _format_type_vals(vals: List[float], type_names: List[str], element_formatter: str = ".6f") -> str:
    """``[A: 1.000000, B: 2.000000]``; one value for all types: ``[A, B: 1.000000]``; no table: ``[A, B: None]``."""
    names = ", ".join(type_names)
    if not vals:
        return f"[{names}: None]"
    if len(vals) == 1:
        return f"[{names}: {format(vals[0], element_formatter)}]"
    if len(vals) != len(type_names):
        raise ValueError(f"{len(vals)} values for the types {type_names}")
    return "[" + ", ".join(f"{n}: {format(v, element_formatter)}" for n, v in zip(type_names, vals)) + "]"
