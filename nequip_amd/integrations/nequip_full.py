"""``enable_NequipAMD_full``: the WHOLE benchmarked path behind nequip's modifier seam.

``enable_NequipAMD`` (``nequip_extension.py``) swaps one module class, ``TensorProductScatter`` -- the seam the reference itself
offers to OpenEquivariance / cuEquivariance (``nequip/nn/_tp_scatter_base.py:40-109``).  What ``bench.py`` times is more than
that module: the edge embedding in one HIP pass, the radial MLP once per reverse-edge pair, Gate + ``linear_1`` +
self-connection as one launch, the energy head, the force / virial tail.  Those fusions live in the mirrors of the modules
AROUND the tensor product (``nequip_amd.nn``), so a model that nequip's own builders produced (``nequip/model/
nequip_models.py:116-399``) reaches them only if those modules are swapped too.  This modifier does that with the same
machinery: ``replace_submodules`` (``nequip/nn/model_modifier_utils.py:92-107``) per reference class, a factory per class that
rebuilds the mirror from what the reference module keeps as attributes, and the parameters carried over BY NAME (the mirrors
use the reference's parameter / buffer names; e3nn-owned persistent buffers that have no counterpart here are re-attached
under their old names, so ``state_dict()`` keys are the same before and after -- nequip issue #572, the reason
``enable_OpenEquivariance`` keeps ``new.tp = old.tp``).

Reference class (attributes read)                                        -> mirror
    ``NodeTypeEmbed`` (``num_types``, ``set_features``, ``embed_module``, categorical graph-field tables) ``nn.embedding.NodeTypeEmbed``
    ``SphericalHarmonicEdgeAttrs`` (``irreps_edge_sh``, ``out_field``, ``sh.normalize/normalization``)  ``SphericalHarmonicEdgeAttrs``
    ``EdgeLengthNormalizer`` (``r_max``, ``num_types``, ``_per_edge_type``, ``_rmax_recip``, fields)    ``EdgeLengthNormalizer``
    ``BesselEdgeLengthEncoding`` (``num_bessels``, ``trainable``, ``cutoff.p``, fields)             ``BesselEdgeLengthEncoding``
    ``ApplyFactor`` on the edge embedding (``in_field``, ``out_field``, ``factor``)                 folded into the Bessel kernel
    ``ConvNetLayer`` (``irreps_in``, ``feature_irreps_hidden``, ``resnet``, ``equivariant_nonlin``,
        ``conv.{use_sc, is_first_layer, edge_mlp.dims, avg_num_neighbors_norm.norm_const}``)        ``ConvNetLayer`` (+ ``InteractionBlock``)
    ``ScalarMLP`` (``field``, ``out_field``, ``mlp_module.{dims, bias/has_bias, mlp}``)             ``ScalarMLP``
    ``PerTypeScaleShift`` (``type_names``, ``field``, ``out_field``, ``scales``, ``shifts`` and
        whether each is an ``nn.Parameter``)                                                    ``PerTypeScaleShift`` (trainable tables stay Parameters)
    ``ZBL`` (``atomic_numbers``, ``_qqr2exesquare``, ``cutoff.p``, ``per_atom_energy_field``)          ``nn.pair_potential.ZBL``
    ``AtomwiseReduce`` (``field``, ``out_field``, ``reduce``, ``constant``)                         ``AtomwiseReduce``
    ``ForceStressOutput`` (``func``, ``do_derivatives``)                                           ``ForceStressOutput``

e3nn leaves are read through what e3nn 0.5 / 0.6 exposes [RECALLED, e3nn is not installable here]: ``Gate.irreps_scalars /
irreps_gates / irreps_gated``, ``Gate.act_scalars.acts[i].f`` (``Activation`` holding ``normalize2mom`` wrappers),
``NormActivation.scalar_nonlinearity(.f)``, ``SphericalHarmonics.normalize / .normalization``.  The unit test drives nequip's
real builder and modifier code with stand-ins shaped like that.

After the swap the cross-module plan of ``nequip_amd.model.nequip_models._plan_fusions`` is applied to the converted chain
(deferred gates between consecutive ``ConvNetLayer`` s, the fused energy head).  Containers (``SequentialGraphNetwork``,
``GraphModel``) stay the reference's own.
"""

from __future__ import annotations

from typing import Any, Callable, Dict, List, Optional

import torch

from ..data import AtomicDataDict
from ..nn.model_modifier_utils import model_modifier

FULL_MODIFIER_NAME = "enable_NequipAMD_full"


# ---- small readers -----------------------------------------------------------------------------------------------------
def _irreps_dict(d) -> Dict[str, Optional[str]]:
    return {k: (None if v is None else str(v)) for k, v in dict(d).items()}


_ACT_NAMES = {"silu": "silu", "tanh": "tanh", "abs": "abs", "shifted_softplus": "ssp", "ssp": "ssp"}


def _act_name(fn) -> str:
    """Name (key of ``nequip/nn/convnetlayer.py:18-23``'s ``acts``) of an activation as e3nn / nequip hold it."""
    fn = getattr(fn, "f", fn)  # e3nn normalize2mom wrapper
    for ref, name in ((torch.nn.functional.silu, "silu"), (torch.tanh, "tanh"), (torch.abs, "abs")):
        if fn is ref:
            return name
    name = getattr(fn, "__name__", type(fn).__name__).lower()
    if name in _ACT_NAMES:
        return _ACT_NAMES[name]
    raise NotImplementedError(f"{FULL_MODIFIER_NAME}: activation {fn!r} has no counterpart in nequip_amd")


def _acts_of(holder) -> List[Any]:
    """The activation callables of a Gate leg: a plain sequence (nequip_amd's Gate) or e3nn's ``Activation.acts``."""
    if holder is None:
        return []
    seq = getattr(holder, "acts", holder)
    return [a for a in seq if a is not None]


def _gate_kwargs(nonlin) -> Dict[str, Any]:
    """``nonlinearity_type / _scalars / _gates`` of ``ConvNetLayer.__init__`` back from the nonlinearity it built."""
    defaults = {"e": "silu", "o": "tanh"}
    if hasattr(nonlin, "irreps_gated"):  # e3nn Gate
        def leg(irreps, holder):
            out = dict(defaults)
            for (_, ir), act in zip(irreps, _acts_of(holder)):
                out["e" if ir.p == 1 else "o"] = _act_name(act)
            return out

        return dict(nonlinearity_type="gate", nonlinearity_scalars=leg(nonlin.irreps_scalars, nonlin.act_scalars),
                    nonlinearity_gates=leg(nonlin.irreps_gates, nonlin.act_gates))
    act = getattr(nonlin, "scalar_nonlinearity", None)  # e3nn NormActivation
    if act is None:
        raise NotImplementedError(f"{FULL_MODIFIER_NAME}: unknown nonlinearity module {type(nonlin).__name__}")
    scal = dict(defaults)
    scal["e"] = _act_name(act)
    return dict(nonlinearity_type="norm", nonlinearity_scalars=scal, nonlinearity_gates=dict(defaults))


def _mlp_shape(fn) -> Dict[str, Any]:
    """depth / width / nonlinearity / bias of a reference ``ScalarMLPFunction`` (``nequip/nn/mlp.py:81-196``)."""
    dims = list(fn.dims)
    depth = len(dims) - 2
    width = dims[1] if depth > 0 else None
    if depth > 1 and any(d != width for d in dims[1:-1]):
        raise NotImplementedError(f"{FULL_MODIFIER_NAME}: hidden layers of different widths {dims}")
    nonlin = None
    layers = getattr(fn, "mlp", None)
    if depth > 0:
        if type(layers).__name__ == "DeepLinearMLP" or not bool(getattr(fn, "is_nonlinear", True)):
            # nonlinearity=None with hidden layers: the reference evaluates a deep LINEAR net (mlp.py:186-196)
            raise NotImplementedError(f"{FULL_MODIFIER_NAME}: ScalarMLPFunction without a nonlinearity between its "
                                      f"{depth + 1} layers (deep linear net) has no mirror here")
        acts = [m for m in layers if not hasattr(m, "weight") and type(m).__name__ != "ParametrizedScalarLinearLayer"]
        for m in acts:
            n = type(m).__name__.lower()
            if n in ("silu", "tanh", "gelu", "mish", "sigmoid", "softplus"):
                this = n
            elif n == "shiftedsoftplus":
                this = "ssp"
            else:
                # nonlinearity "None" / "null" builds torch.nn.Identity modules with is_nonlinear = True (mlp.py:29-36,176-180):
                # converting that to SiLU would change the function silently
                raise NotImplementedError(f"{FULL_MODIFIER_NAME}: activation module {type(m).__name__} between the layers "
                                          "of a ScalarMLPFunction is not one this package mirrors")
            if nonlin is not None and this != nonlin:
                raise NotImplementedError(f"{FULL_MODIFIER_NAME}: mixed activations {nonlin} / {this} in one ScalarMLPFunction")
            nonlin = this
        if nonlin is None:
            raise NotImplementedError(f"{FULL_MODIFIER_NAME}: no activation module found in a ScalarMLPFunction of depth {depth}")
    has_bias = bool(getattr(fn, "has_bias", False) or (getattr(fn, "bias", False) is True))
    return dict(depth=depth, width=width, nonlinearity=nonlin if nonlin is not None else "silu", bias=has_bias)


def _check_mlp_alphas(new_fn, old_fn, where: str) -> None:
    """The rebuilt layers recompute ``alpha = gain / sqrt(fan_in)`` from the defaults (``forward_weight_init=True``, no
    parametrization): compare with what the reference layers actually carry and refuse on any difference (a model built with
    ``forward_weight_init=False`` or a weight parametrization would otherwise be evaluated with other constants)."""
    def linears(fn):
        return [m for m in fn.mlp if hasattr(m, "weight") and hasattr(m, "alpha")]

    if any("parametrizations" in name for name, _ in old_fn.named_modules()):
        raise NotImplementedError(f"{FULL_MODIFIER_NAME}: {where} uses a weight parametrization")
    a, b = linears(new_fn), linears(old_fn)
    if len(a) != len(b):
        raise RuntimeError(f"{FULL_MODIFIER_NAME}: {where}: {len(b)} reference layers, {len(a)} rebuilt")
    for k, (m_new, m_old) in enumerate(zip(a, b)):
        x, y = float(m_new.alpha), float(m_old.alpha)
        if abs(x - y) > 1e-6 * max(1.0, abs(y)):
            raise NotImplementedError(f"{FULL_MODIFIER_NAME}: {where} layer {k}: reference alpha {y!r}, rebuilt {x!r} "
                                      "(forward_weight_init=False or a non-default gain)")


def _avg_num_neighbors(norm, type_names):
    """``avg_num_neighbors`` back from ``AvgNumNeighborsNorm.norm_const = 1 / sqrt(avg)`` (``nequip/nn/norm.py:26-46``)."""
    c = getattr(norm, "norm_const", None)
    if c is None:
        return None
    c = c.detach().double().reshape(-1)
    avg = (1.0 / (c * c)).tolist()
    if len(avg) == 1:
        return None if abs(avg[0] - 1.0) < 1e-12 else float(avg[0])
    return {name: float(a) for name, a in zip(type_names, avg)}


def _type_names(model, n: int) -> List[str]:
    names = list(getattr(model, "type_names", []) or [])
    if len(names) != n:
        for m in model.modules():
            tn = getattr(m, "type_names", None)
            if tn is not None and len(tn) == n:
                return list(tn)
        names = [f"T{i}" for i in range(n)]  # (names only key per-type dictionaries; the order is what matters)
    return names


def _adopt_state(new: torch.nn.Module, old: torch.nn.Module) -> None:
    """Parameters / buffers by name; what only the old module owned (e3nn bookkeeping buffers) is re-attached under its old
    name so that the state-dict keys do not change."""
    old_sd = old.state_dict()
    res = new.load_state_dict(old_sd, strict=False)
    if res.missing_keys:
        raise RuntimeError(f"{FULL_MODIFIER_NAME}: {type(old).__name__} has no entries for {res.missing_keys}")
    for key in res.unexpected_keys:
        *path, leaf = key.split(".")
        mod = new
        for p in path:
            child = mod._modules.get(p)
            if child is None:
                child = torch.nn.Module()
                mod.add_module(p, child)
            mod = child
        if leaf not in mod._buffers and leaf not in mod._parameters and not hasattr(mod, leaf):
            mod.register_buffer(leaf, old_sd[key].detach().clone())


def _finish(new, old, dtype):
    new.train(old.training)
    dev = next((t.device for t in list(old.parameters()) + list(old.buffers())), None)
    return new.to(dev) if dev is not None else new


# ---- per-class factories -------------------------------------------------------------------------------------------------
def _factories(model) -> Dict[str, Callable]:
    from .. import nn as ann
    from ..nn import embedding as aemb

    model_dtype = getattr(model, "model_dtype", None) or torch.get_default_dtype()

    def under_dtype(fn):
        def wrapped(old):
            prev = torch.get_default_dtype()
            torch.set_default_dtype(model_dtype)
            try:
                new = fn(old)
            finally:
                torch.set_default_dtype(prev)
            _adopt_state(new, old)
            return _finish(new, old, model_dtype)

        return wrapped

    def node_type_embed(old):
        # categorical graph-field embeddings (nequip/nn/embedding/node.py:78-118): one Embedding per field under
        # `categorical_graph_field_embed_modules`, shifted by `categorical_graph_field_embed_shifts[field]` (its `min`)
        fields = None
        if getattr(old, "do_categorical_graph_field_embed", False):
            fields = []
            shifts = dict(getattr(old, "categorical_graph_field_embed_shifts", {}))
            for field, mod in old.categorical_graph_field_embed_modules.items():
                if not isinstance(mod, torch.nn.Embedding) or field not in shifts:
                    raise NotImplementedError(f"{FULL_MODIFIER_NAME}: categorical graph field `{field}` is not an "
                                              f"Embedding with a shift ({type(mod).__name__})")
                fields.append({"field": field, "num_features": mod.embedding_dim, "min": int(shifts[field]),
                               "max": int(shifts[field]) + mod.num_embeddings - 1})
        else:
            for name in ("categorical_graph_field_embed_modules", "categorical_embeds"):
                if len(getattr(old, name, None) or []) > 0:
                    raise NotImplementedError(f"{FULL_MODIFIER_NAME}: `{name}` present but "
                                              f"`do_categorical_graph_field_embed` is not set")
        new = aemb.NodeTypeEmbed(type_names=_type_names(model, old.num_types), num_features=old.embed_module.embedding_dim,
                                 type_embed_init=getattr(old, "type_embed_init", None), set_features=old.set_features,
                                 categorical_graph_field_embed=fields, irreps_in=_irreps_dict(old.irreps_in))
        # every entry of the old state must have a home: nothing is re-attached as an inert buffer here
        extra = sorted(set(old.state_dict()) - set(new.state_dict()))
        if extra:
            raise NotImplementedError(f"{FULL_MODIFIER_NAME}: NodeTypeEmbed entries without a counterpart: {extra}")
        if str(new.irreps_out[AtomicDataDict.NODE_ATTRS_KEY]) != str(old.irreps_out[AtomicDataDict.NODE_ATTRS_KEY]):
            raise RuntimeError(f"{FULL_MODIFIER_NAME}: rebuilt NodeTypeEmbed produces "
                               f"{new.irreps_out[AtomicDataDict.NODE_ATTRS_KEY]}, the reference one "
                               f"{old.irreps_out[AtomicDataDict.NODE_ATTRS_KEY]}")
        return new

    def spharm(old):
        sh = getattr(old, "sh", None)
        return aemb.SphericalHarmonicEdgeAttrs(
            irreps_edge_sh=str(old.irreps_edge_sh), edge_sh_normalization=getattr(sh, "normalization", "component"),
            edge_sh_normalize=bool(getattr(sh, "normalize", True)), irreps_in=_irreps_dict(old.irreps_in),
            out_field=old.out_field)

    def edge_norm(old):
        names = _type_names(model, old.num_types)
        per = None
        if old._per_edge_type:
            cut = old._rmax_recip.detach().double().reciprocal().view(old.num_types, old.num_types)
            per = {a: {b: float(cut[i, j]) for j, b in enumerate(names)} for i, a in enumerate(names)}
        return aemb.EdgeLengthNormalizer(r_max=old.r_max, type_names=names, per_edge_type_cutoff=per,
                                         edge_type_field=old.edge_type_field, norm_length_field=old.norm_length_field,
                                         irreps_in=_irreps_dict(old.irreps_in))

    def bessel(old):
        return aemb.BesselEdgeLengthEncoding(
            cutoff=aemb.PolynomialCutoff(float(old.cutoff.p)), num_bessels=old.num_bessels, trainable=old.trainable,
            edge_invariant_field=old.edge_invariant_field, norm_length_field=old.norm_length_field,
            irreps_in=_irreps_dict(old.irreps_in))

    def apply_factor(old):
        return ann.ApplyFactor(in_field=old.in_field, factor=old.factor, out_field=old.out_field,
                               irreps_in=_irreps_dict(old.irreps_in))

    def convnet(old):
        conv = old.conv
        names = _type_names(model, getattr(conv.avg_num_neighbors_norm, "num_types", 0) or len(getattr(model, "type_names", [])))
        shape = _mlp_shape(conv.edge_mlp)
        kw = dict(radial_mlp_depth=shape["depth"], radial_mlp_width=shape["width"] if shape["width"] is not None else 8,
                  use_sc=bool(conv.use_sc), is_first_layer=bool(conv.is_first_layer), type_names=names,
                  avg_num_neighbors=_avg_num_neighbors(conv.avg_num_neighbors_norm, names))
        new = ann.ConvNetLayer(irreps_in=_irreps_dict(old.irreps_in), feature_irreps_hidden=str(old.feature_irreps_hidden),
                               convolution_kwargs=kw, resnet=bool(old.resnet), **_gate_kwargs(old.equivariant_nonlin))
        _check_mlp_alphas(new.conv.edge_mlp, conv.edge_mlp, "the radial MLP of a ConvNetLayer")
        # the factor itself, not its reconstruction: avg -> 1/sqrt(avg) through the reference's float32 buffer and back is
        # not the identity in the last bit
        old_c, new_norm = getattr(conv.avg_num_neighbors_norm, "norm_const", None), new.conv.avg_num_neighbors_norm
        if old_c is not None and tuple(old_c.shape) == tuple(new_norm.norm_const.shape):
            with torch.no_grad():
                new_norm.norm_const.copy_(old_c.detach().to(new_norm.norm_const.dtype))
            if new_norm.norm_shortcut:
                new_norm.norm_scalar = float(old_c.detach().reshape(-1)[0])
        if str(new.irreps_out[AtomicDataDict.NODE_FEATURES_KEY]) != str(old.irreps_out[AtomicDataDict.NODE_FEATURES_KEY]):
            raise RuntimeError(f"{FULL_MODIFIER_NAME}: rebuilt ConvNetLayer produces "
                               f"{new.irreps_out[AtomicDataDict.NODE_FEATURES_KEY]}, the reference one "
                               f"{old.irreps_out[AtomicDataDict.NODE_FEATURES_KEY]}")
        return new

    def scalar_mlp(old):
        shape = _mlp_shape(old.mlp_module)
        new = ann.ScalarMLP(output_dim=int(old.mlp_module.dims[-1]), hidden_layers_depth=shape["depth"],
                            hidden_layers_width=shape["width"], nonlinearity=shape["nonlinearity"], bias=shape["bias"],
                            field=old.field, out_field=old.out_field, irreps_in=_irreps_dict(old.irreps_in))
        _check_mlp_alphas(new.mlp_module, old.mlp_module, f"ScalarMLP({old.field} -> {old.out_field})")
        return new

    def scale_shift(old):
        def val(t, has):
            if not has:
                return None
            t = t.detach().double().reshape(-1)
            return float(t[0]) if t.numel() == 1 else {n: float(v) for n, v in zip(old.type_names, t.tolist())}

        # a table the reference holds as an nn.Parameter (scales_trainable / shifts_trainable, atomwise.py:205-231) stays one:
        # same name, same [T, 1] values, still seen by the optimiser
        return ann.PerTypeScaleShift(type_names=list(old.type_names), field=old.field, out_field=old.out_field,
                                     scales=val(old.scales, old.has_scales), shifts=val(old.shifts, old.has_shifts),
                                     scales_trainable=old.has_scales and isinstance(old.scales, torch.nn.Parameter),
                                     shifts_trainable=old.has_shifts and isinstance(old.shifts, torch.nn.Parameter),
                                     irreps_in=_irreps_dict(old.irreps_in))

    def zbl(old):
        from ..data.chemistry import chemical_symbols
        from ..nn.pair_potential import _QQR2E, ZBL

        z = [int(round(float(v))) for v in old.atomic_numbers.detach().reshape(-1).tolist()]
        q = float(old._qqr2exesquare)
        # (the buffers themselves are carried over by name below: a rescaled prefactor survives whichever units are named)
        units = next((u for u, v in _QQR2E.items() if abs(v * 0.5 - q) <= 1e-9 * v), "metal")
        return ZBL(type_names=_type_names(model, len(z)), chemical_species=[chemical_symbols[v] for v in z], units=units,
                   polynomial_cutoff_p=float(old.cutoff.p), per_atom_energy_field=old.per_atom_energy_field,
                   irreps_in=_irreps_dict(old.irreps_in))

    def reduce_(old):
        avg = None
        if getattr(old, "constant", 1.0) != 1.0:
            raise NotImplementedError(f"{FULL_MODIFIER_NAME}: AtomwiseReduce with avg_num_atoms normalisation")
        return ann.AtomwiseReduce(irreps_in=_irreps_dict(old.irreps_in), reduce=old.reduce, field=old.field,
                                  out_field=old.out_field)

    def force_stress(old):
        return ann.ForceStressOutput(func=old.func, do_derivatives=bool(old.do_derivatives))

    return {
        "NodeTypeEmbed": under_dtype(node_type_embed),
        "SphericalHarmonicEdgeAttrs": under_dtype(spharm),
        "EdgeLengthNormalizer": under_dtype(edge_norm),
        "BesselEdgeLengthEncoding": under_dtype(bessel),
        "ApplyFactor": under_dtype(apply_factor),
        "ConvNetLayer": under_dtype(convnet),
        "ScalarMLP": under_dtype(scalar_mlp),
        "PerTypeScaleShift": under_dtype(scale_shift),
        "ZBL": under_dtype(zbl),
        "AtomwiseReduce": under_dtype(reduce_),
        "ForceStressOutput": under_dtype(force_stress),
    }


def _is_reference_class(cls, name: str) -> bool:
    return cls.__name__ == name and cls.__module__.split(".")[0] == "nequip"


def _replace(model: torch.nn.Module, name: str, factory: Callable) -> torch.nn.Module:
    """``replace_submodules`` semantics (``nequip/nn/model_modifier_utils.py:92-107``) keyed by reference class NAME (the
    classes themselves are only importable where nequip is)."""
    if _is_reference_class(type(model), name):
        return factory(model)
    for k, child in list(model.named_children()):
        setattr(model, k, _replace(child, name, factory))
    return model


def _plan(model: torch.nn.Module) -> None:
    """Cross-module fusions over every converted sequential chain (``model/nequip_models.py::_plan_fusions``)."""
    from .. import nn as ann
    from ..nn import embedding as aemb

    for seq in [m for m in model.modules() if isinstance(m, torch.nn.Sequential) or hasattr(m, "_modules")]:
        kids = list(seq._modules.values())
        # the 2 pi / r_max^2 factor folds into the Bessel kernel (ApplyFactor then is a no-op: nn/misc.py)
        for a, b in zip(kids, kids[1:]):
            if (isinstance(a, aemb.BesselEdgeLengthEncoding) and isinstance(b, ann.ApplyFactor) and not b._folded
                    and b.in_field == a.edge_invariant_field and b.out_field == b.in_field):
                a.factor = float(a.factor) * float(b.factor)
                b._folded = True
        sph = [m for m in kids if isinstance(m, aemb.SphericalHarmonicEdgeAttrs)]
        nrm = [m for m in kids if isinstance(m, aemb.EdgeLengthNormalizer)]
        bes = [m for m in kids if isinstance(m, aemb.BesselEdgeLengthEncoding)]
        if len(sph) == 1 and len(nrm) == 1 and len(bes) == 1 and kids.index(sph[0]) < kids.index(bes[0]):
            from ..model.nequip_models import _plan_embedding_fusion

            _plan_embedding_fusion(sph[0], nrm[0], bes[0])
        convs = [m for m in kids if isinstance(m, ann.ConvNetLayer)]
        if not convs:
            continue
        for a, b in zip(kids, kids[1:]):
            if isinstance(a, ann.ConvNetLayer) and isinstance(b, ann.ConvNetLayer):
                a.defer_gate = True
            if (isinstance(a, ann.ConvNetLayer) and isinstance(b, ann.ScalarMLP) and b.mlp_module.num_layers == 1
                    and b.field == AtomicDataDict.NODE_FEATURES_KEY):
                nxt = kids[kids.index(b) + 1] if kids.index(b) + 1 < len(kids) else None
                if isinstance(nxt, ann.PerTypeScaleShift):
                    b.__dict__["_scale_shift"] = [nxt]
                    a.defer_gate = True
                    a.__dict__["_gate_consumer"] = [b]
        norms = [m for m in kids if isinstance(m, aemb.EdgeLengthNormalizer)]
        if norms and not norms[0].symmetric:
            for layer in convs:
                layer.conv.paired_radial_ok = False


def convert(model: torch.nn.Module) -> torch.nn.Module:
    """Swap every reference module of the table above for its mirror (in place where the root is a container) and plan
    the cross-module fusions.  Modules of other classes are left alone."""
    for name, factory in _factories(model).items():
        model = _replace(model, name, factory)
    _plan(model)
    _carry_cutoff_table(model)
    return model


def _carry_cutoff_table(model: torch.nn.Module) -> None:
    """A converted model keeps publishing its per-edge-type cutoffs: where the root's metadata (the reference's ``GraphModel``
    keeps a ``_metadata`` dict) does not carry the ``per_edge_type_cutoff`` key, it is filled in from the converted
    ``EdgeLengthNormalizer``, so that this project's calculators prune the neighbour list of such a model too."""
    from ..nn import embedding as aemb
    from ..nn.embedding import cutoff_tensor_to_str

    meta = getattr(model, "_metadata", None)
    if not isinstance(meta, dict) or meta.get("per_edge_type_cutoff"):
        return
    for m in model.modules():
        if isinstance(m, aemb.EdgeLengthNormalizer) and m._per_edge_type:
            # (1 / (1 / rc) may land an ulp above r_max, which the calculators' table check would refuse)
            table = m._rmax_recip.detach().to("cpu", torch.float64).reciprocal().clamp(max=float(m.r_max))
            meta["per_edge_type_cutoff"] = cutoff_tensor_to_str(table)
            return


def make_full_modifier(base_cls):
    """The ``enable_NequipAMD_full`` classmethod for ``base_cls`` (nequip's ``ConvNetLayer``)."""

    def enable_NequipAMD_full(cls, model):
        """Replace the modules of the NequIP message-passing path by their MI355X-native (gfx950 HIP) mirrors."""
        if not torch.cuda.is_available() or torch.version.hip is None:
            raise RuntimeError(f"{FULL_MODIFIER_NAME} requires a ROCm build of PyTorch and an AMD GPU")
        return convert(model)

    # eager inference / training only: the compiled (AOTInductor) deployment takes `enable_NequipAMD` on the compile graph
    # model or nequip_amd's own export (utils/aot.py); no TorchScript / train-time-compile form
    return model_modifier(persistent=False, private=False, unsupported_devices=["cpu"], supported_compile_modes=[])(
        classmethod(enable_NequipAMD_full))


def register_full(base_cls=None):
    """Attach ``enable_NequipAMD_full`` to nequip's ``ConvNetLayer`` (or to ``base_cls`` for tests)."""
    if base_cls is None:
        from nequip.nn.convnetlayer import ConvNetLayer as base_cls  # type: ignore
    if not hasattr(base_cls, FULL_MODIFIER_NAME):
        setattr(base_cls, FULL_MODIFIER_NAME, make_full_modifier(base_cls))
    return base_cls
