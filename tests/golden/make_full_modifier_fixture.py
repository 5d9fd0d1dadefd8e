#!/usr/bin/env python3
"""`enable_NequipAMD_full` on models that the REFERENCE's own builder produced, applied by the REFERENCE's own `modify`,
recorded as tests/golden/full_modifier_models.pt.gz for tests/test_reference_full_modifier.py (which runs without the
reference tree).

    NEQUIP_REFERENCE=<mir-group/nequip source tree> python tests/golden/make_full_modifier_fixture.py

nequip is imported from the reference tree.  e3nn is not installable here, so the e3nn classes nequip's modules construct are
served by stand-ins -- functional ones: `e3nn.o3.Irreps / Irrep`, `Linear`, `FullyConnectedTensorProduct`,
`TensorProduct`, `Gate`, `NormActivation` resolve to this package's CPU mirrors (the Gate re-shaped like e3nn's: its
activations sit in `Activation`-like holders of `normalize2mom`-like wrappers), everything else of e3nn / the training stack
to the inert objects of tests/golden/make_reference_golden.py.  What runs is nequip's real code: `nequip.model.NequIPGNNModel`
(`nequip/model/nequip_models.py:116-399` under the `model_builder` wrapper, `nequip/model/utils.py:104-216`), every
`nequip.nn` constructor on the way, modifier discovery and `nequip.model.modify` (`nequip/model/modify_utils.py:35-150`).

Recorded per model shape (`bench`: the hyper-parameters of the model bench.py times, at 8 features; `tutorial`, `options`):
what the reference built (container and chain module paths), what its modifier registry says about the modifier, its
state dict before the conversion (digests), the container module paths after it, the converted chain -- the very nequip_amd objects
the modifier produced, re-seated in this package's `SequentialGraphNetwork` (the reference containers around it cannot be
unpickled without nequip), its parameters of more than STRIP_NUMEL elements replaced by placeholders of the same shape and
dtype (their values are pinned by the digests) -- and the converted model's state dict (digests).  For `bench` also what the conversion helpers read
from the reference's e3nn-shaped Gate / radial MLP / neighbour normalisation, and whether an unknown module survives.
"""

import contextlib
import gzip
import hashlib
import io
import importlib.util
import os
import sys

sys.dont_write_bytecode = True  # (the reference tree is read-only: no __pycache__ in it)
import warnings

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
REFERENCE = os.environ.get("NEQUIP_REFERENCE", "")
FIXTURE = os.path.join(HERE, "full_modifier_models.pt.gz")
STRIP_NUMEL = 64  # parameters larger than this are recorded by name, shape, dtype and digest only

HYPER = dict(seed=3, model_dtype="float32", type_names=["H", "O"], r_max=4.5, num_layers=3, l_max=2, parity=False,
             num_features=8, radial_mlp_width=16, avg_num_neighbors=20.0,
             per_type_energy_scales={"H": 1.5, "O": 0.75}, per_type_energy_shifts={"H": -1.0, "O": -3.0})

OTHER_SHAPES = {
    # configs/tutorial.yaml's hyper-parameters (BASELINE cfg-1): parity irreps, four layers, radial MLP of depth 2 / width 64
    "tutorial": dict(seed=5, model_dtype="float32", type_names=["C", "H", "O"], r_max=5.0, num_layers=4, l_max=1, parity=True,
                     num_features=32, radial_mlp_depth=2, radial_mlp_width=64, avg_num_neighbors=13.0),
    # per-edge-type cutoffs (asymmetric: the reverse-edge pairing must be off), per-type neighbour counts, norm nonlinearity,
    # trainable Bessel roots, no self-connection, resnet update
    "options": dict(seed=7, model_dtype="float32", type_names=["H", "O"], r_max=4.0, num_layers=3, l_max=2, parity=False,
                    num_features=8, radial_mlp_width=16, avg_num_neighbors={"H": 11.0, "O": 23.0},
                    per_edge_type_cutoff={"H": {"H": 3.0, "O": 3.5}, "O": 4.0}, convnet_nonlinearity_type="norm",
                    bessel_trainable=True, convnet_sc=False, convnet_resnet=True,
                    per_type_energy_shifts={"H": 0.5, "O": -0.25}),
}


@contextlib.contextmanager
def reference():
    spec = importlib.util.spec_from_file_location(
        "make_reference_golden", os.path.join(HERE, "make_reference_golden.py"))
    mrg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mrg)

    from nequip_amd.o3 import irreps as my_irreps, modules as my_modules, tensor_product as my_tp

    class _Normalize2Mom(torch.nn.Module):  # e3nn.math.normalize2mom: the wrapped function is `.f`
        def __init__(self, f):
            super().__init__()
            self.f = f

    class _Activation(torch.nn.Module):  # e3nn.nn.Activation: `.acts` holds the wrappers
        def __init__(self, acts):
            super().__init__()
            self.acts = torch.nn.ModuleList([_Normalize2Mom(a) for a in acts])

    class Gate(my_modules.Gate):
        def __init__(self, irreps_scalars, act_scalars, irreps_gates, act_gates, irreps_gated):
            super().__init__(irreps_scalars, act_scalars, irreps_gates, act_gates, irreps_gated)
            self.act_scalars = _Activation(act_scalars)
            self.act_gates = _Activation(act_gates)

    class SphericalHarmonics(torch.nn.Module):
        def __init__(self, irreps_out, normalize, normalization="integral", irreps_in=None):
            super().__init__()
            self.irreps_out, self.normalize, self.normalization = my_irreps.Irreps(str(irreps_out)), normalize, normalization

    class Linear(my_modules.Linear):
        def __init__(self, irreps_in, irreps_out, internal_weights=True, shared_weights=True, **kw):
            super().__init__(irreps_in=irreps_in, irreps_out=irreps_out)

    class TensorProduct(my_tp.TensorProduct):
        def __init__(self, irreps_in1, irreps_in2, irreps_out, instructions, shared_weights=False, internal_weights=False, **kw):
            super().__init__(irreps_in1, irreps_in2, irreps_out, instructions)

    @contextlib.contextmanager
    def isolate_rng(*a, **k):
        state = torch.get_rng_state()
        try:
            yield
        finally:
            torch.set_rng_state(state)

    special = {
        "e3nn.o3._irreps": dict(Irreps=my_irreps.Irreps, Irrep=my_irreps.Irrep),
        "e3nn.o3": dict(Irreps=my_irreps.Irreps, Irrep=my_irreps.Irrep),
        "e3nn.o3._linear": dict(Linear=Linear),
        "e3nn.o3._tensor_product._sub": dict(FullyConnectedTensorProduct=my_modules.FullyConnectedTensorProduct),
        "e3nn.o3._tensor_product._tensor_product": dict(TensorProduct=TensorProduct),
        "e3nn.nn._gate": dict(Gate=Gate),
        "e3nn.nn._normact": dict(NormActivation=my_modules.NormActivation),
        "e3nn.o3._spherical_harmonics": dict(SphericalHarmonics=SphericalHarmonics),
        "e3nn.util.jit": dict(compile_mode=lambda mode: (lambda cls: cls)),
        "lightning.pytorch.utilities.seed": dict(isolate_rng=isolate_rng),
    }

    class Finder(mrg._Finder):
        def exec_module(self, module):
            for k, v in special.get(module.__name__, {}).items():
                setattr(module, k, v)

    finder = Finder()
    for k in [k for k in sys.modules if k == "nequip" or k.startswith("nequip.")]:
        del sys.modules[k]
    sys.meta_path.insert(0, finder)
    sys.path.insert(0, REFERENCE)
    real_filterwarnings = warnings.filterwarnings
    warnings.filterwarnings = lambda action, message="", category=Warning, *a, **k: (
        real_filterwarnings(action, message, category, *a, **k) if isinstance(category, type) else None)
    # nequip's set_global_state switches process-wide torch settings (default dtype float64, TF32 flags): put them back
    saved = (torch.get_default_dtype(), torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32)
    try:
        import nequip.model as nm
        import nequip.model.modify_utils as modify_utils
        import nequip.nn as rnn
        from nequip.utils.global_state import set_global_state

        set_global_state()
        yield dict(model=nm, modify_utils=modify_utils, nn=rnn)
    finally:
        torch.set_default_dtype(saved[0])
        torch.backends.cuda.matmul.allow_tf32, torch.backends.cudnn.allow_tf32 = saved[1], saved[2]
        warnings.filterwarnings = real_filterwarnings
        sys.meta_path[:] = [f for f in sys.meta_path if f is not finder and type(f).__name__ != "_RegisterAfterImport"]
        sys.path.remove(REFERENCE)
        for k in [k for k in sys.modules if k == "nequip" or k.startswith("nequip.") or k.split(".")[0] in mrg._Finder.TOPS]:
            del sys.modules[k]


def tensor_digest(t) -> str:
    """dtype, shape and sha256 of the bytes: equal digests <=> equal tensors (keeps the fixture small)."""
    t = t.detach().cpu().contiguous()
    return f"{t.dtype}|{tuple(t.shape)}|" + hashlib.sha256(t.reshape(-1).view(torch.uint8).numpy().tobytes()).hexdigest()


def strip_parameters(module):
    """Every parameter of more than STRIP_NUMEL elements becomes a stride-0 view of one zero with its shape, dtype and
    requires_grad: the pickle keeps the module tree and the parameter layout, not the bytes (a few KB instead of MB)."""
    for m in module.modules():
        for name, p in list(m._parameters.items()):
            if p is not None and p.numel() > STRIP_NUMEL:
                m._parameters[name] = torch.nn.Parameter(torch.zeros((), dtype=p.dtype).expand(p.shape),
                                                         requires_grad=p.requires_grad)
    return module


def build_reference(ref, hyper):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return ref["model"].NequIPGNNModel(**hyper)


@contextlib.contextmanager
def _on_rocm():  # the modifier refuses CPU-only hosts: pretend a ROCm device is there while `modify` runs
    saved = (torch.cuda.is_available, torch.version.hip)
    torch.cuda.is_available = lambda: True
    torch.version.hip = torch.version.hip or "7.0"
    try:
        yield
    finally:
        torch.cuda.is_available, torch.version.hip = saved


def record(ref, hyper, extras):
    from nequip_amd.integrations import nequip_full
    from nequip_amd.nn import SequentialGraphNetwork

    rec = {"hyper": hyper}
    model = build_reference(ref, hyper)
    chain = model.model.func
    rec["reference"] = {"model": type(model).__module__,
                        "chain": [(n, type(m).__module__) for n, m in chain.named_children()],
                        "conv": type(chain.layer1_convnet.conv).__module__}
    if extras:
        gate = chain.layer1_convnet.equivariant_nonlin
        rec["helpers"] = {
            "gate_e3nn_layout": hasattr(gate.act_scalars, "acts") and hasattr(gate.act_scalars.acts[0], "f"),
            "gate_kwargs": nequip_full._gate_kwargs(gate),
            "mlp_shape": nequip_full._mlp_shape(chain.layer1_convnet.conv.edge_mlp),
            "avg_num_neighbors": nequip_full._avg_num_neighbors(chain.layer1_convnet.conv.avg_num_neighbors_norm,
                                                                list(hyper["type_names"])),
        }

    nequip_full.register_full()  # default target: nequip.nn.convnetlayer.ConvNetLayer
    mmu = sys.modules["nequip.nn.model_modifier_utils"]
    fn = ref["nn"].ConvNetLayer.enable_NequipAMD_full
    rec["modifier"] = {"is_model_modifier": bool(mmu.is_model_modifier(fn)),
                       "is_persistent": bool(mmu.is_persistent_model_modifier(fn)),
                       "unsupported_devices": list(mmu.get_model_modifier_unsupported_devices(fn)),
                       "all_modifiers": sorted(ref["modify_utils"].get_all_modifiers(model))}
    rec["state_before"] = [(k, tensor_digest(v)) for k, v in model.state_dict().items()]
    with _on_rocm():
        converted = ref["modify_utils"].modify(model, [{"modifier": nequip_full.FULL_MODIFIER_NAME}])
    rec["converted"] = {"model": type(converted).__module__, "inner": type(converted.model).__module__,
                        "chain": type(converted.model.func).__module__}
    rec["state_after"] = [(k, tensor_digest(v)) for k, v in converted.state_dict().items()]
    rec["chain"] = strip_parameters(SequentialGraphNetwork(dict(converted.model.func.named_children())))

    if extras:
        class Extra(torch.nn.Module):  # a module the conversion table does not know
            def forward(self, data):
                return data

        model = build_reference(ref, hyper)
        model.model.func.add_module("extra", Extra())
        rec["helpers"]["unknown_module_kept"] = type(nequip_full.convert(model).model.func.extra) is Extra
    return rec


def main():
    if not os.path.isdir(os.path.join(REFERENCE, "nequip")):
        raise SystemExit("set NEQUIP_REFERENCE to a mir-group/nequip source tree")
    with reference() as ref:
        shapes = {"bench": HYPER, **OTHER_SHAPES}
        blob = {name: record(ref, hyper, extras=(name == "bench")) for name, hyper in shapes.items()}
    buf = io.BytesIO()
    torch.save(blob, buf)
    with open(FIXTURE, "wb") as f:
        f.write(gzip.compress(buf.getvalue(), compresslevel=9, mtime=0))
    print("wrote", FIXTURE, os.path.getsize(FIXTURE), "bytes")


def load():
    with gzip.open(FIXTURE, "rb") as f:
        return torch.load(io.BytesIO(f.read()), map_location="cpu", weights_only=False)


if __name__ == "__main__":
    main()
