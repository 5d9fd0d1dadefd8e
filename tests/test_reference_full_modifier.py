"""`enable_NequipAMD_full` on models that the REFERENCE's own builder produced, applied by the REFERENCE's own `modify`
-- as recorded in tests/golden/full_modifier_models.pt.gz by tests/golden/make_full_modifier_fixture.py, which runs nequip's
real code (`nequip.model.NequIPGNNModel`, every `nequip.nn` constructor on the way, modifier discovery and
`nequip.model.modify`) with e3nn served by this package's CPU mirrors.  The fixture holds the converted chains themselves
(the nequip_amd objects the modifier produced), so what is checked here needs no reference tree: the converted tree is
module for module the one `nequip_amd.model.NequIPGNNModel` builds for the same hyper-parameters (the model bench.py
times), with the reference model's parameters, the same cross-module fusion plan, and an unchanged set of state-dict keys.
"""

import importlib.util
import os

import pytest
import torch

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_full_modifier_fixture", os.path.join(GOLDEN, "make_full_modifier_fixture.py"))
mff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mff)


@pytest.fixture(scope="module")
def recorded():
    return mff.load()


def _native(hyper):
    from nequip_amd.model import NequIPGNNModel

    return NequIPGNNModel(**hyper)


def _check_state(rec, chain):
    """Same state-dict keys in the same order before and after the conversion (nequip issue #572: checkpoints load with
    or without modifiers), the same values, and the recorded chain holds exactly those entries: the same values where the
    recording kept them, the same dtype and shape where it kept a placeholder (parameters of > STRIP_NUMEL elements)."""
    before, after = dict(rec["state_before"]), dict(rec["state_after"])
    assert [k for k, _ in rec["state_after"]] == [k for k, _ in rec["state_before"]]
    assert after == before
    bad = []
    for k, v in chain.state_dict().items():
        want, got = before.get("model.func." + k), mff.tensor_digest(v)
        if v.numel() > mff.STRIP_NUMEL and not any(v.stride()):
            want, got = (want or "").rsplit("|", 1)[0], got.rsplit("|", 1)[0]
        if want != got:
            bad.append(k)
    assert chain.state_dict() and not bad, bad


def test_reference_builder_output_is_all_reference_modules(recorded):
    ref = recorded["bench"]["reference"]
    assert ref["model"] == "nequip.nn.graph_model"
    assert [n for n, _ in ref["chain"]] == [
        "type_embed", "spharm", "edge_norm", "bessel_encode", "factor", "layer0_convnet", "layer1_convnet",
        "layer2_convnet", "per_atom_energy_readout", "per_type_energy_scale_shift", "total_energy_sum"]
    assert all(mod.startswith("nequip.") for _, mod in ref["chain"])
    assert ref["conv"] == "nequip.nn.interaction_block"


def test_full_modifier_through_the_reference_machinery(recorded):
    from nequip_amd.integrations import nequip_full

    rec = recorded["bench"]
    m = rec["modifier"]
    assert m["is_model_modifier"] and m["is_persistent"] is False
    assert m["unsupported_devices"] == ["cpu"]
    assert nequip_full.FULL_MODIFIER_NAME in m["all_modifiers"] and "enable_OpenEquivariance" in m["all_modifiers"]

    # containers stay the reference's, everything on the path is the mirror
    assert rec["converted"] == {"model": "nequip.nn.graph_model", "inner": "nequip_amd.nn.grad_output",
                                "chain": "nequip.nn._graph_mixin"}
    chain = rec["chain"]
    assert all(type(m).__module__.startswith("nequip_amd.") for m in chain.children())
    _check_state(rec, chain)

    # module for module the natively built model (what bench.py times), same fusion plan
    native = _native(rec["hyper"])
    nchain = native.model.func
    assert [n for n, _ in chain.named_children()] == [n for n, _ in nchain.named_children()]
    for (name, a), (_, b) in zip(chain.named_children(), nchain.named_children()):
        assert type(a) is type(b), name
        # (the reference chain also carries the model's input fields -- pos, edge_index, atom_types -- through its irreps)
        assert {k: str(a.irreps_out[k]) for k in b.irreps_out} == {k: str(v) for k, v in b.irreps_out.items()}, name
    for name in ("layer0_convnet", "layer1_convnet", "layer2_convnet"):
        a, b = getattr(chain, name), getattr(nchain, name)
        assert a.defer_gate == b.defer_gate is True
        assert a.resnet == b.resnet
        assert a.conv.use_sc == b.conv.use_sc and a.conv.is_first_layer == b.conv.is_first_layer
        assert a.conv.tp_scatter.tp.weight_numel == b.conv.tp_scatter.tp.weight_numel
        assert str(a.conv.tp_scatter.irreps_mid) == str(b.conv.tp_scatter.irreps_mid)
        assert a.conv.tp_scatter.instructions == b.conv.tp_scatter.instructions
        assert a.equivariant_nonlin._op_key == b.equivariant_nonlin._op_key  # same irreps, activations, normalize2mom constants
        assert torch.equal(a.conv.avg_num_neighbors_norm.norm_const, b.conv.avg_num_neighbors_norm.norm_const)
        assert a.conv.edge_mlp.dims == b.conv.edge_mlp.dims
    assert chain.bessel_encode.factor == nchain.bessel_encode.factor and chain.factor._folded
    assert chain.edge_norm.symmetric and float(chain.edge_norm._rmax_recip) == float(nchain.edge_norm._rmax_recip)
    assert "_scale_shift" in chain.per_atom_energy_readout.__dict__
    assert chain.per_atom_energy_readout.__dict__["_scale_shift"][0] is chain.per_type_energy_scale_shift
    assert torch.equal(chain.per_type_energy_scale_shift.scales, nchain.per_type_energy_scale_shift.scales)
    assert torch.equal(chain.per_type_energy_scale_shift.shifts, nchain.per_type_energy_scale_shift.shifts)

    # and the mirror loads the converted model's parameters one to one (what a GPU evaluation would run with)
    state = {"model.func." + k: v for k, v in chain.state_dict().items()}
    missing, unexpected = native.load_state_dict(state, strict=False)
    assert all(k.endswith("_empty") for k in missing + unexpected), (missing, unexpected)  # (placeholders only)


def test_full_modifier_leaves_other_modules_alone_and_reads_the_e3nn_layout(recorded):
    h = recorded["bench"]["helpers"]
    assert h["gate_e3nn_layout"]  # the e3nn shape, not a list
    assert h["gate_kwargs"] == dict(nonlinearity_type="gate", nonlinearity_scalars={"e": "silu", "o": "tanh"},
                                    nonlinearity_gates={"e": "silu", "o": "tanh"})
    assert h["mlp_shape"] == dict(depth=1, width=16, nonlinearity="silu", bias=False)
    assert h["avg_num_neighbors"] == pytest.approx(20.0)
    assert h["unknown_module_kept"] is True  # a module the table does not know is not touched


@pytest.mark.parametrize("shape", ["options", "tutorial"])
def test_full_modifier_other_model_shapes(recorded, shape):
    """The same check on the tutorial's hyper-parameters and on a model that uses the options outside the benchmarked
    configs (per-edge-type cutoffs, per-type neighbour counts, norm nonlinearity, trainable Bessel roots, no
    self-connection, resnet update): the converted chain equals the natively built one module for module, with the
    reference's parameters."""
    rec = recorded[shape]
    hyper = rec["hyper"]
    assert hyper == mff.OTHER_SHAPES[shape]
    native = _native(hyper)
    _check_state(rec, rec["chain"])
    chain, nchain = rec["chain"], native.model.func
    assert [n for n, _ in chain.named_children()] == [n for n, _ in nchain.named_children()]
    for (name, a), (_, b) in zip(chain.named_children(), nchain.named_children()):
        assert type(a) is type(b), name
        assert {k: str(a.irreps_out[k]) for k in b.irreps_out} == {k: str(v) for k, v in b.irreps_out.items()}, name
        if hasattr(b, "conv"):
            assert a.defer_gate == b.defer_gate and a.resnet == b.resnet, name
            assert type(a.equivariant_nonlin) is type(b.equivariant_nonlin), name
            assert a.conv.use_sc == b.conv.use_sc and a.conv.paired_radial_ok == b.conv.paired_radial_ok, name
            assert a.conv.edge_mlp.dims == b.conv.edge_mlp.dims, name
            assert a.conv.tp_scatter.instructions == b.conv.tp_scatter.instructions, name
            assert torch.equal(a.conv.avg_num_neighbors_norm.norm_const, b.conv.avg_num_neighbors_norm.norm_const), name
    assert chain.edge_norm.symmetric == nchain.edge_norm.symmetric
    assert torch.equal(chain.edge_norm._rmax_recip, nchain.edge_norm._rmax_recip)
    assert chain.bessel_encode.trainable == nchain.bessel_encode.trainable
    assert isinstance(chain.bessel_encode.bessel_weights, torch.nn.Parameter) == hyper.get("bessel_trainable", False)
    assert ("_fuse_radial" in chain.spharm.__dict__) == ("_fuse_radial" in nchain.spharm.__dict__)
    assert ("_scale_shift" in chain.per_atom_energy_readout.__dict__) == ("_scale_shift" in nchain.per_atom_energy_readout.__dict__)
    state = {"model.func." + k: v for k, v in chain.state_dict().items()}
    missing, unexpected = native.load_state_dict(state, strict=False)
    assert all(k.endswith("_empty") for k in missing + unexpected), (missing, unexpected)  # (placeholders only)
