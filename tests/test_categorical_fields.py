"""Categorical graph-field embeddings (charge / spin / dataset: ``categorical_graph_field_embed``) on the host: the
``NodeTypeEmbed`` restatement against what the reference's module does (tests/golden/categorical_fields.pt.gz, recorded by
tests/golden/make_categorical_fixture.py), the builders' state-dict keys, the conversion of a reference-built model,
``GraphModel`` / batching plumbing, and the errors."""

import importlib.util
import os

import pytest
import torch

from nequip_amd.data import AtomicDataDict as K

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
_spec = importlib.util.spec_from_file_location("make_categorical_fixture", os.path.join(GOLDEN, "make_categorical_fixture.py"))
mcf = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mcf)


@pytest.fixture(scope="module")
def recorded():
    return mcf.load()


def _embed(**kw):
    from nequip_amd.nn.embedding import NodeTypeEmbed

    return NodeTypeEmbed(type_names=["H", "O"], num_features=4, **kw)


# ---- NodeTypeEmbed --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sorted(mcf.BAD))
def test_assertion_messages_are_the_reference_ones(recorded, case):
    with pytest.raises(AssertionError) as e:
        _embed(categorical_graph_field_embed=mcf.BAD[case])
    assert str(e.value) == recorded["errors"][case]


def test_error_cases_restated():
    """The cases of the reference's own unit test (tests/unit/nn/test_utils.py:121-150), restated."""
    with pytest.raises(AssertionError, match="missing keys"):
        _embed(categorical_graph_field_embed=[{"field": "charge", "num_features": 2, "min": 0}])
    with pytest.raises(AssertionError, match="`max` must be >= `min`"):
        _embed(categorical_graph_field_embed=[{"field": "charge", "num_features": 2, "min": 3, "max": 2}])
    with pytest.raises(AssertionError, match="is not a graph field"):
        _embed(categorical_graph_field_embed=[{"field": "not_a_graph_field", "num_features": 2, "min": 0, "max": 1}])


@pytest.mark.parametrize("training", [False, True])
def test_state_irreps_and_values_equal_the_reference(recorded, training):
    rec = recorded["embed"]
    m = _embed(categorical_graph_field_embed=mcf.FIELDS).double()  # (the reference ran with float64 as default dtype)
    assert list(m.state_dict()) == list(rec["state"])
    m.load_state_dict(rec["state"])
    # (the reference's mixin adds pos / edge_index / atom_types to every irreps_in: compared here is what the module adds)
    assert m.irreps_in == {"dataset": None, "charge": None}
    assert all(rec["irreps_in"][k] is None for k in m.irreps_in)
    for k in (K.NODE_ATTRS_KEY, K.NODE_FEATURES_KEY):
        assert str(m.irreps_out[k]) == rec["irreps_out"][k]
    assert m.categorical_graph_field_embed_shifts == {"dataset": 0, "charge": -2}
    m.train(training)
    for name, inp in (("batched", mcf.BATCHED), ("single", mcf.SINGLE)):
        out = m(dict(inp))
        assert torch.equal(out[K.NODE_ATTRS_KEY].detach(), rec[name]), name
        assert torch.equal(out[K.NODE_FEATURES_KEY].detach(), rec[name]), name
        assert out[K.NODE_ATTRS_KEY].shape[1] == 4 + 3 + 5


def test_published_tables_reproduce_node_attrs():
    """Single frame: node_attrs == table[types] for the published [T, F_total] table.  Batch: the type table and the per-field
    (row index, table, column) triples rebuild node_attrs column block by column block."""
    m = _embed(categorical_graph_field_embed=mcf.FIELDS).eval()
    out = m(dict(mcf.SINGLE))
    tab = out["_nqa_node_attrs_table"]
    assert tab.shape == (2, 12) and "_nqa_node_attrs_classes" not in out
    assert torch.equal(tab[mcf.SINGLE["atom_types"]], out[K.NODE_ATTRS_KEY])
    out = m(dict(mcf.BATCHED))
    a = out[K.NODE_ATTRS_KEY]
    assert torch.equal(out["_nqa_node_attrs_table"][mcf.BATCHED["atom_types"]], a[:, :4])
    for idx, tb, col in out["_nqa_node_attrs_classes"]:
        assert torch.equal(tb[idx], a[:, col : col + tb.shape[1]])


def test_out_of_range_and_malformed_fields_raise():
    m = _embed(categorical_graph_field_embed=mcf.FIELDS).eval()
    for bad in ({"charge": torch.tensor([4])}, {"charge": torch.tensor([-3])}, {"dataset": torch.tensor([3])}):
        with pytest.raises(IndexError, match="outside"):
            m(dict(mcf.SINGLE, **bad))
    with pytest.raises(IndexError, match="outside"):
        m(dict(mcf.BATCHED, charge=torch.tensor([[0], [4], [0]])))
    with pytest.raises(KeyError, match="charge"):
        m({k: v for k, v in mcf.SINGLE.items() if k != "charge"})
    with pytest.raises(TypeError, match="integers"):
        m(dict(mcf.SINGLE, charge=torch.tensor([1.0])))
    with pytest.raises(ValueError, match="frames"):
        m(dict(mcf.BATCHED, charge=torch.tensor([[0], [1]]), num_atoms=torch.tensor([2, 3, 1])))


def test_register_fields_extends_the_graph_fields():
    from nequip_amd.data import register_fields
    from nequip_amd.data._key_registry import _GRAPH_FIELDS

    with pytest.raises(AssertionError):
        register_fields(graph_fields="fidelity")
    with pytest.raises(AssertionError, match="not a graph field"):
        _embed(categorical_graph_field_embed=[{"field": "fidelity_level", "num_features": 2, "min": 0, "max": 1}])
    try:
        register_fields(graph_fields=["fidelity_level"])
        m = _embed(categorical_graph_field_embed=[{"field": "fidelity_level", "num_features": 2, "min": 0, "max": 1}])
        assert m.irreps_out[K.NODE_ATTRS_KEY].dim == 6
    finally:
        _GRAPH_FIELDS.discard("fidelity_level")


def test_keys_and_batching():
    from nequip_amd.data import AtomicDataDict

    assert (K.DATASET_KEY, K.TOTAL_CHARGE_KEY, K.TOTAL_SPIN_KEY) == ("dataset", "charge", "spin")
    frames = []
    for f, q in enumerate([1, -1, 0]):
        n = 2 + f
        frames.append({K.POSITIONS_KEY: torch.randn(n, 3), K.ATOM_TYPE_KEY: torch.zeros(n, dtype=torch.long),
                       K.EDGE_INDEX_KEY: torch.zeros(2, 0, dtype=torch.long), "charge": torch.tensor([q]),
                       "spin": torch.tensor([[f]])})
    b = AtomicDataDict.batched_from_list(frames)
    assert torch.equal(b["charge"], torch.tensor([[1], [-1], [0]]))
    assert torch.equal(b["spin"], torch.tensor([[0], [1], [2]]))


# ---- builders, GraphModel, conversion -----------------------------------------------------------------------------
def _native(hyper):
    from nequip_amd.model import NequIPGNNModel

    return NequIPGNNModel(**hyper)


def test_builder_state_dict_keys_equal_the_reference(recorded):
    rec = recorded["builder"]
    model = _native(rec["hyper"])
    want = [(k, d) for k, d in rec["state_before"] if not k.endswith("._empty")]  # (the reference GraphModel's placeholder)
    assert list(model.state_dict()) == [k for k, _ in want]
    # same construction order under the same seed: the same parameter values too
    got = {k: mcf.mff.tensor_digest(v) for k, v in model.state_dict().items()}
    assert got == dict(want)
    tab = model.model.func.type_embed.categorical_graph_field_embed_modules
    assert list(tab) == ["dataset", "charge"] and tab["charge"].weight.shape == (6, 5)


def test_preset_and_full_builders_take_the_argument():
    from nequip_amd.model import FullNequIPGNNModel, PresetNequIPGNNModel

    fields = [{"field": "spin", "num_features": 3, "min": 0, "max": 4}]
    m = PresetNequIPGNNModel("S", type_names=["H", "O"], r_max=4.0, avg_num_neighbors=10.0,
                             categorical_graph_field_embed=fields)
    assert "model.func.type_embed.categorical_graph_field_embed_modules.spin.weight" in m.state_dict()
    assert m.model.func.layer1_convnet.conv.sc.irreps_in2.dim == 32 + 3
    m = FullNequIPGNNModel(r_max=4.0, type_names=["H"], radial_mlp_depth=[1, 1], radial_mlp_width=[8, 8],
                           feature_irreps_hidden=["4x0e+4x1o", "4x0e"], irreps_edge_sh="0e+1o", type_embed_num_features=4,
                           avg_num_neighbors=10.0,
                           categorical_graph_field_embed=fields)
    assert "spin" in m.model_input_fields


def test_graph_model_passes_the_fields_through(recorded):
    model = _native(recorded["builder"]["hyper"])
    for f in ("dataset", "charge"):
        assert f in model.model_input_fields
        assert f in recorded["builder"]["input_fields"]
    seen = {}

    class Probe(torch.nn.Module):
        irreps_in, irreps_out = model.model.irreps_in, model.model.irreps_out

        def forward(self, data):
            seen.update(data)
            return data

    model.model = Probe()
    model({K.POSITIONS_KEY: torch.zeros(1, 3), K.ATOM_TYPE_KEY: torch.zeros(1, dtype=torch.long),
           "charge": torch.tensor([1]), "dataset": torch.tensor([0]), "spin": torch.tensor([0])})
    assert "charge" in seen and "dataset" in seen and "spin" not in seen


def test_plain_model_input_fields_unchanged():
    from nequip_amd.model import NequIPGNNModel

    m = NequIPGNNModel(type_names=["H"], r_max=4.0, num_layers=2, num_features=4, avg_num_neighbors=10.0)
    assert not any(f in m.model_input_fields for f in ("charge", "spin", "dataset"))


def test_reference_model_with_fields_converts_with_every_table(recorded):
    rec = recorded["builder"]
    before, after = rec["state_before"], rec["state_after"]
    assert [k for k, _ in after] == [k for k, _ in before] and dict(after) == dict(before)
    chain = rec["chain"]
    emb = chain.type_embed
    assert type(emb).__module__ == "nequip_amd.nn.embedding.node"
    assert emb.do_categorical_graph_field_embed and emb.categorical_graph_field_embed_shifts == {"dataset": 0, "charge": -2}
    # the tables are the Embeddings' parameters, not re-attached buffers
    assert {n for n, _ in emb.named_parameters()} == {"embed_module.weight",
                                                      "categorical_graph_field_embed_modules.dataset.weight",
                                                      "categorical_graph_field_embed_modules.charge.weight"}
    assert not list(emb.named_buffers())
    for k, v in emb.state_dict().items():
        assert mcf.mff.tensor_digest(v) == dict(before)["model.func.type_embed." + k], k
    assert emb.irreps_out[K.NODE_ATTRS_KEY].dim == 8 + 3 + 5
    assert chain.layer1_convnet.conv.sc.irreps_in2.dim == 16
    assert all(type(m).__module__.startswith("nequip_amd.") for m in chain.children())


def test_conversion_refuses_what_it_cannot_represent():
    from nequip_amd.integrations import nequip_full

    class Old(torch.nn.Module):  # shaped like the reference NodeTypeEmbed, with an extra table the port has no slot for
        def __init__(self):
            super().__init__()
            self.num_types, self.set_features = 2, True
            self.embed_module = torch.nn.Embedding(2, 4)
            self.do_categorical_graph_field_embed = True
            self.categorical_graph_field_embed_modules = torch.nn.ModuleDict({"charge": torch.nn.Linear(2, 2)})
            self.categorical_graph_field_embed_shifts = {"charge": 0}
            self.irreps_in, self.irreps_out = {}, {K.NODE_ATTRS_KEY: "4x0e"}

    class Model(torch.nn.Module):
        type_names = ["H", "O"]

    factory = nequip_full._factories(Model())["NodeTypeEmbed"]
    with pytest.raises(NotImplementedError, match="charge"):
        factory(Old())
    old = Old()
    old.do_categorical_graph_field_embed = False  # tables without the flag: never silently dropped
    with pytest.raises(NotImplementedError, match="categorical_graph_field_embed_modules"):
        factory(old)


def test_integrations_refuse_up_front():
    from nequip_amd.integrations.lammps_mliap import NequIPLAMMPSMLIAPWrapper
    from nequip_amd.utils.aot import aot_export_model

    fields = [{"field": "charge", "num_features": 2, "min": -1, "max": 1}]
    from nequip_amd.model import NequIPGNNModel

    model = NequIPGNNModel(type_names=["H"], r_max=4.0, num_layers=2, num_features=4, avg_num_neighbors=10.0,
                           categorical_graph_field_embed=fields)
    with pytest.raises(NotImplementedError, match="categorical_graph_field_embed"):
        NequIPLAMMPSMLIAPWrapper(model)
    with pytest.raises(NotImplementedError, match="categorical_graph_field_embed"):
        aot_export_model(model, {}, "x.nequip.pt2")
