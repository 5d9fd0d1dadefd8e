"""``nequip_amd.data.transforms`` and the ``per_edge_type_cutoff`` model metadata, on the CPU.

``NeighborListPruneTransform`` on CPU tensors against ``tests/golden/ref_nl_prune.npz`` (written by
``tests/golden/make_nl_prune_golden.py`` with the reference's own transform): kept mask, pruned ``edge_index`` and the other
per-edge fields, an unregistered field left alone.  ``model.metadata["per_edge_type_cutoff"]`` for partial / nested / asymmetric
dicts against the strings the reference's helper gives (same fixture), the round trip through ``cutoff_str_to_fulldict``, and no
key for a model without a table.
"""

import os

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
PRUNE_CASES = {
    "sym": {"H": {"H": 3.0, "O": 3.5}, "O": {"H": 3.5, "O": 4.5}},
    "asym": {"H": {"H": 3.0, "O": 4.0}, "O": {"H": 3.5}},
}
STRING_CASES = {
    "uniform_rows": ({"H": 3.0}, ["H", "O"], 4.5),
    "nested": ({"H": {"H": 3.0, "O": 3.5}, "O": {"H": 3.5}}, ["H", "O"], 4.5),
    "asymmetric": ({"H": {"O": 4.0, "H": 3.0}, "O": {"H": 3.5, "O": 4.25}}, ["H", "O"], 4.5),
    "three_types": ({"C": 3.25, "O": {"H": 2.0, "C": 3.75}}, ["H", "C", "O"], 5.0),
}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "ref_nl_prune.npz"))


def _data(g):
    from nequip_amd.data import AtomicDataDict as K

    E = g["edge_index"].shape[1]
    return {
        K.POSITIONS_KEY: torch.as_tensor(g["pos"]), K.ATOM_TYPE_KEY: torch.as_tensor(g["types"]),
        K.CELL_KEY: torch.as_tensor(g["cell"]).view(1, 3, 3), K.PBC_KEY: torch.tensor([[True, True, True]]),
        K.EDGE_INDEX_KEY: torch.as_tensor(g["edge_index"]), K.EDGE_CELL_SHIFT_KEY: torch.as_tensor(g["edge_cell_shift"]),
        K.EDGE_ATTRS_KEY: torch.as_tensor(g["edge_attrs"]), "edge_id": torch.arange(E),
    }


@pytest.mark.parametrize("case", sorted(PRUNE_CASES))
def test_prune_transform_matches_the_reference(golden, case):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data.transforms import NeighborListPruneTransform

    t = NeighborListPruneTransform(r_max=float(golden["r_max"]), per_edge_type_cutoff=PRUNE_CASES[case], type_names=["H", "O"])
    data = _data(golden)
    E = data[K.EDGE_INDEX_KEY].shape[1]
    assert np.array_equal(t.keep_mask(data).numpy(), golden[f"{case}_mask"])
    out = t(data)
    assert 0 < out[K.EDGE_INDEX_KEY].shape[1] < E
    assert np.array_equal(out[K.EDGE_INDEX_KEY].numpy(), golden[f"{case}_edge_index"])
    assert np.array_equal(out[K.EDGE_CELL_SHIFT_KEY].numpy(), golden[f"{case}_edge_cell_shift"])
    assert np.array_equal(out[K.EDGE_ATTRS_KEY].numpy(), golden[f"{case}_edge_attrs"])
    assert out["edge_id"].numel() == E  # not a registered per-edge field
    assert out[K.POSITIONS_KEY].shape[0] == golden["pos"].shape[0]


def test_prune_transform_registered_fields_tensor_table_and_errors(golden):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data import register_fields
    from nequip_amd.data.transforms import NeighborListPruneTransform, NeighborListTransform
    from nequip_amd.nn.embedding import cutoff_partialdict_to_tensor

    register_fields(edge_fields=["my_edge_field"])
    table = cutoff_partialdict_to_tensor(PRUNE_CASES["asym"], ["H", "O"], 4.5)
    t = NeighborListPruneTransform(r_max=4.5, per_edge_type_cutoff=table)  # a ready [T, T] table needs no names
    data = _data(golden)
    data["my_edge_field"] = torch.arange(data[K.EDGE_INDEX_KEY].shape[1])
    out = t(data)
    assert np.array_equal(out["my_edge_field"].numpy(), np.nonzero(golden["asym_mask"])[0])
    data = _data(golden)
    del data[K.ATOM_TYPE_KEY]
    with pytest.raises(KeyError, match="atom_types"):
        t(data)
    with pytest.raises(ValueError, match="exceed r_max"):
        NeighborListPruneTransform(r_max=4.0, per_edge_type_cutoff=table)
    with pytest.raises(AssertionError, match="type_names"):
        NeighborListTransform(r_max=4.5, per_edge_type_cutoff={"H": 3.0})
    with pytest.raises(ValueError, match="backend"):
        NeighborListTransform(r_max=4.5, backend="matscipy")(_data(golden))


def _model(type_names, r_max, per_edge_type_cutoff):
    from nequip_amd.model import NequIPGNNModel

    return NequIPGNNModel(seed=0, model_dtype="float32", r_max=r_max, type_names=type_names, num_layers=2, l_max=1,
                          parity=False, num_features=8, radial_mlp_width=16, radial_mlp_depth=1, avg_num_neighbors=10.0,
                          per_edge_type_cutoff=per_edge_type_cutoff)


@pytest.mark.parametrize("case", sorted(STRING_CASES))
def test_model_metadata_carries_the_cutoff_table(golden, case):
    from nequip_amd.data.transforms import cutoff_table_from_model
    from nequip_amd.nn.embedding import cutoff_partialdict_to_tensor, cutoff_str_to_fulldict, cutoff_tensor_to_str

    pt, names, r_max = STRING_CASES[case]
    model = _model(names, r_max, pt)
    text = model.metadata["per_edge_type_cutoff"]
    assert text == str(golden[f"str_{case}"])
    table = cutoff_partialdict_to_tensor(pt, names, r_max)
    assert cutoff_tensor_to_str(table) == text
    full = cutoff_str_to_fulldict(text, names)
    assert set(full) == set(names) and all(set(v) == set(names) for v in full.values())
    assert torch.equal(cutoff_partialdict_to_tensor(full, names, r_max), table)  # round trip
    got = cutoff_table_from_model(model, r_max)
    assert torch.equal(got.table, table) and got.symmetric == bool(torch.equal(table, table.t()))


def test_model_without_table_has_no_key():
    from nequip_amd.data.transforms import cutoff_table_from_model
    from nequip_amd.nn.embedding import cutoff_str_to_fulldict

    model = _model(["H", "O"], 4.5, None)
    assert "per_edge_type_cutoff" not in model.metadata
    assert cutoff_table_from_model(model, 4.5) is None
    assert cutoff_str_to_fulldict("", ["H", "O"]) is None and cutoff_str_to_fulldict(None, ["H", "O"]) is None
    with pytest.raises(ValueError):
        cutoff_str_to_fulldict("1.0 2.0 3.0", ["H", "O"])


def test_converted_model_keeps_publishing_its_table():
    """``enable_NequipAMD_full``'s carry-over on a stand-in for the reference's ``GraphModel`` (a module with a ``_metadata``
    dict): the key is filled in from the converted ``EdgeLengthNormalizer``, never above ``r_max`` (1 / (1 / rc) may round
    up), an existing key is left alone, and a model without a table gets none."""
    from nequip_amd.data.transforms import cutoff_table_from_model
    from nequip_amd.integrations.nequip_full import _carry_cutoff_table
    from nequip_amd.nn.embedding import EdgeLengthNormalizer, cutoff_partialdict_to_tensor

    class Root(torch.nn.Module):
        def __init__(self, norm, metadata):
            super().__init__()
            self.norm = norm
            self._metadata = metadata

        @property
        def metadata(self):
            return dict(self._metadata)

    names = ["H", "C", "O"]
    # cutoffs whose double reciprocal does not round-trip (r_max among them), besides ones that do
    r_max = next(x for x in (4.1 + 0.013 * k for k in range(400)) if 1.0 / (1.0 / x) > x)
    pt = {"H": {"H": 3.0, "O": 0.7 * r_max}, "C": {"H": 3.3}, "O": {"C": 0.49 * r_max}}
    root = Root(EdgeLengthNormalizer(r_max=r_max, type_names=names, per_edge_type_cutoff=pt), {"r_max": str(r_max)})
    _carry_cutoff_table(root)
    values = torch.tensor([float(x) for x in root._metadata["per_edge_type_cutoff"].split()], dtype=torch.float64).view(3, 3)
    assert float(values.max()) <= r_max
    want = cutoff_partialdict_to_tensor(pt, names, r_max)
    torch.testing.assert_close(values, want, rtol=4e-16, atol=0.0)
    table = cutoff_table_from_model(root, r_max)  # (what a calculator does at construction: must not raise)
    assert torch.equal(table.table, values)
    kept = Root(EdgeLengthNormalizer(r_max=4.5, type_names=names, per_edge_type_cutoff={"H": 3.0}),
                {"per_edge_type_cutoff": "1.0 " * 8 + "1.0"})
    _carry_cutoff_table(kept)
    assert kept._metadata["per_edge_type_cutoff"] == "1.0 " * 8 + "1.0"
    none = Root(EdgeLengthNormalizer(r_max=4.5, type_names=names), {})
    _carry_cutoff_table(none)
    assert "per_edge_type_cutoff" not in none._metadata and cutoff_table_from_model(none, 4.5) is None
