#!/usr/bin/env python3
"""Categorical graph-field embeddings (charge / spin / dataset) as the REFERENCE builds and evaluates them, recorded as
tests/golden/categorical_fields.pt.gz for tests/test_categorical_fields.py (which runs without the reference tree).

    NEQUIP_REFERENCE=<mir-group/nequip source tree> python tests/golden/make_categorical_fixture.py

The reference is imported as tests/golden/make_full_modifier_fixture.py does it (nequip's real code, e3nn served by this
package's CPU mirrors).  Recorded:

* ``embed``: a reference ``NodeTypeEmbed`` with two fields -- its state dict, ``irreps_in`` / ``irreps_out`` and its
  ``node_attrs`` for a batched input (through ``batch``) and an unbatched one;
* ``errors``: the reference's assertion messages for a missing key, ``max < min`` and a field that is not a graph field;
* ``builder``: ``NequIPGNNModel(..., categorical_graph_field_embed=...)`` -- its state-dict keys and digests, the input
  fields of its ``GraphModel``, and after ``enable_NequipAMD_full`` (the reference's ``modify``) the converted state dict
  and the converted chain itself.
"""

import gzip
import importlib.util
import io
import os
import sys

sys.dont_write_bytecode = True

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))
FIXTURE = os.path.join(HERE, "categorical_fields.pt.gz")

_spec = importlib.util.spec_from_file_location("make_full_modifier_fixture", os.path.join(HERE, "make_full_modifier_fixture.py"))
mff = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mff)

FIELDS = [{"field": "dataset", "num_features": 3, "min": 0, "max": 2},
          {"field": "charge", "num_features": 5, "min": -2, "max": 3}]
HYPER = dict(seed=11, model_dtype="float32", type_names=["H", "O"], r_max=4.5, num_layers=3, l_max=2, parity=False,
             num_features=8, radial_mlp_width=16, avg_num_neighbors=20.0, categorical_graph_field_embed=FIELDS,
             per_type_energy_scales={"H": 1.5, "O": 0.75}, per_type_energy_shifts={"H": -1.0, "O": -3.0})
BAD = {
    "missing": [{"field": "charge", "num_features": 2, "min": 0}],
    "max_lt_min": [{"field": "charge", "num_features": 2, "min": 2, "max": 1}],
    "not_graph_field": [{"field": "forces", "num_features": 2, "min": 0, "max": 1}],
}
BATCHED = {"atom_types": torch.tensor([0, 1, 1, 0, 1, 0]), "batch": torch.tensor([0, 0, 1, 1, 1, 2]),
           "dataset": torch.tensor([[2], [0], [1]]), "charge": torch.tensor([[-2], [3], [0]])}
SINGLE = {"atom_types": torch.tensor([1, 0, 1]), "dataset": torch.tensor([1]), "charge": torch.tensor([-1])}


def main():
    if not os.path.isdir(os.path.join(mff.REFERENCE, "nequip")):
        raise SystemExit("set NEQUIP_REFERENCE to a mir-group/nequip source tree")
    blob = {}
    with mff.reference() as ref:
        from nequip.nn.embedding import NodeTypeEmbed

        torch.manual_seed(0)
        emb = NodeTypeEmbed(type_names=["H", "O"], num_features=4, categorical_graph_field_embed=FIELDS)
        blob["embed"] = {
            "state": {k: v.detach().clone() for k, v in emb.state_dict().items()},
            "irreps_in": {k: (None if v is None else str(v)) for k, v in emb.irreps_in.items()},
            "irreps_out": {k: (None if v is None else str(v)) for k, v in emb.irreps_out.items()},
            "batched": emb(dict(BATCHED))["node_attrs"].detach().clone(),
            "single": emb(dict(SINGLE))["node_attrs"].detach().clone(),
        }
        errors = {}
        for name, spec in BAD.items():
            try:
                NodeTypeEmbed(type_names=["H", "O"], num_features=4, categorical_graph_field_embed=spec)
            except AssertionError as e:
                errors[name] = str(e)
        blob["errors"] = errors

        from nequip_amd.integrations import nequip_full

        model = mff.build_reference(ref, HYPER)
        rec = {"hyper": HYPER, "input_fields": list(model.model_input_fields),
               "state_before": [(k, mff.tensor_digest(v)) for k, v in model.state_dict().items()]}
        nequip_full.register_full()
        with mff._on_rocm():
            converted = ref["modify_utils"].modify(model, [{"modifier": nequip_full.FULL_MODIFIER_NAME}])
        rec["state_after"] = [(k, mff.tensor_digest(v)) for k, v in converted.state_dict().items()]
        from nequip_amd.nn import SequentialGraphNetwork

        rec["chain"] = SequentialGraphNetwork(dict(converted.model.func.named_children()))
        blob["builder"] = rec
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
