#!/usr/bin/env python3
"""Fixture for tests/test_nl_transforms.py, produced by the REFERENCE's own ``NeighborListPruneTransform``
(nequip/data/transforms/neighborlist.py) and its cutoff-metadata helpers (nequip/nn/embedding/utils.py).

    python tests/golden/make_nl_prune_golden.py     # needs the reference tree; rewrites tests/golden/ref_nl_prune.npz

The reference is imported the way make_reference_golden.py imports it (inert stand-ins for the packages it would pull in).
Only arrays and strings go into the fixture: positions, types, cell, the input list with two more per-edge fields, the kept
mask and the pruned list for a symmetric and an asymmetric table, and the ``per_edge_type_cutoff`` metadata strings of a few
partial dicts.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

from make_reference_golden import _import_reference  # noqa: E402

TYPE_NAMES = ["H", "O"]
R_MAX = 4.5
PRUNE_CASES = {
    "sym": {"H": {"H": 3.0, "O": 3.5}, "O": {"H": 3.5, "O": 4.5}},
    "asym": {"H": {"H": 3.0, "O": 4.0}, "O": {"H": 3.5}},
}
STRING_CASES = {  # name -> (partial dict, type names, r_max)
    "uniform_rows": ({"H": 3.0}, ["H", "O"], 4.5),
    "nested": ({"H": {"H": 3.0, "O": 3.5}, "O": {"H": 3.5}}, ["H", "O"], 4.5),
    "asymmetric": ({"H": {"O": 4.0, "H": 3.0}, "O": {"H": 3.5, "O": 4.25}}, ["H", "O"], 4.5),
    "three_types": ({"C": 3.25, "O": {"H": 2.0, "C": 3.75}}, ["H", "C", "O"], 5.0),
}


def main():
    K = _import_reference()[0]
    from nequip.data.transforms.neighborlist import NeighborListPruneTransform
    from nequip.nn.embedding.utils import cutoff_partialdict_to_str

    from nequip_amd.utils import synthetic as syn

    torch.set_default_dtype(torch.float64)
    pos, types, cell, names = syn.water_box(n_side=2, seed=3)
    assert list(names) == TYPE_NAMES
    edge_index, shifts = syn.neighbor_list(pos, R_MAX, cell, True)
    E = edge_index.shape[1]
    rng = np.random.default_rng(0)
    edge_attrs = rng.standard_normal((E, 4))
    out = {"pos": pos, "types": np.asarray(types, dtype=np.int64), "cell": cell, "r_max": np.float64(R_MAX),
           "edge_index": np.asarray(edge_index, dtype=np.int64), "edge_cell_shift": np.asarray(shifts, dtype=np.float64),
           "edge_attrs": edge_attrs}
    for name, pt in PRUNE_CASES.items():
        data = {
            K.POSITIONS_KEY: torch.as_tensor(pos), K.ATOM_TYPE_KEY: torch.as_tensor(out["types"]),
            K.CELL_KEY: torch.as_tensor(cell).view(1, 3, 3), K.PBC_KEY: torch.tensor([[True, True, True]]),
            K.EDGE_INDEX_KEY: torch.as_tensor(out["edge_index"]), K.EDGE_CELL_SHIFT_KEY: torch.as_tensor(out["edge_cell_shift"]),
            K.EDGE_ATTRS_KEY: torch.as_tensor(edge_attrs),
            "edge_id": torch.arange(E),  # not a registered edge field: left alone by the reference
        }
        pruned = NeighborListPruneTransform(r_max=R_MAX, per_edge_type_cutoff=pt, type_names=TYPE_NAMES)(data)
        kept = pruned[K.EDGE_INDEX_KEY].numpy()
        # the kept mask from the pruned attrs (rows are unique random numbers)
        lookup = {tuple(r): i for i, r in enumerate(edge_attrs)}
        idx = np.array([lookup[tuple(r)] for r in pruned[K.EDGE_ATTRS_KEY].numpy()])
        mask = np.zeros(E, dtype=bool)
        mask[idx] = True
        assert np.array_equal(idx, np.nonzero(mask)[0]) and pruned["edge_id"].numel() == E
        out[f"{name}_mask"] = mask
        out[f"{name}_edge_index"] = kept
        out[f"{name}_edge_cell_shift"] = pruned[K.EDGE_CELL_SHIFT_KEY].numpy()
        out[f"{name}_edge_attrs"] = pruned[K.EDGE_ATTRS_KEY].numpy()
        print(name, E, "->", kept.shape[1])
    for name, (pt, tn, r_max) in STRING_CASES.items():
        out[f"str_{name}"] = np.array(cutoff_partialdict_to_str(pt, tn, r_max))
        print(name, out[f"str_{name}"])
    np.savez_compressed(os.path.join(HERE, "ref_nl_prune.npz"), **out)


if __name__ == "__main__":
    main()
