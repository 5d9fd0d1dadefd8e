"""Typed (per-edge-type cutoff) device neighbour list against what the untyped entry points allow -- the full list followed by
a torch mask -- and what the pruned list buys a model with such cutoffs: energy + forces on the pruned vs the full list, eager
and as a graphed MD step.  Prints one JSON line per case; `--out FILE` also writes them to FILE."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nequip_amd.data import AtomicDataDict as K  # noqa: E402
from nequip_amd.data._nl import as_cutoff_table, compute_neighborlist_  # noqa: E402
from nequip_amd.data.transforms import NeighborListPruneTransform  # noqa: E402
from nequip_amd.utils import synthetic as syn  # noqa: E402

R_MAX = 4.5
NAMES = ["H", "O"]
TABLES = {
    "water": {"H": {"H": 3.0, "O": 3.5}, "O": {"H": 3.5, "O": 4.5}},
    "asym": {"H": {"H": 3.0, "O": 4.0}, "O": {"H": 3.5}},
}


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def _frame(n_side, seed, dev):
    pos, types, cell, names = syn.water_box(n_side, seed=seed)
    assert list(names) == NAMES
    return {K.POSITIONS_KEY: torch.tensor(pos, dtype=torch.float64, device=dev),
            K.ATOM_TYPE_KEY: torch.tensor(types, dtype=torch.long, device=dev),
            K.CELL_KEY: torch.tensor(np.asarray(cell), dtype=torch.float64, device=dev).view(1, 3, 3),
            K.PBC_KEY: torch.tensor([[True, True, True]], device=dev)}


def _batch(frames, dev):
    n = [f[K.POSITIONS_KEY].shape[0] for f in frames]
    out = {k: torch.cat([f[k] for f in frames]) for k in (K.POSITIONS_KEY, K.ATOM_TYPE_KEY, K.CELL_KEY, K.PBC_KEY)}
    out[K.BATCH_KEY] = torch.repeat_interleave(torch.arange(len(frames)), torch.tensor(n)).to(dev)
    out[K.NUM_NODES_KEY] = torch.tensor(n, dtype=torch.long, device=dev)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n-side", type=int, default=15, help="water box of the model evaluation (15: the bench workload)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = []

    def emit(res):
        lines.append(res)
        print(json.dumps(res), flush=True)

    # ---- list build: typed vs untyped + torch mask ----
    cases = {"water_box_8": _frame(8, 0, dev), "256_small_boxes": _batch([_frame(2, s, dev) for s in range(256)], dev)}
    for case, data in cases.items():
        for tname, table in TABLES.items():
            ct = as_cutoff_table(table, NAMES, R_MAX)
            prune = NeighborListPruneTransform(R_MAX, table, NAMES).to(dev)
            res = {"case": f"list_{case}_{tname}", "atoms": int(data[K.POSITIONS_KEY].shape[0])}
            res["untyped_ms"] = _time(lambda: compute_neighborlist_(dict(data), R_MAX), args.warmup, args.reps)
            res["untyped_then_mask_ms"] = _time(lambda: prune(compute_neighborlist_(dict(data), R_MAX)), args.warmup, args.reps)
            res["typed_ms"] = _time(lambda: compute_neighborlist_(dict(data), R_MAX, per_edge_type_cutoff=ct),
                                    args.warmup, args.reps)
            full = compute_neighborlist_(dict(data), R_MAX)
            typed = compute_neighborlist_(dict(data), R_MAX, per_edge_type_cutoff=ct)
            masked = prune(dict(full))
            assert torch.equal(typed[K.EDGE_INDEX_KEY], masked[K.EDGE_INDEX_KEY])
            res["edges_full"], res["edges_typed"] = int(full[K.EDGE_INDEX_KEY].shape[1]), int(typed[K.EDGE_INDEX_KEY].shape[1])
            emit(res)

    # ---- a per-edge-type-cutoff water model on the pruned vs the full list ----
    from nequip_amd.integrations.graphed_step import GraphedStep
    from nequip_amd.model import NequIPGNNModel

    frame = _frame(args.n_side, 0, dev)
    for tname, table in TABLES.items():
        model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=R_MAX, type_names=NAMES, num_layers=3, l_max=2,
                               parity=False, num_features=64, radial_mlp_depth=1, radial_mlp_width=128,
                               avg_num_neighbors=38.0, per_edge_type_cutoff=table).to(dev).eval()
        ct = as_cutoff_table(table, NAMES, R_MAX)
        res = {"case": f"model_water_{args.n_side}_{tname}", "atoms": int(frame[K.POSITIONS_KEY].shape[0])}
        outs = {}
        for mode, tab in (("full", None), ("pruned", ct)):
            def step(tab=tab):
                out = model(compute_neighborlist_(dict(frame), R_MAX, per_edge_type_cutoff=tab))
                return out[K.TOTAL_ENERGY_KEY].detach(), out[K.FORCE_KEY].detach()

            res[f"eager_{mode}_ms"] = _time(step, args.warmup, max(args.reps // 2, 3))
            outs[mode] = step()
            res[f"edges_{mode}"] = int(compute_neighborlist_(dict(frame), R_MAX, per_edge_type_cutoff=tab)[K.EDGE_INDEX_KEY].shape[1])
            g = GraphedStep(model, frame[K.ATOM_TYPE_KEY], frame[K.CELL_KEY][0], (True,) * 3, R_MAX, prune_neighborlist=tab is not None)
            res[f"graphed_{mode}_ms"] = _time(lambda g=g: g(frame[K.POSITIONS_KEY]), args.warmup, args.reps)
            res[f"graphed_edges_{mode}"] = int(g.last_num_edges)
            del g
        res["max_abs_dF"] = float((outs["full"][1] - outs["pruned"][1]).abs().max())
        res["abs_dE"] = float((outs["full"][0] - outs["pruned"][0]).abs().max())
        emit(res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
