#!/usr/bin/env python3
"""Cost of categorical graph-field embeddings (``categorical_graph_field_embed``) on two steps, each timed against the same
model without the fields but with a type embedding as wide as
type + field features (so that both networks have the same shapes and only the cost of the fields is measured), as
hipGraph replays in alternating blocks within one process (clock and thermal drift fall on
both alike).  Prints one JSON line.

* ``cfg3``: water10k (BASELINE cfg-3: 10 125 atoms), eval energy + forces, plain vs a ``charge`` + ``spin`` embedding.  One
  frame: the field rows fold into the per-type table, the node kernels are those of the plain model.
* ``train``: a train256-shaped force-matching step (32 random frames of 256 atoms, forward + double backward + Adam), plain
  vs a ``dataset`` field (the frames spread over 4 dataset labels): per layer one more typed self-connection launch per
  field, forward and backward.

    python scripts/bench_categorical.py [--blocks 10 --steps 30] [--only cfg3|train]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

CHARGE_SPIN = [{"field": "charge", "num_features": 8, "min": -2, "max": 2},
               {"field": "spin", "num_features": 8, "min": 0, "max": 4}]
DATASET = [{"field": "dataset", "num_features": 8, "min": 0, "max": 3}]


def capture(step):
    import torch

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = step()
    g.replay()
    torch.cuda.synchronize()
    return g, out


def timed(g, k):
    import torch

    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(k):
        g.replay()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / k


def compare(g_plain, g_field, blocks, steps):
    for _ in range(2):
        timed(g_plain, 5), timed(g_field, 5)
    t_p, t_f = [], []
    for i in range(blocks):
        order = ((g_plain, t_p), (g_field, t_f)) if i % 2 == 0 else ((g_field, t_f), (g_plain, t_p))
        for g, acc in order:
            acc.append(timed(g, steps))
    mp, mf = statistics.median(t_p), statistics.median(t_f)
    return {"ms_plain": round(mp, 4), "ms_fields": round(mf, 4), "added_us": round((mf - mp) * 1e3, 1),
            "added_frac": round((mf - mp) / mp, 4), "blocks_plain_ms": [round(t, 4) for t in t_p],
            "blocks_fields_ms": [round(t, 4) for t in t_f]}


def bench_cfg3(args, device):
    import torch

    import bench
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.model import NequIPGNNModel

    w = bench.WORKLOADS["water10k"]
    data, names = bench.build_box(w)
    n, e = int(data[K.POSITIONS_KEY].shape[0]), int(data[K.EDGE_INDEX_KEY].shape[1])
    cfg = bench.model_cfg(w, e / n)
    data = {k: v.to(device) for k, v in data.items()}
    kw = {k: v for k, v in cfg.items() if k != "model_dtype"}
    width = kw.get("type_embed_num_features", kw["num_features"]) + sum(f["num_features"] for f in CHARGE_SPIN)
    plain = NequIPGNNModel(seed=0, model_dtype="float32", type_names=names,
                           **dict(kw, type_embed_num_features=width)).to(device).eval()
    field = NequIPGNNModel(seed=0, model_dtype="float32", type_names=names, categorical_graph_field_embed=CHARGE_SPIN,
                           **kw).to(device).eval()
    # labels held on the host, as a calculator's transform would set them: validated without a device read
    fdata = dict(data, charge=torch.tensor([1]), spin=torch.tensor([2]))

    def step_of(model, d):
        return lambda: model(dict(d))[K.FORCE_KEY].detach()

    g_p, _ = capture(step_of(plain, data))
    g_f, _ = capture(step_of(field, fdata))
    return {"workload": "water10k", "atoms": n, "edges": e, "fields": "charge+spin", **compare(g_p, g_f, args.blocks,
                                                                                          args.steps)}


def bench_train(args, device):
    import torch

    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.train import SimpleDDPStrategy
    from nequip_amd.utils import synthetic as syn

    frames = []
    for f in range(32):
        pos, types, cell, names = syn.random_frame(256, 5, seed=f)
        d = syn.make_data(pos, types, 4.5, cell)
        d["dataset"] = torch.tensor([f % 4])
        frames.append(d)
    data = AtomicDataDict.to_device(AtomicDataDict.batched_from_list(frames), device)
    n, e = data["pos"].shape[0], data["edge_index"].shape[1]
    gen = torch.Generator().manual_seed(0)
    f_t = torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device)
    e_t = torch.randn(32, 1, generator=gen, dtype=torch.float64).to(device)

    def make(fields):
        width = 64 + (0 if fields else sum(f["num_features"] for f in DATASET))
        model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=3, l_max=2,
                               type_embed_num_features=width,
                               parity=False, num_features=64, radial_mlp_depth=1, radial_mlp_width=128,
                               avg_num_neighbors=e / n, per_type_energy_scales=1.0, per_type_energy_shifts=0.0,
                               categorical_graph_field_embed=fields).to(device).train()
        strategy = SimpleDDPStrategy(model)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)

        def step():
            opt.zero_grad(set_to_none=True)
            out = model(dict(data))
            loss = (out["forces"] - f_t).square().mean() + (out["total_energy"] - e_t).square().mean()
            strategy.backward(loss * strategy.world_size)
            strategy.post_backward(loss)
            opt.step()
            return loss.detach()

        return step

    plain_step, field_step = make(None), make(DATASET)
    # eager once with the host-side label check, then capture (inside the capture the labels are taken as validated)
    field_step()
    g_p, _ = capture(plain_step)
    g_f, _ = capture(field_step)
    return {"workload": "train256x32", "atoms": int(n), "edges": int(e), "fields": "dataset",
            **compare(g_p, g_f, args.blocks, args.steps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--only", choices=["cfg3", "train"], default=None)
    args = ap.parse_args()

    import torch

    device = torch.device("cuda:0")
    res = {}
    if args.only in (None, "cfg3"):
        res["cfg3"] = bench_cfg3(args, device)
    if args.only in (None, "train"):
        res["train"] = bench_train(args, device)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
