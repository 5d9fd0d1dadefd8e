#!/usr/bin/env python3
"""Cost of trainable per-type energy scales / shifts on the training step (train256 shape: 32 frames of 256 atoms, 5 species,
l_max 2, 64 features, 3 layers; forward, double backward, Adam).

The ``bench.py`` training model with ``per_type_energy_scales_trainable / _shifts_trainable`` set, its optimizer step captured
as one hipGraph the way ``bench.py`` captures it -- once with the training energy head (``nqa_energy_head_train_*``, the
default for trainable tables) and once with ``NQA_NO_ENERGY_HEAD=1`` (Gate, readout, ``PerTypeScaleShift`` and their two
backward passes as ATen launches).  Both graphs are built from the same initial weights; their replays are timed with device
events in alternating blocks within one process, so that clock and thermal drift fall on both alike.  ``--constant`` adds the
step of the model with constant tables (the ``bench.py`` train256 model, which stays on the module chain in training).
Prints one JSON line.

    python scripts/bench_scale_shift.py [--blocks 10 --steps 20] [--constant]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def captured_step(model, data, f_target, e_target):
    """``bench.py::train_bench``'s step (one rank, plain ``loss.backward()``) captured as a hipGraph.  Returns the graph and
    what its replays read and write outside the graph's own memory pool (parameters, optimizer state).  The caller keeps
    both alive: entering a later ``torch.cuda.graph`` empties the allocator's cache, which hands freed blocks back to the
    driver, and a replay of this graph would then touch unmapped memory."""
    import torch

    opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)

    def step():
        opt.zero_grad(set_to_none=True)
        out = model(dict(data))
        loss = (out["forces"] - f_target).square().mean() + (out["total_energy"] - e_target).square().mean()
        loss.backward()
        opt.step()
        return loss

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
    graph = torch.cuda.CUDAGraph()
    opt.zero_grad(set_to_none=True)
    with torch.cuda.graph(graph):
        step()
    graph.replay()
    torch.cuda.synchronize()
    return graph, (model, opt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--constant", action="store_true", help="also time the model with constant tables")
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.nn import _energy_head
    from nequip_amd.utils import synthetic as syn

    device = torch.device("cuda:0")
    w = bench.TRAIN_WORKLOADS["train256"]
    frames = []
    for f in range(w["batch"]):
        pos, types, cell, names = syn.random_frame(w["n_atoms"], w["n_species"], seed=f)
        frames.append(syn.make_data(pos, types, 4.5, cell))
    data = AtomicDataDict.to_device(AtomicDataDict.batched_from_list(frames), device)
    n, e = int(data["pos"].shape[0]), int(data["edge_index"].shape[1])
    gen = torch.Generator().manual_seed(0)
    f_target = torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device)
    e_target = torch.randn(w["batch"], 1, generator=gen, dtype=torch.float64).to(device)

    def model(trainable: bool):
        return NequIPGNNModel(
            seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=w["num_layers"], l_max=w["l_max"],
            parity=False, num_features=w["num_features"], radial_mlp_depth=1, radial_mlp_width=128, avg_num_neighbors=e / n,
            per_type_energy_scales=1.0, per_type_energy_shifts=0.0, per_type_energy_scales_trainable=trainable,
            per_type_energy_shifts_trainable=trainable).to(device).train()

    launches = []
    real = _energy_head._launch_train
    _energy_head._launch_train = lambda order, *a: (launches.append(order), real(order, *a))[1]
    graphs = {"head": captured_step(model(True), data, f_target, e_target)}
    assert launches, "the training energy head did not run"
    launches.clear()
    os.environ["NQA_NO_ENERGY_HEAD"] = "1"
    graphs["aten"] = captured_step(model(True), data, f_target, e_target)
    assert not launches, "NQA_NO_ENERGY_HEAD=1 still ran the training energy head"
    del os.environ["NQA_NO_ENERGY_HEAD"]
    if args.constant:
        graphs["constant"] = captured_step(model(False), data, f_target, e_target)
        assert not launches, "constant tables ran the training energy head"

    def timed(g, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k

    keys = list(graphs)
    times = {k: [] for k in keys}
    for k in keys:
        timed(graphs[k][0], 5)
    for i in range(args.blocks):
        for k in (keys if i % 2 == 0 else keys[::-1]):
            times[k].append(timed(graphs[k][0], args.steps))
    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"workload": "train256, trainable per-type scales and shifts", "atoms": n, "edges": e,
           "ms_step_training_head": round(med["head"], 4), "ms_step_aten_chain": round(med["aten"], 4),
           "saved_us": round((med["aten"] - med["head"]) * 1e3, 1),
           "blocks_ms": {k: [round(t, 4) for t in v] for k, v in times.items()}}
    if args.constant:
        res["ms_step_constant_tables"] = round(med["constant"], 4)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
