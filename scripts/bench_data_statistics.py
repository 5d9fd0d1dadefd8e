#!/usr/bin/env python3
"""Cost of one ``CommonDataStatisticsManager.forward`` at the train256 shape (32 frames of 256 atoms, 5 species, the periodic
neighbour list of ``utils/synthetic`` at r_max 4.5; energies [32, 1] float64, forces [8192, 3] float64):

* ``hip``       the manager on the HIP kernels (``nqa_stats_neighbor_counts`` + ``nqa_stats_update``);
* ``aten_form`` the package's own ATen form forced onto GPU tensors;
* ``reference`` the reference's semantics written in ATen on the same GPU: ``tests/stats_restatement.py`` -- one running object
  per entry and type, boolean indexing per type -- with the reference's ``torch.unique`` neighbour count.  Every selection is a
  host synchronisation with a data-dependent shape, so this variant cannot be captured.

Each variant is timed eagerly (host clock around a block that ends in a device synchronise: what a host-bound loop over a
data set pays per batch); ``hip`` and ``aten_form`` also as a replayed hipGraph (device events), in alternating blocks within
one process.  Device kernels per call are counted with the profiler in a pass of their own.  Before anything is timed the three
variants are compared on the batch they are timed on.  Prints one JSON line.

    python scripts/bench_data_statistics.py [--blocks 10 --steps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()

    import torch

    import bench
    import stats_restatement as sr
    from nequip_amd.data import AtomicDataDict, CommonDataStatisticsManager
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_data_statistics.py measures on the GPU only"
    device = torch.device("cuda:0")
    w = bench.TRAIN_WORKLOADS["train256"]
    frames = []
    for f in range(w["batch"]):
        pos, types, cell, names = syn.random_frame(w["n_atoms"], w["n_species"], seed=f)
        frames.append(syn.make_data(pos, types, 4.5, cell))
    data = AtomicDataDict.to_device(AtomicDataDict.batched_from_list(frames), device)
    n, e = data["pos"].shape[0], data["edge_index"].shape[1]
    gen = torch.Generator().manual_seed(0)
    data["forces"] = torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device)
    data["total_energy"] = (-5.0 * w["n_atoms"] + torch.randn(w["batch"], 1, generator=gen, dtype=torch.float64)).to(device)

    hip = CommonDataStatisticsManager(type_names=names)
    aten = CommonDataStatisticsManager(type_names=names)
    entries = [{"name": "num_neighbors_mean", "field": "num_neighbors", "kind": "mean"},
               {"name": "per_type_num_neighbors_mean", "field": "num_neighbors", "kind": "mean", "per_type": True},
               {"name": "per_atom_energy_mean", "field": "per_atom:total_energy", "kind": "mean"},
               {"name": "forces_rms", "field": "forces", "kind": "rms"},
               {"name": "per_type_forces_rms", "field": "forces", "kind": "rms", "per_type": True}]

    def unique_counts(d):  # the reference's NumNeighbors (right while no atom is isolated, as here)
        counts = torch.unique(d["edge_index"][0], sorted=True, return_counts=True)[1]
        return torch.nn.functional.pad(counts, pad=(0, len(d["pos"]) - len(counts))).to(torch.float64)

    sr.num_neighbors = unique_counts

    def aten_form():
        plan = aten.__dict__["_plan"]
        plan.update([aten._stream(f, k, data) for f, k in zip(aten._stream_fields, plan.group_kinds)], force_aten=True)

    variants = {"hip": lambda: hip(data), "aten_form": aten_form, "reference": lambda: sr.evaluate(entries, [data], names)}

    # ---- the three agree on this batch ----
    hip(data)
    aten_form()
    got, mine, ref = hip.compute(), aten.compute(), sr.evaluate(entries, [data], names)
    worst = 0.0
    for other in (mine, ref):
        for k, v in got.items():
            pairs = zip(v.values(), other[k].values()) if isinstance(v, dict) else [(v, other[k])]
            worst = max([worst] + [abs(a - b) / abs(b) for a, b in pairs])
    assert worst < 1e-10, f"the variants disagree: {worst}"

    graphs = {}
    for k in ("hip", "aten_form"):
        fn = variants[k]
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[k] = g

    def eager_ms(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k

    def graph_ms(g, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k

    keys = list(variants)
    eager, graph = {k: [] for k in keys}, {k: [] for k in graphs}
    for k in keys:
        eager_ms(variants[k], 3)
    for i in range(args.blocks):
        for k in (keys if i % 2 == 0 else keys[::-1]):
            eager[k].append(eager_ms(variants[k], args.steps if k != "reference" else max(2, args.steps // 10)))
            if k in graphs:
                graph[k].append(graph_ms(graphs[k], args.steps))

    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile

        for k, fn in variants.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            launches[k] = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # the counts are then not measured
        launches = {"error": f"{type(exc).__name__}: {exc}"}

    res = {"workload": f"train256 shape: {w['batch']} frames x {w['n_atoms']} atoms, {e} edges, one forward of the common "
                       "manager",
           "device": torch.cuda.get_device_name(0), "blocks": args.blocks, "steps_per_block": args.steps,
           "max_relative_difference_between_variants": worst,
           "eager_us_per_call": {k: round(statistics.median(v) * 1e3, 1) for k, v in eager.items()},
           "graph_replay_us_per_call": {k: round(statistics.median(v) * 1e3, 1) for k, v in graph.items()},
           "eager_us_min_max": {k: [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)] for k, v in eager.items()},
           "graph_us_min_max": {k: [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)] for k, v in graph.items()},
           "device_kernels_and_copies_per_call": launches}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
