#!/usr/bin/env python3
"""Cost of the loss / metrics layer at the train256 shape (32 frames of 256 atoms: energies [32, 1] float64, forces [8192, 3]
float32, stresses [32, 3, 3] float32; float64 targets), forward plus backward w.r.t. the predictions:

* ``EnergyForceLoss`` on the HIP kernels (``nqa_metrics_fwd`` / ``nqa_metrics_bwd``), against the hand-written ATen loss
  expression of ``bench.py``'s training workload and against the package's own ATen form forced onto GPU tensors;
* ``EnergyForceStressMetrics`` with three per-type force terms (15 terms, 4 streams) on the HIP kernels, against its ATen form.

Each variant is timed eagerly (host clock around a block that ends in a device synchronise: what a host-bound eager step pays)
and as a replayed hipGraph (device events: what a captured step pays), in alternating blocks within one process.  Kernel
launches per call are counted with the profiler in a pass of their own.  Prints one JSON line.

    python scripts/bench_metrics.py [--blocks 10 --steps 50]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.train import EnergyForceLoss, EnergyForceStressMetrics, MaximumAbsoluteError, MeanAbsoluteError
    from nequip_amd.train import RootMeanSquaredError

    assert torch.cuda.is_available(), "bench_metrics.py measures on the GPU only"
    device = torch.device("cuda:0")
    w = bench.TRAIN_WORKLOADS["train256"]
    frames, n = w["batch"], w["batch"] * w["n_atoms"]
    names = [f"T{i}" for i in range(w["n_species"])]
    gen = torch.Generator().manual_seed(0)
    preds = {"total_energy": torch.randn(frames, 1, generator=gen, dtype=torch.float64).to(device).requires_grad_(True),
             "forces": torch.randn(n, 3, generator=gen).to(device).requires_grad_(True),
             "stress": torch.randn(frames, 3, 3, generator=gen).to(device).requires_grad_(True),
             "num_atoms": torch.full((frames,), w["n_atoms"], device=device),
             "atom_types": torch.randint(0, w["n_species"], (n,), generator=gen).to(device)}
    target = {"total_energy": torch.randn(frames, 1, generator=gen, dtype=torch.float64).to(device),
              "forces": torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device),
              "stress": torch.randn(frames, 3, 3, generator=gen, dtype=torch.float64).to(device),
              "num_atoms": preds["num_atoms"]}
    leaves = [preds[k] for k in ("total_energy", "forces", "stress")]

    loss = EnergyForceLoss()
    per_type = [{"name": f"forces_{k}_per_type", "field": "forces", "per_type": True, "metric": cls()}
                for k, cls in (("rmse", RootMeanSquaredError), ("mae", MeanAbsoluteError), ("maxabserr", MaximumAbsoluteError))]
    metrics = EnergyForceStressMetrics(type_names=names, extra_metrics=per_type)

    def aten_form(manager):
        plan = manager.__dict__["_plan"]
        return plan.evaluate(manager._streams(preds, target), accumulate=False, force_aten=True)[plan.ws_index]

    def handwritten():  # the `loss = ...` line of bench.py's training workload
        return (preds["forces"] - target["forces"]).square().mean() + (preds["total_energy"] - target["total_energy"]).square().mean()

    variants = {
        "loss_hip": lambda: loss(preds, target)["weighted_sum"],
        "loss_handwritten_aten": handwritten,
        "loss_aten_form": lambda: aten_form(loss),
        "metrics_hip": lambda: metrics(preds, target)["weighted_sum"],
        "metrics_aten_form": lambda: aten_form(metrics),
    }

    def call(fn):
        return torch.autograd.grad(fn(), leaves, allow_unused=True)

    graphs = {}
    for k, fn in variants.items():
        for _ in range(3):
            call(fn)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            call(fn)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            keep = call(fn)
        g.replay()
        torch.cuda.synchronize()
        graphs[k] = (g, keep)

    def eager_ms(fn, k):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(k):
            call(fn)
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
    eager, graph = {k: [] for k in keys}, {k: [] for k in keys}
    for i in range(args.blocks):
        for k in (keys if i % 2 == 0 else keys[::-1]):
            eager[k].append(eager_ms(variants[k], args.steps))
            graph[k].append(graph_ms(graphs[k][0], args.steps))

    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile

        for k, fn in variants.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                call(fn)
                torch.cuda.synchronize()
            launches[k] = sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # the counts are then not measured
        launches = {"error": f"{type(exc).__name__}: {exc}"}

    res = {"workload": "train256 shape: 32 frames x 256 atoms, forward + backward w.r.t. predictions",
           "device": torch.cuda.get_device_name(0), "blocks": args.blocks, "steps_per_block": args.steps,
           "eager_us_per_call": {k: round(statistics.median(v) * 1e3, 1) for k, v in eager.items()},
           "graph_replay_us_per_call": {k: round(statistics.median(v) * 1e3, 1) for k, v in graph.items()},
           "eager_us_min_max": {k: [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)] for k, v in eager.items()},
           "graph_us_min_max": {k: [round(min(v) * 1e3, 1), round(max(v) * 1e3, 1)] for k, v in graph.items()},
           "device_kernels_and_copies_per_call": launches}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
