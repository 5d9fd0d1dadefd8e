#!/usr/bin/env python3
"""Cost of one optimizer step on the parameter list of the train256 model (``bench.py``'s training workload, BASELINE cfg-4:
5 species, l_max 2, 64 features, 3 layers), on gradients that stay in place:

* ``adam_capturable``  ``torch.optim.Adam(capturable=True)``: the optimizer of the captured training steps so far, the baseline;
* ``hip``              ``AdamWScheduleFree.step()``: one multi-tensor launch (``nqa_sfree_step``) that forms the step scalars
                       from the group record in device memory, and the one-thread-per-group launch that advances it;
* ``aten``             this optimizer's own ATen form (``_aten_step``), the ``_foreach`` calls with host scalars (in a captured
                       graph those are frozen: timed for its cost only, its replays step wrongly).

Each is timed eagerly and as a replayed hipGraph with device events, in alternating blocks within one process; kernel launches
per call are counted with the profiler in a pass of their own.  Prints one JSON line.

    python scripts/bench_schedulefree.py [--blocks 10 --steps 50]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

HBM_COPY_TBS = 6.29  # float4 copy rate of the MI355X


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.train import AdamWScheduleFree
    from nequip_amd.train import schedulefree as sf
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_schedulefree.py measures on the GPU only"
    device = torch.device("cuda:0")
    w = bench.TRAIN_WORKLOADS["train256"]
    names = syn.random_frame(w["n_atoms"], w["n_species"], seed=0)[3]
    model = NequIPGNNModel(
        seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=w["num_layers"], l_max=w["l_max"], parity=False,
        num_features=w["num_features"], radial_mlp_depth=1, radial_mlp_width=128, avg_num_neighbors=20.0,
        per_type_energy_scales=1.0, per_type_energy_shifts=0.0).to(device).train()
    gen = torch.Generator().manual_seed(0)
    grads = [(torch.randn(p.shape, generator=gen) * 1e-2).to(device) for p in model.parameters()]

    def parameters():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    numel = sum(g.numel() for g in grads)
    nbytes = sum(g.numel() * g.element_size() for g in grads)

    adam = torch.optim.Adam(parameters(), lr=1e-3, capturable=True)
    hip = AdamWScheduleFree(parameters(), lr=1e-3, warmup_steps=100)
    hip.train()
    aten_params = parameters()
    aten = AdamWScheduleFree(aten_params, lr=1e-3, warmup_steps=100)
    aten.train()
    aten._ensure_state("step")
    aten_rows = [(p, p.grad, aten.state[p]["z"], aten.state[p]["exp_avg_sq"], 0) for p in aten_params]
    aten_group = dict(aten.param_groups[0])

    def aten_step():
        s = sf._step_scalars(aten_group)
        with torch.no_grad():
            sf._aten_step(aten_rows, aten_group, s)
        aten_group.update(k=aten_group["k"] + 1, weight_sum=s["weight_sum"], lr_max=s["lr_max"], scheduled_lr=s["lr_k"])

    variants = {"adam_capturable": adam.step, "hip": hip.step, "aten": aten_step}

    def capture(fn):
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
        return g

    def timed(fn, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k * 1e3  # microseconds

    def alternating(fns, k):
        keys = list(fns)
        times = {key: [] for key in keys}
        for key in keys:
            timed(fns[key], 4)
        for i in range(args.blocks):
            for key in (keys if i % 2 == 0 else keys[::-1]):
                times[key].append(timed(fns[key], k))
        return times

    def report(times):
        return {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2)}
                for k, v in times.items()}

    graphs = {k: capture(fn) for k, fn in variants.items()}  # (all kept alive to the end)
    eager = alternating(variants, args.steps)
    replay = alternating({k: g.replay for k, g in graphs.items()}, args.steps)
    hip_us = statistics.median(replay["hip"])
    res = {"workload": "parameter list of the train256 model", "device": torch.cuda.get_device_name(0),
           "parameters": len(grads), "elements": numel, "bytes_per_step": 7 * nbytes, "blocks": args.blocks,
           "steps_per_block": args.steps, "step_eager": report(eager), "step_graph_replay": report(replay),
           "hip_replay_tb_per_s": round(7 * nbytes / (hip_us * 1e-6) / 1e12, 3),
           "hip_replay_fraction_of_hbm_copy_rate": round(7 * nbytes / (hip_us * 1e-6) / 1e12 / HBM_COPY_TBS, 3),
           "k_after": hip.state_dict()["param_groups"][0]["k"]}

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
    res["device_kernels_and_copies_per_call"] = launches
    print(json.dumps(res))


if __name__ == "__main__":
    main()
