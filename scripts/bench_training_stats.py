#!/usr/bin/env python3
"""Cost of the training statistics (``nequip_amd.train.TrainingStatsMonitor``) on the parameter list of the train256 model
(``bench.py``'s training workload: 5 species, l_max 2, 64 features, 3 layers) with gradients and the Adam state of two steps; one
call is ``on_after_backward`` + ``on_before_optimizer_step``:

* ``hip_logging``       the hooks on ``nqa_tstats_reduce`` / ``nqa_tstats_advance`` with ``log_freq = 1``: every call reads every
                        weight, gradient and moment once (2 + 3 launches);
* ``hip_non_logging``   the same launches with a ``log_freq`` that never divides the count: every workgroup returns after
                        reading the counter;
* ``aten_item``         the reference's lines: 13 ATen reductions per parameter, each ending in ``.item()`` (cannot be captured);
* ``aten_no_item``      the same ATen reductions stacked into rows on the device, no host read.

Each is timed eagerly and, where it can be captured, as a replayed hipGraph with device events, in alternating blocks within
one process; kernel launches per call are counted with the profiler in a pass of their own.  Then the whole training step of
``bench.py`` (forward, double backward, Adam) captured as one hipGraph, with and without the monitor's hooks in it
(``log_freq = 1``: every replay logs; both steps zero the gradients in place, so that they keep their addresses), timed the same
way.  Prints one JSON line.

    python scripts/bench_training_stats.py [--blocks 10 --steps 50 --train-steps 20] [--no-train]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--no-train", action="store_true", help="skip the captured training step")
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.train import TrainingStatsMonitor
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_training_stats.py measures on the GPU only"
    device = torch.device("cuda:0")
    w = bench.TRAIN_WORKLOADS["train256"]
    frames = []
    for f in range(w["batch"]):
        pos, types, cell, names = syn.random_frame(w["n_atoms"], w["n_species"], seed=f)
        frames.append(syn.make_data(pos, types, 4.5, cell))
    data = AtomicDataDict.to_device(AtomicDataDict.batched_from_list(frames), device)
    n, e = int(data["pos"].shape[0]), int(data["edge_index"].shape[1])

    def make_model():
        return NequIPGNNModel(
            seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=w["num_layers"], l_max=w["l_max"],
            parity=False, num_features=w["num_features"], radial_mlp_depth=1, radial_mlp_width=128, avg_num_neighbors=e / n,
            per_type_energy_scales=1.0, per_type_energy_shifts=0.0).to(device).train()

    # ---- the hooks alone: parameters, gradients and an Adam state of two steps ---------------------------------------------------
    model = make_model()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
    gen = torch.Generator(device=device).manual_seed(0)
    for _ in range(2):
        for p in model.parameters():
            p.grad = torch.randn(p.shape, generator=gen, device=device, dtype=p.dtype) * 0.1
        opt.step()
    params = [p for p in model.parameters() if p.requires_grad]
    numel = sum(p.numel() for p in params)
    nbytes = sum(p.numel() * p.element_size() for p in params)

    mons = {"hip_logging": TrainingStatsMonitor(log_freq=1), "hip_non_logging": TrainingStatsMonitor(log_freq=1 << 40)}

    def hooks(mon):
        def call():
            mon.on_after_backward(model)
            mon.on_before_optimizer_step(model, [opt])
        return call

    def reference_lines(read):
        """training_stats.py:44-159 of the reference for one optimizer; ``read`` is ``.item()`` or the identity."""
        out = []
        for p in params:
            g = p.grad
            out += [read(g.abs().max()), read(torch.sqrt(torch.mean(g ** 2)))]
        for p in params:
            d = p.data
            a = d.abs()
            out += [read(d.min()), read(d.max()), read(d.mean()), read(d.std()), read(a.min()), read(a.max())]
        for p, state in opt.state.items():
            m, v = state["exp_avg"], state["exp_avg_sq"]
            r = torch.sqrt(v)
            out += [read(m.abs().max()), read(torch.sqrt(torch.mean(m ** 2))), read(r.min()), read(r.max()), read(r.mean())]
        return out

    kept = {}

    def aten_item():
        kept["item"] = reference_lines(lambda t: t.item())

    def aten_no_item():
        kept["no_item"] = torch.stack(reference_lines(lambda t: t))

    variants = {"hip_logging": hooks(mons["hip_logging"]), "hip_non_logging": hooks(mons["hip_non_logging"]),
                "aten_item": aten_item, "aten_no_item": aten_no_item}
    capturable = ("hip_logging", "hip_non_logging", "aten_no_item")

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

    for fn in variants.values():
        fn()  # builds the device tables
    graphs = {k: capture(variants[k]) for k in capturable}  # (all kept alive to the end)
    res = {"workload": "parameter list of the train256 model, gradients, Adam state", "device": torch.cuda.get_device_name(0),
           "parameters": len(params), "elements": numel, "bytes_read_per_logging_call": 4 * nbytes, "blocks": args.blocks,
           "steps_per_block": args.steps, "keys": len(mons["hip_logging"].compute()),
           "hooks_eager": report(alternating(variants, args.steps)),
           "hooks_graph_replay": report(alternating({k: g.replay for k, g in graphs.items()}, args.steps))}
    pairs = list(zip(mons["hip_logging"].compute().values(), kept["item"]))
    assert len(pairs) == len(kept["item"]) == res["keys"]
    res["largest_difference_from_aten"] = max(abs(a - b) for a, b in pairs if a == a and b == b)
    res["logged_steps"] = {k: m.logged_step for k, m in mons.items()}

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

    # ---- the whole captured training step -----------------------------------------------------------------------------------
    if not args.no_train:
        gen = torch.Generator().manual_seed(0)
        f_target = torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device)
        e_target = torch.randn(w["batch"], 1, generator=gen, dtype=torch.float64).to(device)

        def captured_step(with_monitor):
            net = make_model()
            adam = torch.optim.Adam(net.parameters(), lr=1e-2, capturable=True)
            mon = TrainingStatsMonitor(log_freq=1) if with_monitor else None

            def step():  # (the gradients keep their addresses: the monitor's tables are keyed on them)
                adam.zero_grad(set_to_none=False)
                out = net(dict(data))
                loss = (out["forces"] - f_target).square().mean() + (out["total_energy"] - e_target).square().mean()
                loss.backward()
                if mon is not None:
                    mon.on_after_backward(net)
                    mon.on_before_optimizer_step(net, [adam])
                adam.step()

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
                step()
            g.replay()
            torch.cuda.synchronize()
            return g, (net, adam, mon)  # the caller keeps what the replays read and write alive

        steps = {"train_step": captured_step(False), "train_step_with_monitor": captured_step(True)}
        times = alternating({k: v[0].replay for k, v in steps.items()}, args.train_steps)
        res["train_step_graph_replay"] = report(times)
        res["monitor_in_train_step_us"] = round(statistics.median(times["train_step_with_monitor"])
                                                - statistics.median(times["train_step"]), 2)
        mon = steps["train_step_with_monitor"][1][2]
        res["step_count_after"], res["logged_step_after"] = mon.step_count, mon.logged_step
    print(json.dumps(res))


if __name__ == "__main__":
    main()
