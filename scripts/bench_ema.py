#!/usr/bin/env python3
"""Cost of the weight averaging (``nequip_amd.train.EMAWeights``) on the parameter list of the train256 model (``bench.py``'s
training workload: 5 species, l_max 2, 64 features, 3 layers), one update per call after the warm-up copy:

* ``aten_host_scalar``    the reference's arithmetic: ``torch._foreach_lerp_`` per dtype with the weight as a Python scalar (in
                          a captured graph that scalar is frozen: timed for its cost only, its replays average wrongly);
* ``hip``                 ``nqa_ema_update``: one multi-tensor launch that reads the update count from device memory, and the
                          one-thread launch that advances it;
* ``aten_device_decay``   what ATen offers with the count on the device: the weight formed by scalar-tensor operations, then
                          ``_foreach_sub`` (temporaries), ``_foreach_mul_`` by the weight tensor, ``_foreach_add_``.

Each is timed eagerly and as a replayed hipGraph with device events, in alternating blocks within one process; kernel launches
per call are counted with the profiler in a pass of their own.  Then the whole training step of ``bench.py`` (forward, double
backward, Adam) captured as one hipGraph, with and without the EMA update in it, timed the same way; and
``swap_parameters`` against the reference's copy-swap.  Prints one JSON line.

    python scripts/bench_ema.py [--blocks 10 --steps 50 --train-steps 20] [--no-train]
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
    from nequip_amd.train import EMAWeights
    from nequip_amd.train import ema as ema_mod
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_ema.py measures on the GPU only"
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

    model = make_model()
    params = [p.detach() for p in model.parameters()]
    numel = sum(p.numel() for p in params)
    nbytes = sum(p.numel() * p.element_size() for p in params)
    decay = 0.999

    # ---- the update alone -------------------------------------------------------------------------------------------------
    emas = {k: EMAWeights(model, decay) for k in ("aten_host_scalar", "hip", "aten_device_decay")}
    for m in emas.values():
        m.update_parameters(model)  # the copy; builds the device tables
    host_n = [1]
    dev_n = torch.ones((), dtype=torch.float64, device=device)

    def aten_host_scalar():
        m = emas["aten_host_scalar"]
        ema_mod._aten_update(m.ema_weights, params, host_n[0], decay)
        host_n[0] += 1

    def aten_device_decay():
        bufs = emas["aten_device_decay"].ema_weights
        weight = 1.0 - torch.clamp((1.0 + dev_n) / (10.0 + dev_n), max=decay)
        diff = torch._foreach_sub(params, bufs)
        torch._foreach_mul_(diff, weight.to(torch.float32))
        torch._foreach_add_(bufs, diff)
        dev_n.add_(1.0)

    variants = {"aten_host_scalar": aten_host_scalar, "hip": lambda: emas["hip"].update_parameters(model),
                "aten_device_decay": aten_device_decay}

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
    res = {"workload": "parameter list of the train256 model", "device": torch.cuda.get_device_name(0),
           "parameters": len(params), "elements": numel, "bytes_per_update": 3 * nbytes, "blocks": args.blocks,
           "steps_per_block": args.steps,
           "update_eager": report(alternating(variants, args.steps)),
           "update_graph_replay": report(alternating({k: g.replay for k, g in graphs.items()}, args.steps))}

    # ---- the swap ---------------------------------------------------------------------------------------------------------
    def aten_swap():  # the reference's: a temporary per tensor, three copies
        for b, p in zip(emas["aten_host_scalar"].ema_weights, params):
            tmp = torch.empty_like(b)
            tmp.copy_(b)
            b.copy_(p)
            p.copy_(tmp)

    swaps = {"aten_copy_swap": aten_swap, "hip": lambda: emas["hip"].swap_parameters(model)}
    res["swap_eager"] = report(alternating(swaps, 2 * (args.steps // 2)))  # (an even count: the weights end where they were)
    assert emas["hip"].is_holding_ema_weights

    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile

        for k, fn in {**variants, **{f"swap_{k}": f for k, f in swaps.items()}}.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                if k.startswith("swap_"):
                    fn()
                torch.cuda.synchronize()
            count = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
            launches[k] = count // 2 if k.startswith("swap_") else count
    except Exception as exc:  # the counts are then not measured
        launches = {"error": f"{type(exc).__name__}: {exc}"}
    res["device_kernels_and_copies_per_call"] = launches

    # ---- the whole captured training step -----------------------------------------------------------------------------------
    if not args.no_train:
        gen = torch.Generator().manual_seed(0)
        f_target = torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device)
        e_target = torch.randn(w["batch"], 1, generator=gen, dtype=torch.float64).to(device)

        def captured_step(with_ema):
            net = make_model()
            opt = torch.optim.Adam(net.parameters(), lr=1e-2, capturable=True)
            avg = EMAWeights(net, decay) if with_ema else None

            def step():
                opt.zero_grad(set_to_none=True)
                out = net(dict(data))
                loss = (out["forces"] - f_target).square().mean() + (out["total_energy"] - e_target).square().mean()
                loss.backward()
                opt.step()
                if avg is not None:
                    avg.update_parameters(net)

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
            opt.zero_grad(set_to_none=True)
            with torch.cuda.graph(g):
                step()
            g.replay()
            torch.cuda.synchronize()
            return g, (net, opt, avg)  # the caller keeps what the replays read and write alive

        steps = {"train_step": captured_step(False), "train_step_with_ema": captured_step(True)}
        times = alternating({k: v[0].replay for k, v in steps.items()}, args.train_steps)
        res["train_step_graph_replay"] = report(times)
        res["ema_in_train_step_us"] = round(statistics.median(times["train_step_with_ema"])
                                            - statistics.median(times["train_step"]), 2)
        res["num_updates_after"] = steps["train_step_with_ema"][1][2].num_updates
    print(json.dumps(res))


if __name__ == "__main__":
    main()
