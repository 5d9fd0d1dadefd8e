#!/usr/bin/env python3
"""Cost of one optimizer step on the parameter list of the train256 model (``bench.py``'s training workload, BASELINE cfg-4:
5 species, l_max 2, 64 features, 3 layers), on gradients that stay in place:

* ``adam_capturable``  ``torch.optim.Adam(capturable=True)`` in its ``foreach`` form: the optimizer of the captured training
                       steps so far, the baseline;
* ``adam_fused``       ``torch.optim.Adam(capturable=True, fused=True)``, if the installed torch offers it on this device;
* ``hip``              ``nequip_amd.train.Adam.step()``: one multi-tensor launch (``nqa_adam_step``) and the
                       one-thread-per-parameter launch that advances the counts;
* ``hip_clip_norm``    the same with ``gradient_clip_val`` (two more launches: ``nqa_adam_grad_norm``);
* ``hip_amsgrad``      the same with ``amsgrad`` (9 words per element instead of 7);
* ``aten``             this optimizer's own ATen form (``_aten_step``), the ``_foreach`` calls with host scalars (it reads the
                       step counts on the host, so it is timed eagerly only).

Each is timed eagerly and as a replayed hipGraph with device events, in alternating blocks within one process; kernel launches
per call are counted with the profiler in a pass of their own.  Then the whole train256 step (forward, double backward, optimizer)
is captured once with torch's capturable Adam and once with this one and replayed in alternating blocks.  Prints one JSON line
and writes it to ``--out``.

    python scripts/bench_adam.py [--blocks 10 --steps 50 --out profiles/adam_bench.json]
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
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adam_bench.json"))
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.train import Adam
    from nequip_amd.train import adam as ad
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_adam.py measures on the GPU only"
    device = torch.device("cuda:0")
    w = bench.TRAIN_WORKLOADS["train256"]
    names = syn.random_frame(w["n_atoms"], w["n_species"], seed=0)[3]

    def new_model(avg_num_neighbors=20.0):
        return NequIPGNNModel(
            seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=w["num_layers"], l_max=w["l_max"],
            parity=False, num_features=w["num_features"], radial_mlp_depth=1, radial_mlp_width=128,
            avg_num_neighbors=avg_num_neighbors, per_type_energy_scales=1.0, per_type_energy_shifts=0.0).to(device).train()

    model = new_model()
    gen = torch.Generator().manual_seed(0)
    grads = [(torch.randn(p.shape, generator=gen) * 1e-2).to(device) for p in model.parameters()]

    def parameters():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
        for p, g in zip(ps, grads):
            p.grad = g.clone()
        return ps

    numel = sum(g.numel() for g in grads)
    nbytes = sum(g.numel() * g.element_size() for g in grads)
    norm = float(torch.sqrt(sum(g.double().square().sum() for g in grads)))

    variants, skipped = {}, {}
    variants["adam_capturable"] = torch.optim.Adam(parameters(), lr=1e-3, capturable=True, foreach=True).step
    try:
        fused = torch.optim.Adam(parameters(), lr=1e-3, capturable=True, fused=True)
        fused.step()
        torch.cuda.synchronize()
        variants["adam_fused"] = fused.step
    except Exception as exc:  # this torch does not offer the fused form here
        skipped["adam_fused"] = f"{type(exc).__name__}: {exc}"
    hip = Adam(parameters(), lr=1e-3)
    variants["hip"] = hip.step
    variants["hip_clip_norm"] = Adam(parameters(), lr=1e-3, gradient_clip_val=0.5 * norm).step
    variants["hip_amsgrad"] = Adam(parameters(), lr=1e-3, amsgrad=True).step
    aten_params = parameters()
    aten = Adam(aten_params, lr=1e-3)
    aten._ensure_state()
    aten_rows = [(p, p.grad, aten.state[p]["exp_avg"], aten.state[p]["exp_avg_sq"], None, aten.state[p]["step"], 0)
                 for p in aten_params]

    def aten_step():
        with torch.no_grad():
            ad._aten_step(aten_rows, aten.param_groups[0], 1.0, None)

    eager_only = {"aten": aten_step}

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
    eager = alternating({**variants, **eager_only}, args.steps)
    replay = alternating({k: g.replay for k, g in graphs.items()}, args.steps)
    med = {k: statistics.median(v) for k, v in replay.items()}
    res = {"workload": "parameter list of the train256 model", "device": torch.cuda.get_device_name(0), "torch": torch.__version__,
           "parameters": len(grads), "elements": numel, "bytes_per_step": 7 * nbytes, "blocks": args.blocks,
           "steps_per_block": args.steps, "step_eager": report(eager), "step_graph_replay": report(replay), "skipped": skipped,
           "hip_replay_tb_per_s": round(7 * nbytes / (med["hip"] * 1e-6) / 1e12, 3),
           "hip_replay_fraction_of_hbm_copy_rate": round(7 * nbytes / (med["hip"] * 1e-6) / 1e12 / HBM_COPY_TBS, 3),
           "hip_replay_over_adam_capturable_replay": round(med["hip"] / med["adam_capturable"], 4),
           "step_count_after": float(hip.state[hip.param_groups[0]["params"][0]]["step"])}
    if "adam_fused" in med:
        res["hip_replay_over_adam_fused_replay"] = round(med["hip"] / med["adam_fused"], 4)

    launches = {}
    try:
        from torch.profiler import ProfilerActivity, profile

        for k, fn in {**variants, **eager_only}.items():
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                fn()
                torch.cuda.synchronize()
            launches[k] = sum(1 for ev in prof.events() if ev.device_type == torch.autograd.DeviceType.CUDA)
    except Exception as exc:  # the counts are then not measured
        launches = {"error": f"{type(exc).__name__}: {exc}"}
    res["device_kernels_and_copies_per_call"] = launches

    # ---- the whole train256 step, captured with either optimizer ------------------------------------------------------------------
    try:
        frames = []
        for f in range(w["batch"]):
            pos, types, cell, _ = syn.random_frame(w["n_atoms"], w["n_species"], seed=f)
            frames.append(syn.make_data(pos, types, 4.5, cell))
        data = AtomicDataDict.to_device(AtomicDataDict.batched_from_list(frames), device)
        n_atoms, n_edges = data["pos"].shape[0], data["edge_index"].shape[1]
        f_target = torch.randn(n_atoms, 3, generator=gen, dtype=torch.float64).to(device)
        e_target = torch.randn(w["batch"], 1, generator=gen, dtype=torch.float64).to(device)

        def train_graph(make_optimizer):
            m = new_model(n_edges / n_atoms)
            opt = make_optimizer(m.parameters())

            def step():
                opt.zero_grad(set_to_none=False)  # (the gradient buffers stay where they are: the capture recipe)
                out = m(dict(data))
                loss = (out["forces"] - f_target).square().mean() + (out["total_energy"] - e_target).square().mean()
                loss.backward()
                opt.step()

            return capture(step), m, opt

        trains = {"train256_torch_adam_capturable": train_graph(lambda ps: torch.optim.Adam(ps, lr=1e-2, capturable=True)),
                  "train256_hip_adam": train_graph(lambda ps: Adam(ps, lr=1e-2))}
        times = alternating({k: t[0].replay for k, t in trains.items()}, args.train_steps)
        res["train256_step_graph_replay"] = report(times)
        a, b = (statistics.median(times[k]) for k in ("train256_hip_adam", "train256_torch_adam_capturable"))
        res["train256_hip_over_torch"] = round(a / b, 4)
    except Exception as exc:  # reported, not hidden: the optimizer-only numbers above stand on their own
        res["train256_step_graph_replay"] = {"error": f"{type(exc).__name__}: {exc}"}

    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
