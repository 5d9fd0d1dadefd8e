#!/usr/bin/env python3
"""Cost of the conflict-free gradients (``nequip_amd.train.ConFIGGradients``) on the parameter list of the train256 model
(``bench.py``'s training workload), with K = 2 and 3 loss terms.  One call of a variant starts from K stored per-term gradients,
copies each into the ``.grad``s (``torch._foreach_copy_``: what a backward pass would have left there; the same in every
variant and timed alone as ``fill``) and ends with the new gradient in every ``.grad``:

* ``hip``          ``nqa_config_collect`` after each copy, ``nqa_config_gram``, ``nqa_config_apply`` (csrc/config.hip);
* ``aten_pinv``    the reference's lines in ATen on the GPU: ``torch.cat`` per term, ``stack``, three ``normalize``s,
                   ``torch.linalg.pinv`` on the [K, P] matrix, one ``narrow`` + ``.to`` + ``view`` per parameter;
* ``aten_lstsq``   the same with ``torch.linalg.lstsq`` where the device accepts it (if not: the message is recorded).

Each is timed eagerly, and ``fill`` and ``hip`` also as a replayed hipGraph (the solvers of the ATen forms read results back on
the host and do not capture), with device events in alternating blocks within one
process.  Kernel count and kernel time of the ``hip`` variant come from ``rocprofv3 --kernel-trace --stats`` around a fresh
child process that runs only that variant (``--trace-child``).  Then the whole training step captured as one hipGraph:
``EnergyForceLoss`` with the weighted sum and one backward pass, against ConFIG with K = 2 backward passes (context: about K
backward passes against one).  Prints one JSON line.

    python scripts/bench_config.py [--blocks 10 --steps 50 --train-steps 20] [--no-train] [--no-trace]
"""
import argparse
import csv
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def kernel_trace(k, calls):
    """Kernel count and time per call of the hip variant, from rocprofv3 around a child process of its own."""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return {"error": "rocprofv3 not found"}
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [tool, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "--", sys.executable,
               os.path.abspath(__file__), "--trace-child", str(k), "--trace-calls", str(calls)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        if r.returncode != 0:
            return {"error": f"rocprofv3 exit {r.returncode}: {r.stderr[-500:]}"}
        files = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            return {"error": "no kernel_stats.csv written"}
        rows = list(csv.DictReader(open(files[0])))
    out = {}
    for row in rows:
        name = row.get("Name", "")
        if "config_" in name:
            short = name.split("(")[0].split("::")[-1]
            out[short] = {"calls_per_call": int(row["Calls"]) / calls,
                          "us_per_call": round(float(row["TotalDurationNs"]) / calls / 1e3, 2)}
    out["kernels_per_call"] = sum(v["calls_per_call"] for v in out.values())
    out["kernel_us_per_call"] = round(sum(v["us_per_call"] for v in out.values() if isinstance(v, dict)), 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--train-steps", type=int, default=20)
    ap.add_argument("--no-train", action="store_true", help="skip the captured training step")
    ap.add_argument("--no-trace", action="store_true", help="skip the rocprofv3 pass")
    ap.add_argument("--trace-child", type=int, default=0, help="(internal) run only the hip variant with this K")
    ap.add_argument("--trace-calls", type=int, default=20)
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.train import ConFIGGradients, EnergyForceLoss
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_config.py measures on the GPU only"
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
    params = [p for p in model.parameters() if p.requires_grad]
    numel = sum(p.numel() for p in params)
    eps = 1e-8

    class Coefficients:  # what ConFIGGradients reads of a MetricsManager
        def __init__(self, k):
            self.entries = {f"t{i}": argparse.Namespace(coeff=c) for i, c in enumerate([1.0, 5.0, 0.25][:k])}

    def variants_for(k):
        gen = torch.Generator().manual_seed(k)
        stored = [[(torch.randn(p.shape, generator=gen) * (0.1 + i)).to(device=device, dtype=p.dtype) for p in params]
                  for i in range(k)]
        coeffs = [c.coeff for c in Coefficients(k).entries.values()]
        cf = ConFIGGradients(model, Coefficients(k), norm_eps=eps)
        for p in params:
            if p.grad is None:
                p.grad = torch.zeros_like(p)
        grads = [p.grad for p in params]
        t = cf._device_tables(device, params, k)
        t.b[:k].copy_(torch.tensor(coeffs, dtype=torch.float64))
        def fill():
            for i in range(k):
                torch._foreach_copy_(grads, stored[i])

        def hip():  # the launches of ConFIGGradients.backward, a copy in the place of each backward pass
            cf._collect(t, -1)
            for i in range(k):
                torch._foreach_copy_(grads, stored[i])
                cf._collect(t, i)
            cf._combine(t)

        b_host = torch.tensor(coeffs, dtype=torch.float32)

        def aten(lsqr):
            def run():
                rows = []
                for i in range(k):
                    torch._foreach_copy_(grads, stored[i])
                    rows.append(torch.cat([g.flatten() for g in grads]))
                    torch._foreach_zero_(grads)
                a_raw = torch.stack(rows, dim=0)
                a = torch.nn.functional.normalize(a_raw, dim=1, eps=eps)
                b = torch.nn.functional.normalize(b_host.to(device=a.device, dtype=a.dtype), dim=0, eps=eps)
                x = torch.linalg.lstsq(a, b).solution if lsqr else torch.linalg.pinv(a) @ b
                x = torch.nn.functional.normalize(x, dim=0, eps=eps)
                new_grad = torch.sum(a_raw * x) * x
                start = 0
                for p in params:
                    p.grad.copy_(new_grad.narrow(0, start, p.numel()).to(dtype=p.dtype).view(p.shape))
                    start += p.numel()
            return run

        return {"fill": fill, "hip": hip, "aten_pinv": aten(False), "aten_lstsq": aten(True)}, (cf, stored)

    if args.trace_child:
        fns, keep = variants_for(args.trace_child)
        for _ in range(args.trace_calls):
            fns["hip"]()
        torch.cuda.synchronize()
        return

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

    res = {"workload": "parameter list of the train256 model", "device": torch.cuda.get_device_name(0),
           "parameters": len(params), "elements": numel, "blocks": args.blocks, "steps_per_block": args.steps}
    keep = []
    for k in (2, 3):
        fns, alive = variants_for(k)
        keep.append(alive)
        failed = {}
        for name in list(fns):  # a variant the device refuses is recorded, not timed
            try:
                fns[name]()
                torch.cuda.synchronize()
            except Exception as exc:
                failed[name] = f"{type(exc).__name__}: {str(exc)[:300]}"
                del fns[name]
        # (the ATen forms are not captured: pinv and lstsq read results back on the host, which a capturing stream refuses)
        graphs = {name: capture(fns[name]) for name in ("fill", "hip")}
        keep.append(graphs)
        # the hip result against the pinv form, on the stored gradients
        fns["hip"]()
        got = torch.cat([p.grad.flatten() for p in params]).double()
        fns["aten_pinv"]()
        ref = torch.cat([p.grad.flatten() for p in params]).double()
        res[f"K{k}"] = {"eager": report(alternating(fns, args.steps)),
                        "graph_replay": report(alternating({name: g.replay for name, g in graphs.items()}, args.steps)),
                        "not_run": failed,
                        "hip_vs_aten_pinv_float32_rel": float((got - ref).abs().max() / ref.abs().max())}
        if not args.no_trace:
            try:
                res[f"K{k}"]["hip_kernel_trace"] = kernel_trace(k, args.trace_calls)
            except Exception as exc:
                res[f"K{k}"]["hip_kernel_trace"] = {"error": f"{type(exc).__name__}: {exc}"}

    # ---- the whole captured training step -----------------------------------------------------------------------------------
    if not args.no_train:
        gen = torch.Generator().manual_seed(0)
        target = {"forces": torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device),
                  "total_energy": torch.randn(w["batch"], 1, generator=gen, dtype=torch.float64).to(device),
                  "num_atoms": data["num_atoms"] if "num_atoms" in data else torch.full((w["batch"],), w["n_atoms"], device=device)}

        def captured_step(with_config):
            net = make_model()
            opt = torch.optim.Adam(net.parameters(), lr=1e-2, capturable=True)
            loss_fn = EnergyForceLoss()
            cf = ConFIGGradients(net, loss_fn) if with_config else None

            def step():
                out = dict(net(dict(data)))
                out["num_atoms"] = target["num_atoms"]
                loss_dict = loss_fn(out, target)
                if cf is not None:
                    cf.backward(loss_dict)
                else:
                    opt.zero_grad(set_to_none=True)
                    loss_dict["weighted_sum"].backward()
                opt.step()

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
            if cf is None:
                opt.zero_grad(set_to_none=True)
            with torch.cuda.graph(g):
                step()
            g.replay()
            torch.cuda.synchronize()
            return g, (net, opt, cf, loss_fn)

        steps = {"weighted_sum_step": captured_step(False), "config_step_K2": captured_step(True)}
        times = alternating({k: v[0].replay for k, v in steps.items()}, args.train_steps)
        res["train_step_graph_replay"] = report(times)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
