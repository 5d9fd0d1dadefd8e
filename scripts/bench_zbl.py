#!/usr/bin/env python3
"""Cost of the ZBL pair term on the benchmarked step (water10k, cfg-3: 10 125 atoms, 400 558 edges, eval energy + forces).

Two models with the same weights -- with and without ``pair_potential`` (ZBL, H / O, metal units) -- each captured as a
hipGraph of one evaluation the way ``bench.py`` captures it; their replays are timed with device events in alternating
blocks within one process, so that clock and thermal drift fall on both alike.  Prints one JSON line.

``--trace``: afterwards runs this script again (``--replays-only``) under ``rocprofv3 --kernel-trace --stats`` in a child
process and adds the ZBL kernels' own times from that run's statistics, with their bytes over kernel time as a fraction of
the HBM peak (``--hbm-tbs``, default 8 TB/s).

    python scripts/bench_zbl.py [--blocks 10 --steps 50] [--trace]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)

ZBL = {"_target_": "nequip.nn.pair_potential.ZBL", "chemical_species": ["H", "O"], "units": "metal"}


def capture(model, data):
    import torch

    from nequip_amd.data import AtomicDataDict as K

    def step():
        out = model(dict(data))
        return out[K.TOTAL_ENERGY_KEY].detach(), out[K.FORCE_KEY].detach()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = step()
    g.replay()
    torch.cuda.synchronize()
    ref = step()
    assert torch.allclose(outs[1], ref[1], atol=1e-5, rtol=1e-5), "graph replay disagrees with eager"
    return g, outs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--replays-only", action="store_true", help="(child of --trace) replay both graphs, print nothing")
    ap.add_argument("--hbm-tbs", type=float, default=8.0)
    args = ap.parse_args()

    import torch

    import bench
    from nequip_amd.data import AtomicDataDict as K

    device = torch.device("cuda:0")
    w = bench.WORKLOADS["water10k"]
    data, names = bench.build_box(w)
    n, e = int(data[K.POSITIONS_KEY].shape[0]), int(data[K.EDGE_INDEX_KEY].shape[1])
    cfg = bench.model_cfg(w, e / n)
    data = {k: v.to(device) for k, v in data.items()}
    plain = bench.build_model(cfg, names, device)
    kw = {k: v for k, v in cfg.items() if k != "model_dtype"}
    from nequip_amd.model import NequIPGNNModel

    zbl = NequIPGNNModel(seed=0, model_dtype=cfg["model_dtype"], type_names=names, pair_potential=ZBL, **kw)
    zbl = zbl.to(device).eval()
    g_plain, o_plain = capture(plain, data)
    g_zbl, o_zbl = capture(zbl, data)
    d_e = float((o_zbl[0] - o_plain[0]).abs().max())

    def timed(g, k):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(k):
            g.replay()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / k

    for _ in range(2):
        timed(g_plain, 5), timed(g_zbl, 5)
    if args.replays_only:
        for _ in range(args.blocks):
            timed(g_plain, args.steps), timed(g_zbl, args.steps)
        return
    t_plain, t_zbl = [], []
    for i in range(args.blocks):
        order = ((g_plain, t_plain), (g_zbl, t_zbl)) if i % 2 == 0 else ((g_zbl, t_zbl), (g_plain, t_plain))
        for g, acc in order:
            acc.append(timed(g, args.steps))
    mp, mz = statistics.median(t_plain), statistics.median(t_zbl)
    res = {"workload": "water10k", "atoms": n, "edges": e, "ms_plain": round(mp, 4), "ms_zbl": round(mz, 4),
           "added_us": round((mz - mp) * 1e3, 1), "added_frac": round((mz - mp) / mp, 4),
           "blocks_plain_ms": [round(t, 4) for t in t_plain], "blocks_zbl_ms": [round(t, 4) for t in t_zbl],
           "zbl_energy_eV": round(d_e, 3)}
    if args.trace:
        res["kernels"] = trace(args, n, e)
    print(json.dumps(res))


# bytes moved per call (float64 vectors, int32 CSR, int64 types; per-atom reads / writes): what the roofline divides by
def _bytes(kernel: str, n: int, e: int) -> float:
    per_edge = 24 + 4 + 4 + 8  # edge vector, edge id, neighbour, neighbour type
    per_atom = 4 + 8 + 16      # row pointer, type, energy in / gradient in, energy out
    if "zbl_kernel<1>" in kernel:
        per_edge += 24         # dE/d edge_vec out
    elif "zbl_kernel<2>" in kernel:
        per_edge += 48         # cotangent in, second-order gradient out
    return per_edge * e + per_atom * n


def trace(args, n: int, e: int):
    out_dir = tempfile.mkdtemp(prefix="zbl_trace_")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out_dir, "-o", "zbl", "--",
           sys.executable, os.path.abspath(__file__), "--replays-only", "--blocks", "4", "--steps", str(args.steps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT)
    if r.returncode != 0:
        return {"error": f"rocprofv3 exited {r.returncode}", "stderr": r.stderr[-2000:]}
    stats = glob.glob(os.path.join(out_dir, "**", "*kernel_stats.csv"), recursive=True)
    if not stats:
        return {"error": "no kernel_stats.csv", "dir": out_dir}
    rows = {}
    total_ns = 0.0
    with open(stats[0]) as f:
        for row in csv.DictReader(f):
            total_ns += float(row["TotalDurationNs"])
            if "zbl_kernel" in row["Name"]:
                avg_ns = float(row["AverageNs"])
                rows[row["Name"]] = {"calls": int(row["Calls"]), "avg_us": round(avg_ns / 1e3, 2),
                                     "hbm_frac": round(_bytes(row["Name"], n, e) / (avg_ns * 1e-9) / (args.hbm_tbs * 1e12), 3)}
    zbl_ns = sum(float(v["avg_us"]) * 1e3 * v["calls"] for v in rows.values())
    return {"per_kernel": rows, "share_of_kernel_time": round(zbl_ns / total_ns, 4) if total_ns else None,
            "stats_file": stats[0]}


if __name__ == "__main__":
    main()
