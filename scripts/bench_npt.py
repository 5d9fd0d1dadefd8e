#!/usr/bin/env python3
"""Steps per second of constant-pressure Langevin dynamics on the bench water box (``bench.py``'s default workload: 10 125 atoms,
the cfg-3 model), three loops around ONE ``GraphedStep`` (energy, forces and stress):

* ``npt_device``   ``nequip_amd.integrations.LangevinNPT``: positions, velocities, the cell and the records stay on the device,
                   three HIP launches between two replays, the cell goes to the step by ``set_cell_from_device``;
* ``nvt_device``   ``nequip_amd.integrations.Langevin`` around the same stress-producing step at the fixed start cell: the parent
                   to compare with (two launches; what NPT adds is one launch, one wavefront longer, and the cell copies);
* ``npt_host``     the route without the driver, restated: replay, copy energy, forces and stress to numpy, BAOAB and the
                   stochastic cell rescaling in numpy (numpy's own generator), then ``set_cell`` and the upload of the positions.

All start from the same state and take one force evaluation per step.  Timed with the host clock around blocks that end in a
device synchronisation, in alternating blocks within one process after a warm-up of all; median, minimum and maximum over the
blocks are reported.  The dynamics are gentle on purpose (50 K, 0.1 fs, taup 10 ps): the model is untrained, and a neighbour list
that outgrows its capacity would put a new capture into a timed block (``captures_in_timed_blocks`` says whether that happened).
The step's output buffers are shared, so the first step of a device block takes the forces the previous loop left there (its
trajectory is a neighbour of this one): harmless to the timing, and why this script is no physics run.
Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_npt.py [--blocks 10 --steps 50 --warmup 20] [--workload water10k] [--out profiles/npt_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50, help="MD steps per timed block")
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps of each loop")
    ap.add_argument("--workload", default="water10k")
    ap.add_argument("--headroom", type=float, default=1.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.integrations import Langevin, LangevinNPT, maxwell_boltzmann_velocities, units
    from nequip_amd.integrations.graphed_step import GraphedStep

    assert torch.cuda.is_available(), "bench_npt.py measures on the GPU only"
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS[args.workload]
    data, names = bench.build_box(w, seed=0)
    n = int(data[K.POSITIONS_KEY].shape[0])
    cfg = bench.model_cfg(w, data[K.EDGE_INDEX_KEY].shape[1] / n)
    model = bench.build_model(cfg, names, dev)
    types = data[K.ATOM_TYPE_KEY].view(-1)
    mass_of = {"H": 1.008, "O": 15.999, "Si": 28.085, "Cu": 63.546}
    masses = torch.tensor([mass_of[s] for s in names], dtype=torch.float64)[types]
    pos0 = data[K.POSITIONS_KEY].to(torch.float64)
    cell0 = data[K.CELL_KEY].view(3, 3).to(torch.float64)
    dt, temperature, friction = 0.1 * units.fs, 50.0, 0.01 / units.fs
    p0, compressibility, taup = 1.0 * units.bar, 4.57e-5 / units.bar, 1.0e4 * units.fs
    vel0 = maxwell_boltzmann_velocities(masses, temperature, generator=torch.Generator().manual_seed(0))
    outputs = (K.TOTAL_ENERGY_KEY, K.FORCE_KEY, K.STRESS_KEY)
    step = GraphedStep(model, types.to(dev), cell0.to(dev), True, float(cfg["r_max"]), headroom=args.headroom, outputs=outputs)
    cell0_dev = cell0.to(dev).reshape(1, 3, 3)

    # ---- (a) NPT on the device, (b) NVT on the device around the same step -----------------------------------------------
    npt = LangevinNPT(step, masses.to(dev), dt, temperature, friction, p0, compressibility, taup, pos0.to(dev), cell0.to(dev),
                      vel0.to(dev), seed=1)
    nvt = Langevin(step, masses.to(dev), dt, temperature, friction, pos0.to(dev), vel0.to(dev), seed=1)

    def npt_device(k):
        npt.run(k)
        torch.cuda.synchronize()

    def nvt_device(k):
        step.set_cell_from_device(cell0_dev)  # (the step is shared: back to the fixed cell, once per block)
        nvt.run(k)
        torch.cuda.synchronize()

    # ---- (c) the host route -----------------------------------------------------------------------------------------------
    class Host:
        def __init__(self):
            self.m = masses.numpy()[:, None]
            self.x, self.v, self.cell = pos0.numpy().copy(), vel0.numpy().copy(), cell0.numpy().copy()
            self.rng = np.random.default_rng(1)
            self.kt = units.kB * temperature
            self.c1 = math.exp(-friction * dt)
            self.c2 = math.sqrt(1.0 - self.c1 * self.c1)
            self.a = compressibility * dt / taup
            self.pressure, self.nsteps = 0.0, 0
            self.results = self.evaluate()

        def evaluate(self):
            step.set_cell(torch.as_tensor(self.cell).to(dev))
            out = step(torch.as_tensor(self.x).to(dev))
            return {k: out[k].detach().cpu().numpy() for k in outputs}

        def step(self):
            hdt = 0.5 * dt
            f = self.results[K.FORCE_KEY].astype(np.float64)
            sigma = self.results[K.STRESS_KEY].astype(np.float64).reshape(3, 3)
            ekin = 0.5 * float(np.sum(self.m * self.v * self.v))
            v1 = self.v + hdt * (f / self.m)
            x = self.x + hdt * v1
            v2 = self.c1 * v1 + (self.c2 * np.sqrt(self.kt / self.m)) * self.rng.standard_normal(self.v.shape)
            x = x + hdt * v2
            vol = abs(float(np.linalg.det(self.cell)))
            self.pressure = (2.0 * ekin) / (3.0 * vol) - float(np.trace(sigma)) / 3.0
            d_eps = -self.a * (p0 - self.pressure) + math.sqrt((2.0 * self.kt * self.a) / vol) * float(self.rng.standard_normal())
            mu = math.exp(d_eps / 3.0)
            self.cell, self.x, v2 = mu * self.cell, mu * x, v2 / mu
            self.results = self.evaluate()
            self.v = v2 + hdt * (self.results[K.FORCE_KEY].astype(np.float64) / self.m)
            self.nsteps += 1

    host = Host()

    def npt_host(k):
        for _ in range(k):
            host.step()
        torch.cuda.synchronize()

    loops = {"npt_device": npt_device, "nvt_device": nvt_device, "npt_host": npt_host}
    for fn in loops.values():
        fn(args.warmup)
    captures_before = step.num_captures
    times = {k: [] for k in loops}
    keys = list(loops)
    for i in range(args.blocks):
        for key in (keys if i % 2 == 0 else keys[::-1]):
            t0 = time.perf_counter()
            loops[key](args.steps)
            times[key].append((time.perf_counter() - t0) / args.steps)

    def report(v):
        return {"median_ms": round(statistics.median(v) * 1e3, 4), "min_ms": round(min(v) * 1e3, 4),
                "max_ms": round(max(v) * 1e3, 4), "steps_per_s": round(1.0 / statistics.median(v), 1)}

    med = {k: statistics.median(v) for k, v in times.items()}
    res = {"workload": args.workload, "atoms": n, "device": torch.cuda.get_device_name(0), "blocks": args.blocks,
           "steps_per_block": args.steps, "warmup_steps": args.warmup, "outputs_per_step_host_route": list(outputs),
           "barostat": {"a": compressibility * dt / taup, "p0_eV_per_A3": p0, "timestep_fs": dt / units.fs,
                        "temperature_K": temperature},
           **{k: report(v) for k, v in times.items()},
           "npt_minus_nvt_ms": round((med["npt_device"] - med["nvt_device"]) * 1e3, 4),
           "host_over_device": round(med["npt_host"] / med["npt_device"], 3),
           "captures_in_timed_blocks": step.num_captures - captures_before, "eager_fallbacks": step.num_eager_fallbacks,
           "edges": step.last_num_edges, "edge_capacity": step.edge_capacity,
           "nsteps": {"npt_device": npt.nsteps, "nvt_device": nvt.nsteps, "npt_host": host.nsteps},
           "pressure_eV_per_A3": {"npt_device": round(npt.pressure, 8), "npt_host": round(host.pressure, 8)},
           "volume_A3": {"start": round(abs(float(np.linalg.det(cell0.numpy()))), 4), "npt_device": round(npt.volume, 4),
                         "npt_host": round(abs(float(np.linalg.det(host.cell))), 4)},
           "temperature_K": {"npt_device": round(npt.temperature, 2), "nvt_device": round(nvt.temperature, 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
