#!/usr/bin/env python3
"""Steps per second of Nose-Hoover dynamics on the bench water box (``bench.py``'s default workload: 10 125 atoms, the cfg-3
model), two loops around ONE ``GraphedStep`` (the calculator's: energy, per-atom energies, forces, stress, virial):

* ``device_driver``  ``nequip_amd.integrations.NoseHoover``: positions, velocities and the bath variable stay on the device, two
                     HIP launches between two replays; per step the host reads the two status flags of ``GraphedStep``;
* ``host_numpy``     today's route through ``NequIPCalculator(graphed_md=True)`` and a host integrator, restated: upload the
                     positions, replay, copy the five outputs to numpy, the reference's Nose-Hoover arithmetic in numpy.

Both start from the same state and take one force evaluation per step.  Timed with the host clock around blocks that end in a
device synchronisation, in alternating blocks within one process after a warm-up of both; median, minimum and maximum over the
blocks are reported.  The dynamics are gentle on purpose (50 K, 0.1 fs): the model is untrained, and a list that outgrows its
capacity would put a new capture into a timed block (``captures`` in the result says whether that happened).
Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_md_integrator.py [--blocks 10 --steps 50 --warmup 20] [--workload water10k] [--out FILE]
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
    from nequip_amd.integrations import NoseHoover, maxwell_boltzmann_velocities, units
    from nequip_amd.integrations.graphed_step import GraphedStep

    assert torch.cuda.is_available(), "bench_md_integrator.py measures on the GPU only"
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
    dt, temperature, q = 0.1 * units.fs, 50.0, 0.01 * n
    vel0 = maxwell_boltzmann_velocities(masses, temperature, generator=torch.Generator().manual_seed(0))
    outputs = (K.TOTAL_ENERGY_KEY, K.PER_ATOM_ENERGY_KEY, K.FORCE_KEY, K.STRESS_KEY, K.VIRIAL_KEY)
    step = GraphedStep(model, types.to(dev), data[K.CELL_KEY].view(3, 3).to(dev), True, float(cfg["r_max"]),
                       headroom=args.headroom, outputs=outputs)

    # ---- (a) the device driver --------------------------------------------------------------------------------------------
    drv = NoseHoover(step, masses.to(dev), dt, temperature, q, pos0.to(dev), vel0.to(dev))
    vel0 = drv.velocities.cpu()  # (without drift: the start of both loops)

    def device_driver(k):
        drv.run(k)
        torch.cuda.synchronize()

    # ---- (b) the host route -----------------------------------------------------------------------------------------------
    class Host:
        def __init__(self):
            self.m = masses.numpy()[:, None]
            self.x, self.v, self.xi = pos0.numpy().copy(), vel0.numpy().copy(), 0.0
            self.results = self.evaluate()

        def evaluate(self):
            out = step(torch.as_tensor(self.x).to(dev))
            return {k: out[k].detach().cpu().numpy() for k in outputs if k in out}

        def step(self):
            g = (3 * n + 1) * units.kB * temperature
            f = self.results[K.FORCE_KEY]
            a = f / self.m - self.xi * self.v
            self.x = self.x + dt * self.v + 0.5 * dt * dt * a
            v_half = self.v + 0.5 * dt * a
            xi_half = self.xi + 0.5 * dt * (0.5 * (np.sum(self.m * self.v * self.v) - g)) / q
            self.xi = xi_half + 0.5 * dt * (0.5 * (np.sum(self.m * v_half * v_half) - g)) / q
            self.results = self.evaluate()
            self.v = (v_half + 0.5 * dt * self.results[K.FORCE_KEY] / self.m) / (1.0 + 0.5 * dt * self.xi)

    host = Host()

    def host_numpy(k):
        for _ in range(k):
            host.step()
        torch.cuda.synchronize()

    loops = {"device_driver": device_driver, "host_numpy": host_numpy}
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

    res = {"workload": args.workload, "atoms": n, "device": torch.cuda.get_device_name(0), "blocks": args.blocks,
           "steps_per_block": args.steps, "warmup_steps": args.warmup,
           "outputs_per_step_host_route": [k for k in outputs if k in host.results],
           **{k: report(v) for k, v in times.items()},
           "host_over_device": round(statistics.median(times["host_numpy"]) / statistics.median(times["device_driver"]), 3),
           "captures_in_timed_blocks": step.num_captures - captures_before, "eager_fallbacks": step.num_eager_fallbacks,
           "edges": step.last_num_edges, "edge_capacity": step.edge_capacity,
           "temperature_K": {"device_driver": round(drv.temperature, 2),
                             "host_numpy": round(float(np.sum(host.m * host.v * host.v) / (3 * n * units.kB)), 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
