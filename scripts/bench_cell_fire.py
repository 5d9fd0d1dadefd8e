#!/usr/bin/env python3
"""Steps per second of a variable-cell FIRE relaxation on the bench water box (``bench.py``'s default workload: 10 125 atoms, the
cfg-3 model), two loops around ONE ``GraphedStep`` (energy, forces and stress):

* ``device_driver``  ``nequip_amd.integrations.CellFIRE``: positions, velocities, the deformation gradient and the optimizer's
                     record stay on the device, three HIP launches between two replays, the cell goes to the step by
                     ``set_cell_from_device``; the verdict is read once per block (``check_every`` = the block);
* ``host_numpy``     today's route through a calculator, a cell filter and a host optimizer, restated: replay, copy energy,
                     forces and stress to numpy, the literal ``UnitCellFilter`` + FIRE loop (ASE's arithmetic, its ``fmax``
                     test included) in numpy, then ``set_cell`` and the upload of the positions.

There is no fixed-cell parent to compare with: the host route around the same step is the baseline.  Both start from the same
perturbed box and take one force evaluation per step.  Timed with the host clock around blocks that end in a device
synchronisation, in alternating blocks within one process after a warm-up of both; median, minimum and maximum over the blocks
are reported.  The steps are short on purpose (``maxstep`` 0.01 for the whole box): the model is untrained, and a neighbour list
that outgrows its capacity would put a new capture into a timed block (``captures_in_timed_blocks`` says whether that happened).
Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_cell_fire.py [--blocks 10 --steps 50 --warmup 20] [--workload water10k] [--out profiles/cell_fire_bench.json]
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
    ap.add_argument("--steps", type=int, default=50, help="FIRE steps per timed block")
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps of each loop")
    ap.add_argument("--workload", default="water10k")
    ap.add_argument("--headroom", type=float, default=1.02)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.integrations import CellFIRE
    from nequip_amd.integrations.graphed_step import GraphedStep

    assert torch.cuda.is_available(), "bench_cell_fire.py measures on the GPU only"
    dev = torch.device("cuda:0")
    w = bench.WORKLOADS[args.workload]
    data, names = bench.build_box(w, seed=0)
    n = int(data[K.POSITIONS_KEY].shape[0])
    cfg = bench.model_cfg(w, data[K.EDGE_INDEX_KEY].shape[1] / n)
    model = bench.build_model(cfg, names, dev)
    types = data[K.ATOM_TYPE_KEY].view(-1)
    pos0 = data[K.POSITIONS_KEY].to(torch.float64)
    pos0 = pos0 + 0.01 * torch.randn(pos0.shape, dtype=torch.float64, generator=torch.Generator().manual_seed(0))
    cell0 = data[K.CELL_KEY].view(3, 3).to(torch.float64)
    params = dict(dt=0.1, maxstep=0.01, dtmax=1.0, nmin=5, finc=1.1, fdec=0.5, astart=0.1, fa=0.99)
    target = 1e-6  # (not reached: every step of both loops moves the box)
    outputs = (K.TOTAL_ENERGY_KEY, K.FORCE_KEY, K.STRESS_KEY)
    step = GraphedStep(model, types.to(dev), cell0.to(dev), True, float(cfg["r_max"]), headroom=args.headroom, outputs=outputs)

    # ---- (a) the device driver --------------------------------------------------------------------------------------------
    drv = CellFIRE(step, pos0.to(dev), cell0.to(dev), **params)

    def device_driver(k):
        drv.run(fmax=target, steps=k, check_every=k)
        torch.cuda.synchronize()

    # ---- (b) the host route -----------------------------------------------------------------------------------------------
    class Host:
        def __init__(self):
            self.x, self.cell, self.c0, self.v = pos0.numpy().copy(), cell0.numpy().copy(), cell0.numpy().copy(), None
            self.dt, self.a, self.npos, self.nsteps, self.fmax = params["dt"], params["astart"], 0, 0, float("inf")
            self.factor = float(n)

        def evaluate(self):
            step.set_cell(torch.as_tensor(self.cell).to(dev))
            out = step(torch.as_tensor(self.x).to(dev))
            return {k: out[k].detach().cpu().numpy() for k in outputs}

        def step(self):
            res = self.evaluate()
            # the filter: get_positions / get_forces
            D = np.linalg.solve(self.c0, self.cell).T
            r = np.concatenate([np.linalg.solve(D, self.x.T).T, self.factor * D])
            sigma = res[K.STRESS_KEY].astype(np.float64).reshape(3, 3)
            virial = -abs(np.linalg.det(self.cell)) * sigma
            virial = np.linalg.solve(D, virial.T).T
            f = np.concatenate([res[K.FORCE_KEY].astype(np.float64) @ D, virial / self.factor])
            self.fmax = float(np.sqrt((f * f).sum(axis=1).max()))
            if self.fmax < target:
                return
            if self.v is None:
                self.v = np.zeros_like(r)
            else:
                vf = np.vdot(f, self.v)
                if vf > 0.0:
                    self.v = (1.0 - self.a) * self.v + self.a * f / np.sqrt(np.vdot(f, f)) * np.sqrt(np.vdot(self.v, self.v))
                    if self.npos > params["nmin"]:
                        self.dt = min(self.dt * params["finc"], params["dtmax"])
                        self.a *= params["fa"]
                    self.npos += 1
                else:
                    self.v[:] *= 0.0
                    self.a = params["astart"]
                    self.dt *= params["fdec"]
                    self.npos = 0
            self.v += self.dt * f
            dr = self.dt * self.v
            normdr = np.sqrt(np.vdot(dr, dr))
            if normdr > params["maxstep"]:
                dr = params["maxstep"] * dr / normdr
            r = r + dr
            # the filter: set_positions
            D_new = r[n:] / self.factor
            self.cell = self.c0 @ D_new.T
            self.x = r[:n] @ D_new.T
            self.nsteps += 1

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
           "steps_per_block": args.steps, "warmup_steps": args.warmup, "outputs_per_step_host_route": list(outputs),
           "fire": params, **{k: report(v) for k, v in times.items()},
           "host_over_device": round(statistics.median(times["host_numpy"]) / statistics.median(times["device_driver"]), 3),
           "captures_in_timed_blocks": step.num_captures - captures_before, "eager_fallbacks": step.num_eager_fallbacks,
           "edges": step.last_num_edges, "edge_capacity": step.edge_capacity,
           "nsteps": {"device_driver": int(drv.nsteps[0]), "host_numpy": host.nsteps},
           "fmax_eV_per_A": {"device_driver": round(float(drv.fmax[0]), 6), "host_numpy": round(host.fmax, 6)},
           "volume_A3": {"device_driver": round(float(drv.volume[0]), 4), "host_numpy": round(abs(float(np.linalg.det(host.cell))), 4)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
