#!/usr/bin/env python3
"""Milliseconds per step of Langevin dynamics of MANY small systems at once: 256 periodic water boxes of about 64 atoms (19 to 24
molecules of a 27-molecule ``water_box``, in its cell) through ONE batched force evaluation per step (the cfg-3 model of
``bench.py`` under ``NequIPTorchSimCalc``), and three integrators around it:

* ``batched_device``  ``nequip_amd.integrations.BatchedLangevin``: the state and one record per system stay on the device, two
                      HIP launches for the whole batch between two force evaluations;
* ``aten_device``     the same driver with ``backend="aten"`` on the device: the same equations as a chain of ATen ops, the noise
                      made by numpy on the host and uploaded;
* ``host_numpy``      the route without a driver: forces copied to numpy, BAOAB in numpy (numpy's own generator), positions
                      uploaded.

And the integrator alone, with a constant force in place of the model: the batched launches for all 256 systems and for the
first ``--singles`` of them, against that many single-system ``Langevin`` objects stepped one after the other (2 launches each:
the route there was before the batched driver).

Timed with the host clock around blocks that end in a device synchronisation, in alternating blocks within one process after a
warm-up of all; median, minimum and maximum over the blocks are reported.  The dynamics are gentle on purpose (50 K, 0.1 fs): the
model is untrained.  Prints one JSON line; ``--out`` also writes it to a file.

    python scripts/bench_md_batched.py [--systems 256 --singles 64 --blocks 8 --steps 5 --warmup 3] [--out profiles/md_batched_bench.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time
from types import SimpleNamespace

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=256)
    ap.add_argument("--singles", type=int, default=64, help="how many single-system Langevin objects the integrator-alone loop steps")
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--steps", type=int, default=5, help="MD steps per timed block of the routes around the model")
    ap.add_argument("--integrator-steps", type=int, default=50, help="steps per timed block of the integrator-alone loops")
    ap.add_argument("--warmup", type=int, default=3, help="untimed steps of each loop")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch

    import bench
    from nequip_amd.integrations import BatchedLangevin, Langevin, maxwell_boltzmann_velocities, units
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc
    from nequip_amd.utils import synthetic as syn

    assert torch.cuda.is_available(), "bench_md_batched.py measures on the GPU only"
    dev = torch.device("cuda:0")
    S = args.systems
    rng = np.random.default_rng(0)
    z_of, mass_of = {"H": 1, "O": 8}, {"H": 1.008, "O": 15.999}
    pos, numbers, masses, cells, sidx = [], [], [], [], []
    for s in range(S):
        p, types, cell, names = syn.water_box(3, seed=s)
        keep = 3 * int(rng.integers(19, 25))  # whole molecules: 57 to 72 atoms
        pos.append(p[:keep])
        numbers += [z_of[names[t]] for t in types[:keep]]
        masses += [mass_of[names[t]] for t in types[:keep]]
        cells.append(cell)
        sidx += [s] * keep
    counts = [len(p) for p in pos]
    begin = np.concatenate([[0], np.cumsum(counts)])
    t = lambda a, dtype: torch.tensor(np.asarray(a), dtype=dtype, device=dev)  # noqa: E731
    x0, cell, z, idx, m = (t(np.concatenate(pos), torch.float64), t(np.stack(cells), torch.float64), t(numbers, torch.long),
                           t(sidx, torch.long), t(masses, torch.float64))
    n = int(x0.shape[0])
    dt, temperature, friction = 0.1 * units.fs, 50.0, 0.01 / units.fs
    v0 = maxwell_boltzmann_velocities(m.cpu(), temperature, generator=torch.Generator().manual_seed(0)).to(dev)

    w = bench.WORKLOADS["water10k"]
    model = bench.build_model(bench.model_cfg(w, 38.0), names, dev)
    calc = NequIPTorchSimCalc(model, device=dev)
    calc.compute_stress = False

    # ---- the three routes around the model ---------------------------------------------------------------------------------
    batched = BatchedLangevin.from_torchsim(calc, x0, cell, True, z, idx, m, dt, temperature, friction, velocities=v0, seed=1)
    aten = BatchedLangevin.from_torchsim(calc, x0, cell, True, z, idx, m, dt, temperature, friction, velocities=v0, seed=1,
                                         backend="aten")
    assert batched._hip and not aten._hip

    class Host:
        def __init__(self):
            self.m = m.cpu().numpy()[:, None]
            self.x, self.v = x0.cpu().numpy().copy(), v0.cpu().numpy().copy()
            self.rng = np.random.default_rng(1)
            self.c1 = math.exp(-friction * dt)
            self.c2 = math.sqrt(1.0 - self.c1 * self.c1)
            self.sigma = self.c2 * np.sqrt(units.kB * temperature / self.m)
            numbers_for_calc = None if getattr(calc, "atomic_numbers_in_init", False) else z
            self.state = SimpleNamespace(positions=None, row_vector_cell=cell, pbc=True, atomic_numbers=numbers_for_calc,
                                         system_idx=idx)
            self.nsteps = 0
            self.f = self.evaluate()

        def evaluate(self):
            self.state.positions = torch.as_tensor(self.x).to(dev)
            return calc(self.state)["forces"].detach().cpu().numpy().astype(np.float64)

        def step(self):
            hdt = 0.5 * dt
            v1 = self.v + hdt * (self.f / self.m)
            x = self.x + hdt * v1
            v2 = self.c1 * v1 + self.sigma * self.rng.standard_normal(self.v.shape)
            self.x = x + hdt * v2
            self.f = self.evaluate()
            self.v = v2 + hdt * (self.f / self.m)
            self.nsteps += 1

    host = Host()

    def run_driver(drv):
        def loop(k):
            drv.run(k)
            torch.cuda.synchronize()
        return loop

    def host_numpy(k):
        for _ in range(k):
            host.step()
        torch.cuda.synchronize()

    model_loops = {"batched_device": run_driver(batched), "aten_device": run_driver(aten), "host_numpy": host_numpy}

    # ---- the integrator alone: a constant force in place of the model ------------------------------------------------------
    force = 0.01 * torch.randn(n, 3, dtype=torch.float32, device=dev, generator=torch.Generator(device=dev).manual_seed(2))
    energy = torch.zeros(S, dtype=torch.float64, device=dev)
    k_single = min(args.singles, S)
    n_first = int(begin[k_single])

    def constant(lo, hi, systems):
        out = {"forces": force[lo:hi], "total_energy": energy[:systems]}
        return lambda positions: out

    alone_all = BatchedLangevin(constant(0, n, S), m, dt, temperature, friction, x0, idx, v0, seed=1)
    alone_first = BatchedLangevin(constant(0, n_first, k_single), m[:n_first], dt, temperature, friction, x0[:n_first],
                                  idx[:n_first], v0[:n_first], seed=1)
    singles = [Langevin(constant(int(begin[s]), int(begin[s + 1]), 1), m[begin[s]:begin[s + 1]], dt, temperature, friction,
                        x0[begin[s]:begin[s + 1]], v0[begin[s]:begin[s + 1]], seed=1 + s) for s in range(k_single)]

    def single_objects(k):
        for _ in range(k):
            for one in singles:
                one.step()
        torch.cuda.synchronize()

    integrator_loops = {f"integrator_batched_{S}": run_driver(alone_all), f"integrator_batched_{k_single}": run_driver(alone_first),
                        f"integrator_{k_single}_single_objects": single_objects}

    def measure(loops, steps):
        for fn in loops.values():
            fn(args.warmup)
        times = {k: [] for k in loops}
        keys = list(loops)
        for i in range(args.blocks):
            for key in (keys if i % 2 == 0 else keys[::-1]):
                t0 = time.perf_counter()
                loops[key](steps)
                times[key].append((time.perf_counter() - t0) / steps)
        return times

    def report(v):
        return {"median_ms": round(statistics.median(v) * 1e3, 4), "min_ms": round(min(v) * 1e3, 4),
                "max_ms": round(max(v) * 1e3, 4)}

    model_times = measure(model_loops, args.steps)
    integrator_times = measure(integrator_loops, args.integrator_steps)
    # the batch and the single objects take the same steps (seeds 1 + s): the check that the loops compared do the same work
    same = all(torch.equal(alone_first.positions[begin[s]:begin[s + 1]], singles[s].positions) for s in range(k_single))
    res = {"systems": S, "atoms": n, "atoms_per_system": {"min": min(counts), "max": max(counts)},
           "device": torch.cuda.get_device_name(0), "blocks": args.blocks, "steps_per_block": args.steps,
           "integrator_steps_per_block": args.integrator_steps, "warmup_steps": args.warmup,
           "timestep_fs": dt / units.fs, "temperature_K": temperature,
           "per_step_around_the_model": {k: report(v) for k, v in model_times.items()},
           "integrator_alone_per_step": {k: report(v) for k, v in integrator_times.items()},
           "launches_per_step": {"batched": 2, f"{k_single}_single_objects": 2 * k_single},
           "batch_and_single_objects_same_bits": bool(same),
           "nsteps": {"batched_device": int(batched.nsteps[0]), "aten_device": int(aten.nsteps[0]), "host_numpy": host.nsteps},
           "temperature_K_mean": {"batched_device": round(float(batched.temperature.mean()), 2),
                                  "aten_device": round(float(aten.temperature.mean()), 2)}}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
