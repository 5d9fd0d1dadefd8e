"""What the batched Langevin tests share (tests/test_langevin_batched.py on the CPU, tests/test_langevin_batched_gpu.py on the
GPU): batches of unequal systems with per-system parameters, the drivers of a batch and of one of its systems alone around the
same analytic forces, and a view of one system of a batch with the scalar interface of the single-system drivers, so that the
comparisons of ``langevin_restatement`` and ``npt_restatement`` apply to it unchanged.

NVT force: a spring per atom, ``F_i = -k_i (x_i - CENTRE)``, element-wise, so that a system alone and inside a batch is handed
the same bits.  NPT force and stress: the tethered-site potential of ``cell_fire_restatement``, element-wise per atom and added
per system by a fixed tree that does not depend on the place of the rows in a larger array."""
import functools

import numpy as np
import torch

import cell_fire_restatement as C
import langevin_restatement as LR
import npt_restatement as NR
from nequip_amd.integrations import BatchedLangevin, BatchedLangevinNPT, Langevin, LangevinNPT

DT, T, FRICTION = 0.5 * LR.FS, 300.0, 0.01 / LR.FS
P0, COMPRESSIBILITY, TAUP = 0.01, 0.5, 50.0 * DT  # the stiff barostat of tests/test_langevin_npt.py
# 3, 255, 258, 3, 513 and 16 386 flat components: a fraction of a chunk, one component short of a chunk, the first component of
# a second chunk (which begins inside an atom), three chunks, and 65 chunks, so that the bath lanes add runs of two rows
COUNTS = (1, 85, 86, 1, 171, 5462)
DTYPES = {"f32": torch.float32, "f64": torch.float64}


@functools.lru_cache(maxsize=None)
def batch(counts, salt=0):
    """The systems of a batch, a dict each: masses, positions, velocities, springs, the site system, and their own time step,
    temperature, friction, seed, pressure, compressibility and taup.  Never modified."""
    systems = []
    for s, n in enumerate(counts):
        key = 1000 * salt + 37 * s + n
        m, x, v = LR.system(n, seed=key)
        part = C.site_system(n, seed=key)
        k = np.random.default_rng(key + 5).uniform(0.5, 2.0, size=n)
        r = s % 6  # (the parameters repeat after six systems, the seeds do not)
        systems.append(dict(n=n, m=m, x=x, v=v, k=k, part=part, dt=DT * (1.0 + 0.125 * r), temperature=T + 50.0 * r,
                            friction=FRICTION * (1.0 + 0.5 * r), seed=LR.SEED + 1000 * salt + 7 * s * s,
                            pressure=P0 * (1.0 - 0.5 * r), compressibility=COMPRESSIBILITY / (1.0 + 0.25 * r),
                            taup=TAUP * (1.0 + 0.1 * r)))
    return tuple(systems)


def offsets(systems):
    return np.concatenate([[0], np.cumsum([q["n"] for q in systems])])


def spring_force_step(systems, device, dtype=torch.float64):
    k = torch.from_numpy(np.concatenate([q["k"] for q in systems])).to(device)
    sidx = torch.from_numpy(np.repeat(np.arange(len(systems)), [q["n"] for q in systems])).to(device)
    centre = torch.tensor(LR.CENTRE, dtype=torch.float64, device=device)
    S = len(systems)

    def step(pos):
        d = pos - centre
        e = torch.zeros(S, dtype=torch.float64, device=pos.device).index_add_(0, sidx, 0.5 * k * (d * d).sum(1))
        return {"forces": (-k[:, None] * d).to(dtype), "total_energy": e}

    return step


def spring_force_restated(q, device, dtype=torch.float64):
    """The force callback of the restatement of one system: the same function on the same device, rounded like the driver's."""
    step = spring_force_step([q], device, dtype)
    return lambda x: step(torch.from_numpy(np.ascontiguousarray(x)).to(device))["forces"].double().cpu().numpy()


def _cat(systems, name, device):
    return torch.from_numpy(np.concatenate([q[name] for q in systems])).to(device)


def _sidx(systems, device):
    return torch.from_numpy(np.repeat(np.arange(len(systems)), [q["n"] for q in systems])).to(device)


def _each(systems, name):
    return [q[name] for q in systems]


def batched_nvt(systems, device, dtype=torch.float64, backend="auto", **kw):
    args = dict(timestep=_each(systems, "dt"), temperature=_each(systems, "temperature"), friction=_each(systems, "friction"),
                seed=_each(systems, "seed"))
    args.update(kw)
    return BatchedLangevin(spring_force_step(systems, device, dtype), _cat(systems, "m", device), args.pop("timestep"),
                           args.pop("temperature"), args.pop("friction"), _cat(systems, "x", device), _sidx(systems, device),
                           _cat(systems, "v", device), backend=backend, **args)


def single_nvt(q, device, dtype=torch.float64, backend="auto"):
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    return Langevin(spring_force_step([q], device, dtype), t(q["m"]), q["dt"], q["temperature"], q["friction"], t(q["x"]),
                    t(q["v"]), seed=q["seed"], backend=backend)


def restated_nvt(q, device, dtype=torch.float64):
    return LR.Restated(spring_force_restated(q, device, dtype), q["m"], q["dt"], q["temperature"], q["friction"], q["x"], q["v"],
                       seed=q["seed"])


def batched_npt(systems, device, dtype=torch.float64, backend="auto", **kw):
    args = {name: _each(systems, name) for name in ("dt", "temperature", "friction", "pressure", "compressibility", "taup", "seed")}
    args.update(kw)
    parts = [q["part"] for q in systems]
    x = torch.from_numpy(np.concatenate([p["x"] for p in parts])).to(device)
    cell = torch.from_numpy(np.stack([p["c0"] for p in parts])).to(device)
    return BatchedLangevinNPT(C.torch_force_step(parts, device, dtype), _cat(systems, "m", device), args["dt"], args["temperature"],
                              args["friction"], args["pressure"], args["compressibility"], args["taup"], x, cell,
                              _sidx(systems, device), _cat(systems, "v", device), seed=args["seed"], backend=backend)


def single_npt(q, device, dtype=torch.float64, backend="auto"):
    t = lambda a: torch.from_numpy(a).to(device)  # noqa: E731
    part = q["part"]
    return LangevinNPT(C.torch_force_step([part], device, dtype), t(q["m"]), q["dt"], q["temperature"], q["friction"],
                       q["pressure"], q["compressibility"], q["taup"], t(part["x"]), t(part["c0"]), t(q["v"]), seed=q["seed"],
                       backend=backend)


def restated_npt(q, device, dtype=torch.float64):
    part = q["part"]
    return NR.Restated(C.restated_force(part, device, dtype), q["m"], q["dt"], q["temperature"], q["friction"], q["pressure"],
                       q["compressibility"], q["taup"], part["x"], part["c0"], q["v"], seed=q["seed"])


class View:
    """System ``s`` of a batched driver behind the scalar interface of ``Langevin`` / ``LangevinNPT``."""

    def __init__(self, drv, s):
        b = np.concatenate([[0], np.cumsum(drv._counts)])
        self.drv, self.s, self.lo, self.hi = drv, s, int(b[s]), int(b[s + 1])

    @property
    def positions(self):
        return self.drv.positions[self.lo:self.hi]

    @property
    def velocities(self):
        return self.drv.velocities[self.lo:self.hi]

    @property
    def stored_velocities(self):
        return self.drv._vel[self.lo:self.hi]

    @property
    def kinetic_energy(self):
        return float(self.drv.kinetic_energy[self.s])

    @property
    def temperature(self):
        return float(self.drv.temperature[self.s])

    @property
    def nsteps(self):
        return int(self.drv.nsteps[self.s])

    @property
    def cell(self):
        return self.drv.cell[self.s:self.s + 1]

    @property
    def pressure(self):
        return float(self.drv.pressure[self.s])

    @property
    def volume(self):
        return float(self.drv.volume[self.s])

    @property
    def scaling(self):
        return float(self.drv.scaling[self.s])


def same_bits_nvt(view, alone):
    """Positions, stored velocities, completed velocities, kinetic energy and step count of a system in a batch and alone."""
    return (torch.equal(view.positions, alone.positions) and torch.equal(view.stored_velocities, alone._vel)
            and torch.equal(view.velocities.clone(), alone.velocities.clone()) and view.kinetic_energy == alone.kinetic_energy
            and view.temperature == alone.temperature and view.nsteps == alone.nsteps)
