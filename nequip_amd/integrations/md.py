"""Molecular dynamics with the state on the device: the reference's Nose-Hoover NVT scheme (``nequip/ase/nosehoover.py``) and,
as its thermostat-off case, velocity Verlet.

The reference integrates in numpy inside ``ase.md.MolecularDynamics``: through a calculator every step uploads the positions
and downloads energy, forces and stress.  Here positions, velocities, masses and the bath variable are device tensors, advanced
between two force evaluations by two HIP launches (``csrc/md.hip``: ``nqa_md_step`` + ``nqa_md_bath``), so a step moves nothing
to the host beyond what the force evaluation itself reads (``GraphedStep``: its two status flags).

One step, with ``F(t)`` the force at the positions of the start of the step and ``g = (3N + 1) kB T`` (3N + 1 degrees of freedom,
as the reference counts them)::

    a        = F(t)/m - xi v
    x(t+dt)  = x + dt v + dt^2/2 a
    v_half   = v + dt/2 a
    xi_half  = xi + dt/2 (sum m v^2 - g) / (2 Q)
    xi_new   = xi_half + dt/2 (sum m v_half^2 - g) / (2 Q)
    v(t+dt)  = (v_half + dt/2 F(t+dt)/m) / (1 + dt/2 xi_new)

The force is evaluated once per step: the last line is carried out by the launch of the NEXT step, with the force that step is
handed anyway, and ``velocities`` completes it into a buffer of its own when somebody asks.

Units are ASE's (eV, Angstrom, amu; time in ``units.fs``), so the model must give eV and eV/Angstrom.  Positions are not wrapped
into the cell, as in the reference: the device neighbour list wraps internally.

CPU tensors (and ``backend="aten"``) take an ATen form of the same equations, for any callable ``force_step``.

``Langevin`` is the stochastic NVT ensemble on the same state and the same two-launch step (``nqa_md_langevin_step`` +
``nqa_md_bath``): BAOAB with its noise made on the device by a counter-based generator, a function of (seed, step count,
component) alone (``langevin_noise``), so that a run is reproducible bit for bit, survives a checkpoint and captures into a
hipGraph.

``LangevinNPT`` is the isotropic constant-pressure ensemble for one system: the same Langevin launch, then a one-wavefront launch
that forms the pressure from the kinetic energy and the stress and rescales the cell on the device (stochastic cell rescaling,
``nqa_md_npt_bath``), then a flat launch that rescales positions and stored velocities (``nqa_md_npt_scale``).  The cell is a
device buffer that ``force_step(positions, cell)`` reads; a ``GraphedStep`` follows it through ``set_cell_from_device``.

Batches of independent systems: ``BatchedLangevin`` and ``BatchedLangevinNPT`` (``integrations/md_batched.py``).

Not provided: anisotropic cells and other barostats, a centre-of-mass constraint during the run, an
``ase.md.MolecularDynamics`` subclass.
"""

from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import numpy as np
import torch

from ..data import AtomicDataDict
from ._driver import (_M32, _det3, _philox_numpy, atoms_tensors, check_cells, checked_forces, checked_stress, select_backend,
                      state_arrays)

# CODATA 2014, the values behind ase.units
_e, _amu, _k = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
units = SimpleNamespace(kB=_k / _e, fs=1e-5 * math.sqrt(_e / _amu), GPa=1e-21 / _e, bar=1e-25 / _e)

_MD_FINISH_ONLY, _MD_THERMOSTAT = 1, 2
# the 8-byte words of nqa_md_state (include/nequip_amd.h)
_DT, _G, _Q, _XI, _EKIN, _NSTEPS, _FRESH, _EKIN_OBSERVED = range(8)


def maxwell_boltzmann_velocities(masses: torch.Tensor, temperature: float,
                                 generator: Optional[torch.Generator] = None) -> torch.Tensor:
    """Velocities ``[N, 3]`` (float64, on the device of ``masses``) drawn from the Maxwell-Boltzmann distribution at
    ``temperature`` (K): every component is normal with variance ``kB T / m``."""
    m = masses.detach().reshape(-1).to(torch.float64)
    where = generator.device if generator is not None else m.device
    xi = torch.randn(m.numel(), 3, dtype=torch.float64, device=where, generator=generator).to(m.device)
    return xi * torch.sqrt(units.kB * float(temperature) / m)[:, None]


def _sqrt(t: torch.Tensor) -> torch.Tensor:
    """The square root, correctly rounded.  ATen's vectorised float64 square root on the CPU is off by an ulp for some
    arguments; numpy's is IEEE's, as is the device's."""
    if t.device.type == "cpu":
        return torch.from_numpy(np.sqrt(t.detach().numpy()))
    return torch.sqrt(t)


def _remove_drift(pos: torch.Tensor, vel: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """``vel`` without centre-of-mass momentum and without angular momentum about the centre of mass (float64)."""
    mc = m[:, None]
    total = m.sum()
    vel = vel - (mc * vel).sum(0) / total
    r = pos - (mc * pos).sum(0) / total
    ang = torch.linalg.cross(r, mc * vel).sum(0)
    inertia = (m * (r * r).sum(1)).sum() * torch.eye(3, dtype=torch.float64, device=pos.device) - (mc * r).T @ r
    # a 3 x 3 system, once: solved on the host (a single atom or collinear atoms have a singular tensor: no rotation to remove)
    inertia_h, ang_h = inertia.cpu().numpy(), ang.cpu().numpy()
    eig = np.linalg.eigvalsh(inertia_h)
    if not (eig[0] > 1e-12 * max(eig[2], 1e-300)):
        return vel
    omega = torch.as_tensor(np.linalg.solve(inertia_h, ang_h)).to(pos.device)
    return vel - torch.linalg.cross(omega.expand_as(r), r)


def _graphed_step_for(atoms, model, device, r_max, chemical_symbols, outputs=None):
    """A ``GraphedStep`` for the species, cell and periodicity of ``atoms`` (the species mapping of ``NequIPCalculator``);
    ``outputs``: the fields it keeps (default: its own, energy and forces)."""
    from .graphed_step import GraphedStep

    if r_max is None:
        raise ValueError("from_atoms builds a GraphedStep around a model: pass r_max")
    pbc = tuple(bool(b) for b in np.asarray(atoms.get_pbc(), dtype=bool).reshape(3))
    if not any(pbc):
        raise ValueError("a GraphedStep needs a periodic cell: pass a force_step of your own for a molecule")
    type_names = list(getattr(model, "type_names", []) or [])
    if chemical_symbols is None:
        chemical_symbols = type_names
    if isinstance(chemical_symbols, dict):
        type_of = {sym: type_names.index(name) for sym, name in chemical_symbols.items()}
    else:
        type_of = {sym: i for i, sym in enumerate(chemical_symbols)}
    symbols = atoms.get_chemical_symbols()
    try:
        types = np.fromiter((type_of[s] for s in symbols), dtype=np.int64, count=len(symbols))
    except KeyError as e:
        raise ValueError(f"chemical species {e.args[0]!r} is not among the model's types {sorted(type_of)}") from None
    cell = np.asarray(atoms.get_cell(), dtype=np.float64).reshape(3, 3)
    kwargs = {} if outputs is None else {"outputs": tuple(outputs)}
    return GraphedStep(model, torch.as_tensor(types).to(device), torch.as_tensor(cell).to(device), pbc, float(r_max), **kwargs)


def _cell_following_step(force_step):
    """``force_step`` as a ``(positions, cell buffer)`` callable.  A ``GraphedStep`` takes the cell through its own buffers
    (``set_cell_from_device``) before every evaluation and must keep the stress; any other callable is returned as it is."""
    if not hasattr(force_step, "set_cell_from_device"):
        return force_step
    graphed = force_step
    if AtomicDataDict.STRESS_KEY not in getattr(graphed, "outputs", ()):
        raise ValueError("stress: the GraphedStep must be built with outputs=(total_energy, forces, stress)")

    def step(pos, cell_buffer, _step=graphed):
        _step.set_cell_from_device(cell_buffer)
        return _step(pos)

    step.device = getattr(graphed, "device", None)
    step.graphed_step = graphed
    return step


class _DeviceMD:
    """What the drivers share: the checks of the constructor's arguments, the buffers, the force evaluation and the interface.
    A driver adds its record (``_write_state``), the two forms of its step (``_launch``, ``_aten_finished`` + ``_aten_step``)
    and its checkpoints."""

    def _check_system(self, force_step, masses, positions, velocities, timestep) -> None:
        if not callable(force_step):
            raise TypeError("force_step must be callable: positions [N, 3] -> {'forces', 'total_energy'}")
        if not (isinstance(masses, torch.Tensor) and isinstance(positions, torch.Tensor)):
            raise TypeError("masses and positions must be tensors")
        if positions.dim() != 2 or positions.shape[1] != 3:
            raise ValueError(f"positions must have shape [N, 3], got {tuple(positions.shape)}")
        n = int(positions.shape[0])
        if n == 0:
            raise ValueError("no atoms: positions has N == 0")
        if tuple(masses.shape) != (n,):
            raise ValueError(f"masses must have shape [{n}] to match positions, got {tuple(masses.shape)}")
        if velocities is not None and tuple(velocities.shape) != (n, 3):
            raise ValueError(f"velocities must have shape [{n}, 3] to match positions, got {tuple(velocities.shape)}")
        device = positions.device
        for name, t in (("masses", masses), ("velocities", velocities)):
            if t is not None and t.device != device:
                raise ValueError(f"mixed devices: positions on {device}, {name} on {t.device}")
        step_device = getattr(force_step, "device", None)
        if isinstance(step_device, torch.device) and step_device != device:
            raise ValueError(f"mixed devices: positions on {device}, force_step on {step_device}")
        if not bool((masses > 0).all()) or not bool(torch.isfinite(masses).all()):
            raise ValueError("masses must be positive and finite")
        if not (timestep > 0.0 and math.isfinite(timestep)):
            raise ValueError("timestep must be positive")

    def _setup(self, force_step, masses, positions, velocities, remove_drift, backend) -> None:
        """The backend, the buffers and, on the kernel path, the partial sums and the ``nqa_md_state`` record."""
        device, n = positions.device, int(positions.shape[0])
        self._hip = select_backend(backend, device)
        self.force_step = force_step
        self.device = device
        self.num_atoms = n
        self._m = masses.detach().to(torch.float64).contiguous().clone()
        self._pos = positions.detach().to(torch.float64).contiguous().clone()
        vel = torch.zeros_like(self._pos) if velocities is None else velocities.detach().to(torch.float64)
        if remove_drift:
            vel = _remove_drift(self._pos, vel, self._m)
        self._vel = vel.contiguous().clone()  # v(t) while `fresh`, the half-step velocities between two steps
        self._vel_out = torch.empty_like(self._vel)
        self._out: Dict[str, torch.Tensor] = {}
        self._forces: Optional[torch.Tensor] = None
        if self._hip:
            from .. import _lib

            self._lib = _lib
            lib = _lib.load()
            self._n_partials = int(lib.nqa_md_num_partials(n))
            self._partials = torch.zeros(2 * self._n_partials, dtype=torch.float64, device=device)
            self._partials_observed = torch.zeros_like(self._partials)
            self._rec = torch.zeros(8, dtype=torch.float64, device=device)
            self._rec_i = self._rec.view(torch.int64)
        else:
            self._ekin = torch.zeros((), dtype=torch.float64, device=device)
            self._fresh = True
            self._nsteps = 0

    def _evaluate(self) -> None:
        out = self.force_step(self._pos)
        self._out, self._forces = out, checked_forces(out, self.num_atoms, self.device)

    def set_timestep(self, timestep: float) -> None:
        """The time step from the next step on.  The step that is under way is completed with the step it began with."""
        if not (timestep > 0.0 and math.isfinite(timestep)):
            raise ValueError("timestep must be positive")
        self._vel.copy_(self.velocities)
        self._dt = float(timestep)
        if self._hip:
            self._rec_i[_FRESH:_FRESH + 1].fill_(1)
            self._rec[_DT:_DT + 1].fill_(self._dt)
        else:
            self._fresh = True

    # ---- interface ----------------------------------------------------------------------------------------------------------
    def step(self) -> None:
        """One MD step: two launches, then one force evaluation at the new positions."""
        if self._hip:
            self._launch(finish_only=False)
        else:
            self._aten_step()
        self._evaluate()

    def run(self, n: int) -> None:
        for _ in range(int(n)):
            self.step()

    @property
    def positions(self) -> torch.Tensor:
        return self._pos

    @property
    def forces(self) -> torch.Tensor:
        return self._forces

    @property
    def masses(self) -> torch.Tensor:
        return self._m

    @property
    def velocities(self) -> torch.Tensor:
        """The completed velocities ``v(t)`` at the current positions; leaves the trajectory alone."""
        if self._hip:
            self._launch(finish_only=True, bath=False)
        else:
            self._vel_out.copy_(self._aten_finished())
        return self._vel_out

    @property
    def kinetic_energy(self) -> float:
        """``1/2 sum m v(t)^2`` of the completed velocities at the current positions (eV)."""
        if self._hip:
            self._launch(finish_only=True)
            return float(self._rec[_EKIN_OBSERVED])
        v = self._aten_finished()
        return float(0.5 * (self._m[:, None] * v * v).sum())

    @property
    def temperature(self) -> float:
        return 2.0 * self.kinetic_energy / (3 * self.num_atoms * units.kB)

    @property
    def potential_energy(self) -> float:
        return float(self._out[AtomicDataDict.TOTAL_ENERGY_KEY].detach().reshape(-1)[0])

    @property
    def nsteps(self) -> int:
        return int(self._rec_i[_NSTEPS]) if self._hip else self._nsteps

    # ---- Atoms --------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model_or_step, *args, device="cuda", r_max: Optional[float] = None, chemical_symbols=None,
                   **kwargs):
        """The driver for an ``Atoms`` object (positions, velocities, masses, cell, periodicity, species); ``args`` and
        ``kwargs`` are the constructor's between ``masses`` and ``positions`` (``timestep, temperature, nvt_q``, or ``friction``
        for ``Langevin``) and after ``velocities``.  ``model_or_step``: an eval-mode model (``torch.nn.Module`` with ``type_names``; a ``GraphedStep`` is
        built around it, which needs a periodic cell and ``r_max``) or a ready ``force_step``.  ``chemical_symbols``: as for
        ``NequIPCalculator``."""
        device = torch.device(device)
        pos, vel, masses = atoms_tensors(atoms, device, "positions", "velocities", "masses")
        step = model_or_step
        if isinstance(model_or_step, torch.nn.Module):
            step = _graphed_step_for(atoms, model_or_step, device, r_max, chemical_symbols)
        return cls(step, masses, *args, positions=pos, velocities=vel, **kwargs)

    def write_back(self, atoms) -> None:
        """Positions and completed velocities into ``atoms`` (one copy each)."""
        atoms.set_positions(self._pos.detach().cpu().numpy())
        atoms.set_velocities(self.velocities.detach().cpu().numpy())


class NoseHoover(_DeviceMD):
    """Nose-Hoover NVT dynamics of a fixed set of atoms, state on the device of ``positions``.

    ``force_step``: a ``GraphedStep`` or any callable ``pos [N, 3] -> {"forces": [N, 3], "total_energy": ...}`` (float32 or
    float64 forces, eV/Angstrom; all tensors on the device of ``positions``).  ``masses`` ``[N]`` in amu, ``timestep`` in ASE's
    time unit (``0.5 * units.fs``), ``temperature`` in K, ``nvt_q`` the bath's inertia ``Q``.  ``velocities`` default to zero.
    ``remove_drift``: once, here, centre-of-mass momentum and angular momentum are set to zero (the reference does this in its
    constructor).  ``thermostat=False``: the bath variable stays 0, i.e. velocity Verlet.
    ``backend``: ``"hip"`` (the kernels; the default on the GPU), ``"aten"`` (the default on the CPU).

    ``positions`` and ``forces`` are the live tensors (``forces`` is what ``force_step`` returned last: a ``GraphedStep``
    overwrites it at the next step).  ``velocities`` are the completed ``v(t)`` in a buffer that the next read overwrites.
    The scalar properties copy one value to the host; ``step`` and ``run`` read nothing themselves."""

    def __init__(self, force_step: Callable[[torch.Tensor], Dict[str, torch.Tensor]], masses: torch.Tensor, timestep: float,
                 temperature: float, nvt_q: float, positions: torch.Tensor, velocities: Optional[torch.Tensor] = None,
                 thermostat: bool = True, remove_drift: bool = True, backend: str = "auto"):
        self._check_system(force_step, masses, positions, velocities, timestep)
        if thermostat and not (nvt_q > 0.0 and temperature >= 0.0):
            raise ValueError("the thermostat needs nvt_q > 0 and temperature >= 0")
        self.thermostat = bool(thermostat)
        self._temperature = float(temperature)
        self._dt, self._q = float(timestep), float(nvt_q)
        self._setup(force_step, masses, positions, velocities, remove_drift, backend)
        if self._hip:
            self._mode = _MD_THERMOSTAT if self.thermostat else 0
        else:
            self._xi = torch.zeros((), dtype=torch.float64, device=self.device)
        self._write_state(xi=0.0, nsteps=0)
        self._evaluate()

    # ---- state -------------------------------------------------------------------------------------------------------------
    def _g(self) -> float:
        return (3 * self.num_atoms + 1) * units.kB * self._temperature

    def _write_state(self, xi: float, nsteps: int) -> None:
        """The whole record, with ``velocities`` taken as completed."""
        if self._hip:
            words = torch.tensor([self._dt, self._g(), self._q, float(xi), 0.0, 0.0, 0.0, 0.0], dtype=torch.float64)
            words.view(torch.int64)[_NSTEPS] = int(nsteps)
            words.view(torch.int64)[_FRESH] = 1
            self._rec.copy_(words)
        else:
            self._xi.fill_(float(xi))
            self._fresh, self._nsteps = True, int(nsteps)

    def set_temperature(self, temperature: float) -> None:
        """The bath's target from the next step on; written in place, nothing is read back."""
        self._temperature = float(temperature)
        if self._hip:
            self._rec[_G:_G + 1].fill_(self._g())

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch(self, finish_only: bool, bath: bool = True) -> None:
        lib, L = self._lib.load(), self._lib
        f = self._forces
        mode = self._mode | (_MD_FINISH_ONLY if finish_only else 0)
        partials = self._partials_observed if finish_only else self._partials
        stream = L.stream_ptr(self.device)
        L.check(lib.nqa_md_step(L.NQA_F64 if f.dtype == torch.float64 else L.NQA_F32, L.ptr(f), L.ptr(self._m), L.ptr(self._pos),
                                L.ptr(self._vel), L.ptr(self._vel_out), self.num_atoms, L.ptr(self._rec), L.ptr(partials), mode,
                                stream), "nqa_md_step")
        if bath:
            L.check(lib.nqa_md_bath(L.ptr(partials), self._n_partials, L.ptr(self._rec), mode, stream), "nqa_md_bath")

    def _aten_finished(self) -> torch.Tensor:
        if self._fresh:
            return self._vel
        hdt = 0.5 * self._dt
        fm = self._forces.to(torch.float64) / self._m[:, None]
        return (self._vel + hdt * fm) / (1.0 + hdt * self._xi)

    def _aten_step(self) -> None:
        dt, hdt, mc = self._dt, 0.5 * self._dt, self._m[:, None]
        v = self._aten_finished()
        a = self._forces.to(torch.float64) / mc - self._xi * v
        self._pos.copy_(self._pos + dt * v + (0.5 * (dt * dt)) * a)
        vh = v + hdt * a
        s_full, s_half = (mc * v * v).sum(), (mc * vh * vh).sum()
        if self.thermostat:
            g, q = self._g(), self._q
            xi_half = self._xi + hdt * (0.5 * (s_full - g)) / q
            self._xi = xi_half + hdt * (0.5 * (s_half - g)) / q
        self._ekin = 0.5 * s_full
        self._vel.copy_(vh)
        self._fresh = False
        self._nsteps += 1

    @property
    def nvt_bath(self) -> float:
        return float(self._rec[_XI]) if self._hip else float(self._xi)

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        return {"positions": self._pos.detach().clone(), "velocities": self.velocities.detach().clone(), "nvt_bath": self.nvt_bath,
                "nsteps": self.nsteps, "timestep": self._dt, "temperature": self._temperature, "nvt_q": self._q,
                "thermostat": self.thermostat}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        pos, vel = state_arrays(state, self.num_atoms)
        if "nvt_bath" not in state or "friction" in state:
            raise ValueError("the state was not saved by a Nose-Hoover / velocity-Verlet run (a Langevin state has no nvt_bath)")
        if bool(state["thermostat"]) != self.thermostat:
            raise ValueError("the state was saved with the thermostat " + ("on" if state["thermostat"] else "off"))
        self._pos.copy_(pos)
        self._vel.copy_(vel)
        self._dt, self._temperature, self._q = float(state["timestep"]), float(state["temperature"]), float(state["nvt_q"])
        self._write_state(xi=float(state["nvt_bath"]), nsteps=int(state["nsteps"]))
        self._evaluate()


class VelocityVerlet(NoseHoover):
    """Velocity Verlet (NVE): ``NoseHoover`` with the thermostat off."""

    def __init__(self, force_step, masses: torch.Tensor, timestep: float, positions: torch.Tensor,
                 velocities: Optional[torch.Tensor] = None, remove_drift: bool = True, backend: str = "auto"):
        super().__init__(force_step, masses, timestep, 0.0, 1.0, positions, velocities, thermostat=False,
                         remove_drift=remove_drift, backend=backend)


# ---- Langevin dynamics ---------------------------------------------------------------------------------------------------------
# the 8-byte words of nqa_md_langevin_params (include/nequip_amd.h)
_C1, _C2, _KT, _SEED = range(4)


def _check_u64(name: str, value) -> int:
    if isinstance(value, bool) or not isinstance(value, (int, np.integer)) or not (0 <= int(value) < 2 ** 64):
        raise ValueError(f"{name} must be an integer in [0, 2^64), got {value!r}")
    return int(value)


def _normals_numpy(words: np.ndarray) -> np.ndarray:
    """Box-Muller on two 53-bit uniforms, ``u1`` in (0, 1] and ``u2`` in [0, 1); the second normal is dropped."""
    w = [(words[:, k] >> np.uint64(5 + k % 2)).astype(np.float64) for k in range(4)]
    u1 = (w[0] * 67108864.0 + w[1] + 1.0) * 2.0 ** -53
    u2 = (w[2] * 67108864.0 + w[3]) * 2.0 ** -53
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def langevin_noise(seed: int, step: int, count: int, device="cpu", *, backend: str = "auto", return_words: bool = False):
    """The standard normals ``[count]`` (float64, on ``device``) that ``Langevin`` with ``seed`` draws at step ``step`` for the
    flat components ``0 .. count - 1`` (component ``i`` of atom ``i // 3``), a function of these three numbers alone::

        (w0, w1, w2, w3) = philox4x32_10(counter=(i & 0xffffffff, i >> 32, step & 0xffffffff, step >> 32),
                                         key=(seed & 0xffffffff, seed >> 32))
        u1 = ((w0 >> 5) * 2^26 + (w1 >> 6) + 1) * 2^-53;  u2 = ((w2 >> 5) * 2^26 + (w3 >> 6)) * 2^-53
        z  = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2)

    ``backend``: ``"hip"`` (``nqa_md_noise``, the default on the GPU) or ``"aten"`` (numpy ``uint64`` on the host, uploaded).
    The Philox words of the two are the same bits; the normals differ by the ``log`` and ``cos`` of the two libraries, a few
    ulp.  ``return_words``: also the words, ``[count, 4]`` int64 with values below 2^32."""
    seed, step = _check_u64("seed", seed), _check_u64("step", step)
    count, device = int(count), torch.device(device)
    if count < 0:
        raise ValueError(f"count must not be negative, got {count}")
    if backend not in ("auto", "hip", "aten"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'aten', got {backend!r}")
    if backend == "hip" and device.type != "cuda":
        raise ValueError("backend='hip' needs a GPU device: the kernel runs there")
    if count > 0 and (backend == "hip" or (backend == "auto" and device.type == "cuda")):
        from .. import _lib as L

        z = torch.empty(count, dtype=torch.float64, device=device)
        w = torch.empty(count, 4, dtype=torch.int32, device=device) if return_words else None
        with torch.cuda.device(device):
            L.check(L.load().nqa_md_noise(seed, step, count, L.ptr(w), L.ptr(z), L.stream_ptr(device)), "nqa_md_noise")
        return (z, w.to(torch.int64) & _M32) if return_words else z
    words = _philox_numpy(seed, step, np.arange(count, dtype=np.uint64))
    z = torch.from_numpy(_normals_numpy(words)).to(device)
    return (z, torch.from_numpy(words.astype(np.int64)).to(device)) if return_words else z


class Langevin(_DeviceMD):
    """Langevin NVT dynamics of a fixed set of atoms, state on the device of ``positions``: the BAOAB splitting of Leimkuhler
    and Matthews with one force evaluation per step.  With ``F`` the force at the start of the step, ``F'`` the one at the new
    positions and ``hdt = dt / 2``::

        B   v1 = v + hdt F/m
        A   x  = x + hdt v1
        O   v2 = c1 v1 + (c2 sqrt(kB T / m)) z      c1 = exp(-friction dt),  c2 = sqrt(1 - c1^2),  z ~ N(0, 1) per component
        A   x  = x + hdt v2
        B   v' = v2 + hdt F'/m

    The last line is carried out by the launch of the next step, as in ``NoseHoover``.  The noise is made on the device and is a
    function of ``(seed, step count, component)`` alone (``langevin_noise``): the same seed gives the same trajectory bit for
    bit, whatever is read in between, a reloaded ``state_dict`` continues bit for bit, and a captured pair of launches draws
    fresh noise at every replay, since the step count lives in the device record.

    ``force_step``, ``masses``, ``timestep``, ``temperature``, ``positions``, ``velocities``, ``backend`` and the properties: as
    for ``NoseHoover``.  ``friction`` in 1/time (``0.01 / units.fs``); ``friction=0`` is velocity Verlet.  ``seed``: an integer
    in [0, 2^64).  ``remove_drift``: once, here, centre-of-mass momentum and angular momentum are set to zero.  The centre of
    mass is NOT held fixed during the run (ASE's ``fixcm``): the noise moves it like any other degree of freedom."""

    def __init__(self, force_step: Callable[[torch.Tensor], Dict[str, torch.Tensor]], masses: torch.Tensor, timestep: float,
                 temperature: float, friction: float, positions: torch.Tensor, velocities: Optional[torch.Tensor] = None,
                 seed: int = 0, remove_drift: bool = False, backend: str = "auto"):
        self._check_system(force_step, masses, positions, velocities, timestep)
        self._check_temperature(temperature)
        self._check_friction(friction)
        self.seed = _check_u64("seed", seed)
        self.friction = float(friction)
        self._temperature = float(temperature)
        self._dt = float(timestep)
        self._setup(force_step, masses, positions, velocities, remove_drift, backend)
        if self._hip:
            self._par = torch.zeros(4, dtype=torch.float64, device=self.device)
            self._par_i = self._par.view(torch.int64)
        self._write_state(nsteps=0)
        self._evaluate()

    # ---- state -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_temperature(temperature) -> None:
        if not (temperature >= 0.0 and math.isfinite(temperature)):
            raise ValueError(f"temperature must be non-negative and finite, got {temperature!r}")

    @staticmethod
    def _check_friction(friction) -> None:
        if not (friction >= 0.0 and math.isfinite(friction)):
            raise ValueError(f"friction must be non-negative and finite, got {friction!r}")

    def _coefficients(self):
        """``c1`` and ``c2`` in the host's float64: the bits a restatement with ``math.exp`` and ``math.sqrt`` holds."""
        c1 = math.exp(-self.friction * self._dt)
        return c1, math.sqrt(1.0 - c1 * c1)

    def _write_params(self) -> None:
        self._c1, self._c2 = self._coefficients()
        self._kt = units.kB * self._temperature
        if self._hip:
            self._par[_C1:_C1 + 1].fill_(self._c1)
            self._par[_C2:_C2 + 1].fill_(self._c2)
            self._par[_KT:_KT + 1].fill_(self._kt)
            self._par_i[_SEED:_SEED + 1].fill_(self.seed - 2 ** 64 if self.seed >= 2 ** 63 else self.seed)  # (the same 64 bits)

    def _write_state(self, nsteps: int) -> None:
        """Both records, with ``velocities`` taken as completed."""
        if self._hip:
            words = torch.zeros(8, dtype=torch.float64)
            words[_DT] = self._dt
            words.view(torch.int64)[_NSTEPS] = int(nsteps)
            words.view(torch.int64)[_FRESH] = 1
            self._rec.copy_(words)
        else:
            self._fresh, self._nsteps = True, int(nsteps)
        self._write_params()

    def set_temperature(self, temperature: float) -> None:
        """The target from the next step on; ``kB T`` is written in place, nothing is read back."""
        self._check_temperature(temperature)
        self._temperature = float(temperature)
        self._write_params()

    def set_friction(self, friction: float) -> None:
        """The friction (1/time) from the next step on; ``c1`` and ``c2`` are written in place."""
        self._check_friction(friction)
        self.friction = float(friction)
        self._write_params()

    def set_timestep(self, timestep: float) -> None:
        """The time step from the next step on, ``c1`` and ``c2`` with it.  The step that is under way is completed with the
        step it began with."""
        super().set_timestep(timestep)
        self._write_params()

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch(self, finish_only: bool, bath: bool = True) -> None:
        lib, L = self._lib.load(), self._lib
        f = self._forces
        mode = _MD_FINISH_ONLY if finish_only else 0
        partials = self._partials_observed if finish_only else self._partials
        stream = L.stream_ptr(self.device)
        L.check(lib.nqa_md_langevin_step(L.NQA_F64 if f.dtype == torch.float64 else L.NQA_F32, L.ptr(f), L.ptr(self._m),
                                         L.ptr(self._pos), L.ptr(self._vel), L.ptr(self._vel_out), self.num_atoms,
                                         L.ptr(self._rec), L.ptr(self._par), L.ptr(partials), mode, stream),
                "nqa_md_langevin_step")
        if bath:
            L.check(lib.nqa_md_bath(L.ptr(partials), self._n_partials, L.ptr(self._rec), mode, stream), "nqa_md_bath")

    def _aten_finished(self) -> torch.Tensor:
        if self._fresh:
            return self._vel
        hdt = 0.5 * self._dt
        fm = self._forces.to(torch.float64) / self._m[:, None]
        return self._vel + hdt * fm

    def _aten_step(self) -> None:
        hdt, mc = 0.5 * self._dt, self._m[:, None]
        v = self._aten_finished()
        fm = self._forces.to(torch.float64) / mc
        z = langevin_noise(self.seed, self._nsteps, 3 * self.num_atoms, self.device, backend="aten").reshape(-1, 3)
        v1 = v + hdt * fm
        x = self._pos + hdt * v1
        # (a true division: `float / tensor` is the tensor's reciprocal times the float, which rounds twice)
        v2 = self._c1 * v1 + (self._c2 * _sqrt(torch.full_like(mc, self._kt) / mc)) * z
        self._pos.copy_(x + hdt * v2)
        self._ekin = 0.5 * (mc * v * v).sum()
        self._vel.copy_(v2)
        self._fresh = False
        self._nsteps += 1

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        return {"positions": self._pos.detach().clone(), "velocities": self.velocities.detach().clone(), "nsteps": self.nsteps,
                "timestep": self._dt, "temperature": self._temperature, "friction": self.friction, "seed": self.seed}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        pos, vel = state_arrays(state, self.num_atoms)
        if "friction" not in state or "seed" not in state or "nvt_bath" in state:
            raise ValueError("the state was not saved by a Langevin run (a Nose-Hoover state has no friction and no seed)")
        self._pos.copy_(pos)
        self._vel.copy_(vel)
        self._dt, self._temperature = float(state["timestep"]), float(state["temperature"])
        self.friction, self.seed = float(state["friction"]), _check_u64("seed", state["seed"])
        self._write_state(nsteps=int(state["nsteps"]))
        self._evaluate()


# ---- constant pressure ---------------------------------------------------------------------------------------------------------
# the 8-byte words of nqa_md_npt_state (include/nequip_amd.h)
_NPT_A, _NPT_P0, _NPT_INDEX, _NPT_MU, _NPT_P, _NPT_EKIN, _NPT_VOLUME, _NPT_FAILED = range(8)


def _aten_barostat(ekin, cell, stress, xi, a, p0, kT):
    """The stochastic cell rescaling of ``LangevinNPT`` over ``[S]`` systems in ATen: ``(mu, p, bad)`` from the kinetic
    energies, the cells and stresses ``[S, 3, 3]``, one normal each and the ``[S]`` float64 tensors ``a``, ``p0``, ``kB T``."""
    vol = _det3(cell).abs()
    three = torch.full_like(vol, 3.0)  # (tensor divisors: a true division on every device)
    p = (2.0 * ekin) / (3.0 * vol) - (stress[:, 0, 0] + stress[:, 1, 1] + stress[:, 2, 2]) / three
    d_eps = -a * (p0 - p) + torch.sqrt((2.0 * kT * a) / vol) * xi
    mu = torch.exp(d_eps / three)
    bad = ~torch.isfinite(mu) | ~(vol > 0.0)
    return torch.where(bad, torch.ones_like(mu), mu), p, bad


class LangevinNPT(Langevin):
    """Isotropic NPT dynamics of one system, state and cell on the device of ``positions``: the BAOAB step of ``Langevin``
    followed by a stochastic cell rescaling barostat (Bernetti and Bussi, J. Chem. Phys. 153, 114107, 2020), which is first order
    in the volume and samples the isothermal-isobaric ensemble.  It shares ``kB T`` and the noise generator with the thermostat.
    With ``F`` the force and ``sigma`` the stress at the positions ``x`` and the cell ``C`` (rows are the lattice vectors) of the
    start of the step, ``s`` the count of completed steps and ``a = compressibility dt / taup``::

        x', v2 = the B, A, O, A of ``Langevin`` (the closing B is deferred to the next step, as there)
        K      = 1/2 sum m v^2 over the completed velocities;  V = |det C|
        P      = (2 K) / (3 V) - (sigma_00 + sigma_11 + sigma_22) / 3
        xi     = langevin_noise(seed, s, 3N + 1)[3N]            (one past the atoms' components: independent of their noise)
        d_eps  = -a (p0 - P) + sqrt((2 kB T a) / V) xi;  mu = exp(d_eps / 3)
        C      = mu C;  x = mu x';  v2 = v2 / mu

    then ``force_step`` at the new ``(x, C)``.  The pressure that drives a step is the one of its start, applied after the move:
    the force is evaluated once per step, and ``taup >> dt``.  ``compressibility = 0`` gives ``mu = 1`` exactly, the trajectory of
    ``Langevin`` with the same seed bit for bit.  A ``mu`` that is not finite or a cell without volume leaves ``mu = 1`` and sets
    a flag in the device record; the next read of ``nsteps``, ``pressure`` or ``volume`` raises ``RuntimeError``.

    Three HIP launches (``csrc/md.hip``: ``nqa_md_langevin_step`` + ``nqa_md_npt_bath`` + ``nqa_md_npt_scale``); the second writes
    ``C`` into ``cell``, the ``[1, 3, 3]`` float64 buffer that ``force_step`` is handed at every call, so nothing of a step passes
    through the host.

    ``force_step``: ``(positions [N, 3], cell [1, 3, 3]) -> {"forces", "total_energy", "stress"}`` (the stress ``[3, 3]`` or
    ``[1, 3, 3]``, float32 or float64, ``(1/V) dE/d(strain)``: ASE's sign, what ``CellFIRE`` takes), or a ``GraphedStep`` built
    with ``outputs=(total_energy, forces, stress)`` in a fully periodic cell (its cell is set by ``set_cell_from_device``).
    ``pressure``: the target ``p0`` in eV/A^3 (``1.0 * units.bar``); ``compressibility`` in A^3/eV (``4.57e-5 / units.bar`` for
    water); ``taup`` in time units.  The other arguments and the interface are those of ``Langevin``; added are ``cell`` (the
    live buffer), ``volume``, ``pressure`` (the ``P`` of the last step; 0 before the first), ``stress``, ``target_pressure``,
    ``set_pressure`` and ``set_barostat``.

    Not provided: anisotropic or semi-isotropic cells, Nose-Hoover / MTK barostats (batches of systems:
    ``BatchedLangevinNPT``)."""

    def __init__(self, force_step, masses: torch.Tensor, timestep: float, temperature: float, friction: float, pressure: float,
                 compressibility: float, taup: float, positions: torch.Tensor, cell: torch.Tensor,
                 velocities: Optional[torch.Tensor] = None, seed: int = 0, remove_drift: bool = False, backend: str = "auto"):
        if hasattr(force_step, "set_cell_from_device") and not all(getattr(force_step, "_pbc", (True,) * 3)):
            raise ValueError("NPT around a GraphedStep needs all three directions periodic")
        force_step = _cell_following_step(force_step)
        self._check_system(force_step, masses, positions, velocities, timestep)
        self._check_temperature(temperature)
        self._check_friction(friction)
        self._check_pressure(pressure)
        self._check_barostat(compressibility, taup)
        if not isinstance(cell, torch.Tensor) or tuple(cell.shape) not in ((3, 3), (1, 3, 3)):
            raise ValueError("cell must be a tensor of shape [3, 3] or [1, 3, 3], got "
                             f"{tuple(cell.shape) if isinstance(cell, torch.Tensor) else type(cell).__name__}")
        if cell.device != positions.device:
            raise ValueError(f"mixed devices: positions on {positions.device}, cell on {cell.device}")
        check_cells(cell, single=True)
        self.seed = _check_u64("seed", seed)
        self.friction = float(friction)
        self._temperature = float(temperature)
        self._dt = float(timestep)
        self._p0, self.compressibility, self.taup = float(pressure), float(compressibility), float(taup)
        self._setup(force_step, masses, positions, velocities, remove_drift, backend)
        self._cell = cell.detach().to(torch.float64).reshape(1, 3, 3).contiguous().clone()
        self._stress: Optional[torch.Tensor] = None
        if self._hip:
            self._par = torch.zeros(4, dtype=torch.float64, device=self.device)
            self._par_i = self._par.view(torch.int64)
            self._npt = torch.zeros(8, dtype=torch.float64, device=self.device)
            self._npt_i = self._npt.view(torch.int64)
        self._write_state(nsteps=0)
        self._evaluate()

    # ---- state -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_pressure(pressure) -> None:
        if not (isinstance(pressure, (int, float)) and math.isfinite(pressure)):
            raise ValueError(f"pressure must be finite, got {pressure!r}")

    @staticmethod
    def _check_barostat(compressibility, taup) -> None:
        if not (compressibility >= 0.0 and math.isfinite(compressibility)):
            raise ValueError(f"compressibility must be non-negative and finite, got {compressibility!r}")
        if not (taup > 0.0 and math.isfinite(taup)):
            raise ValueError(f"taup must be positive and finite, got {taup!r}")

    def _write_params(self) -> None:
        """The thermostat's record and the two words of the barostat's that the host owns beside the noise index."""
        super()._write_params()
        self._a = self.compressibility * self._dt / self.taup
        if self._hip:
            self._npt[_NPT_A:_NPT_A + 1].fill_(self._a)
            self._npt[_NPT_P0:_NPT_P0 + 1].fill_(self._p0)

    def _write_state(self, nsteps: int) -> None:
        """All three records, with ``velocities`` taken as completed, ``mu = 1`` and the flag cleared."""
        super()._write_state(nsteps)
        if self._hip:
            words = torch.zeros(8, dtype=torch.float64)
            words[_NPT_A], words[_NPT_P0], words[_NPT_MU] = self._a, self._p0, 1.0
            words.view(torch.int64)[_NPT_INDEX] = 3 * self.num_atoms
            self._npt.copy_(words)
        else:
            self._mu = torch.ones((), dtype=torch.float64, device=self.device)
            self._pressure = torch.zeros((), dtype=torch.float64, device=self.device)
            self._failed = torch.zeros((), dtype=torch.bool, device=self.device)

    def set_pressure(self, pressure: float) -> None:
        """The target pressure (eV/A^3) from the next step on; written in place, nothing is read back."""
        self._check_pressure(pressure)
        self._p0 = float(pressure)
        self._write_params()

    def set_barostat(self, compressibility: float, taup: float) -> None:
        """Compressibility (A^3/eV) and relaxation time from the next step on; ``a`` is written in place."""
        self._check_barostat(compressibility, taup)
        self.compressibility, self.taup = float(compressibility), float(taup)
        self._write_params()

    def _evaluate(self) -> None:
        out = self.force_step(self._pos, self._cell)
        stress = checked_stress(out, 1, self.device, "[3, 3] or [1, 3, 3]", "([3, 3] or [1, 3, 3]) next to the forces for NPT")
        self._out, self._forces, self._stress = out, checked_forces(out, self.num_atoms, self.device), stress.reshape(3, 3)

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch(self, finish_only: bool, bath: bool = True) -> None:
        if finish_only:
            return super()._launch(finish_only, bath)
        super()._launch(False, bath=False)
        lib, L = self._lib.load(), self._lib
        sig = self._stress
        stream = L.stream_ptr(self.device)
        L.check(lib.nqa_md_npt_bath(L.ptr(self._partials), self._n_partials, L.ptr(self._rec), L.ptr(self._par), L.ptr(self._npt),
                                    L.NQA_F64 if sig.dtype == torch.float64 else L.NQA_F32, L.ptr(sig), L.ptr(self._cell),
                                    stream), "nqa_md_npt_bath")
        L.check(lib.nqa_md_npt_scale(L.ptr(self._pos), L.ptr(self._vel), self.num_atoms, L.ptr(self._npt), stream),
                "nqa_md_npt_scale")

    def _aten_step(self) -> None:
        step, sig, n3 = self._nsteps, self._stress.to(torch.float64), 3 * self.num_atoms
        super()._aten_step()
        xi = _normals_numpy(_philox_numpy(self.seed, step, n3))
        one = lambda value: torch.as_tensor(value, dtype=torch.float64).reshape(1).to(self.device)  # noqa: E731
        mu, p, bad = (t[0] for t in _aten_barostat(self._ekin.reshape(1), self._cell, sig.reshape(1, 3, 3), one(xi), one(self._a),
                                                   one(self._p0), one(self._kt)))
        self._failed = self._failed | bad
        self._cell.copy_(mu * self._cell)
        self._pos.copy_(mu * self._pos)
        self._vel.copy_(self._vel / mu)
        self._mu, self._pressure = mu, p

    # ---- interface ----------------------------------------------------------------------------------------------------------
    def _check_failed(self, failed: bool) -> None:
        if failed:
            raise RuntimeError("the barostat met a scaling factor that is not finite or a cell without volume: the run is invalid "
                               "from that step on (smaller compressibility / taup or time step)")

    @property
    def nsteps(self) -> int:
        self._check_failed(bool(self._npt_i[_NPT_FAILED]) if self._hip else bool(self._failed))
        return super().nsteps

    @property
    def cell(self) -> torch.Tensor:
        """``[1, 3, 3]`` float64, rows are the lattice vectors: the live buffer that ``force_step`` reads."""
        return self._cell

    @property
    def stress(self) -> torch.Tensor:
        """``[3, 3]``: the stress ``force_step`` returned last, at the current positions and cell."""
        return self._stress

    @property
    def target_pressure(self) -> float:
        return self._p0

    @property
    def pressure(self) -> float:
        """The ``P`` that drove the last step (eV/A^3; kinetic plus potential part, at the start of that step); one copy."""
        if self._hip:
            words = self._npt[_NPT_P:].cpu()
            self._check_failed(bool(words.view(torch.int64)[_NPT_FAILED - _NPT_P]))
            return float(words[0])
        self._check_failed(bool(self._failed))
        return float(self._pressure)

    @property
    def volume(self) -> float:
        """``|det C|`` of the current cell (A^3)."""
        self._check_failed(bool(self._npt_i[_NPT_FAILED]) if self._hip else bool(self._failed))
        return float(_det3(self._cell).abs())

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        state = super().state_dict()
        state.update({"cell": self._cell.detach().clone(), "pressure": self._p0, "compressibility": self.compressibility,
                      "taup": self.taup})
        return state

    def load_state_dict(self, state: Dict[str, object]) -> None:
        if "compressibility" not in state or "cell" not in state:
            raise ValueError("the state was not saved by a LangevinNPT run (it holds no cell and no barostat)")
        cell = state["cell"]
        if tuple(cell.shape) != (1, 3, 3):
            raise ValueError(f"the state holds a cell of shape {tuple(cell.shape)}, this run has one system ([1, 3, 3])")
        if tuple(state["positions"].shape) != (self.num_atoms, 3) or "friction" not in state or "seed" not in state:
            raise ValueError(f"the state was not saved by a LangevinNPT run of {self.num_atoms} atoms")
        self._check_pressure(state["pressure"])
        self._check_barostat(state["compressibility"], state["taup"])
        check_cells(cell, single=True)
        self._cell.copy_(cell)
        self._p0 = float(state["pressure"])
        self.compressibility, self.taup = float(state["compressibility"]), float(state["taup"])
        super().load_state_dict(state)

    # ---- Atoms --------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model_or_step, *args, device="cuda", r_max: Optional[float] = None, chemical_symbols=None,
                   **kwargs):
        """The driver for an ``Atoms`` object (positions, velocities, masses, cell, periodicity, species); ``args`` and
        ``kwargs`` are the constructor's between ``masses`` and ``positions`` (``timestep, temperature, friction, pressure,
        compressibility, taup``) and after ``velocities``.  ``model_or_step``: an eval-mode model (a ``GraphedStep`` with energy,
        forces and stress is built around it, which needs ``r_max`` and all three directions periodic) or a ready
        ``force_step``."""
        device = torch.device(device)
        pos, vel, masses, cell = atoms_tensors(atoms, device, "positions", "velocities", "masses", "cell")
        step = model_or_step
        if isinstance(model_or_step, torch.nn.Module):
            if not all(bool(b) for b in np.asarray(atoms.get_pbc(), dtype=bool).reshape(3)):
                raise ValueError("NPT around a GraphedStep needs all three directions periodic")
            K = AtomicDataDict
            step = _graphed_step_for(atoms, model_or_step, device, r_max, chemical_symbols,
                                     outputs=(K.TOTAL_ENERGY_KEY, K.FORCE_KEY, K.STRESS_KEY))
        return cls(step, masses, *args, positions=pos, cell=cell, velocities=vel, **kwargs)

    def write_back(self, atoms) -> None:
        """Cell, positions and completed velocities into ``atoms`` (one copy each; the positions are already the scaled ones)."""
        atoms.set_cell(self._cell[0].detach().cpu().numpy(), scale_atoms=False)
        super().write_back(atoms)
