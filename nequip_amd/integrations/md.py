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
"""

from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import numpy as np
import torch

from ..data import AtomicDataDict

# CODATA 2014, the values behind ase.units
_e, _amu, _k = 1.6021766208e-19, 1.660539040e-27, 1.38064852e-23
units = SimpleNamespace(kB=_k / _e, fs=1e-5 * math.sqrt(_e / _amu))

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


def _graphed_step_for(atoms, model, device, r_max, chemical_symbols):
    """A ``GraphedStep`` for the species, cell and periodicity of ``atoms`` (the species mapping of ``NequIPCalculator``)."""
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
    return GraphedStep(model, torch.as_tensor(types).to(device), torch.as_tensor(cell).to(device), pbc, float(r_max))


class NoseHoover:
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
        if thermostat and not (nvt_q > 0.0 and temperature >= 0.0):
            raise ValueError("the thermostat needs nvt_q > 0 and temperature >= 0")
        if backend not in ("auto", "hip", "aten"):
            raise ValueError(f"backend must be 'auto', 'hip' or 'aten', got {backend!r}")
        if backend == "hip" and device.type != "cuda":
            raise ValueError("backend='hip' needs device tensors: the kernels run on the GPU")
        self._hip = backend == "hip" or (backend == "auto" and device.type == "cuda")
        self.force_step = force_step
        self.device = device
        self.num_atoms = n
        self.thermostat = bool(thermostat)
        self._m = masses.detach().to(torch.float64).contiguous().clone()
        self._pos = positions.detach().to(torch.float64).contiguous().clone()
        vel = torch.zeros_like(self._pos) if velocities is None else velocities.detach().to(torch.float64)
        if remove_drift:
            vel = _remove_drift(self._pos, vel, self._m)
        self._vel = vel.contiguous().clone()  # v(t) while `fresh`, v_half between two steps
        self._vel_out = torch.empty_like(self._vel)
        self._temperature = float(temperature)
        self._dt, self._q = float(timestep), float(nvt_q)
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
            self._mode = _MD_THERMOSTAT if self.thermostat else 0
        else:
            self._xi = torch.zeros((), dtype=torch.float64, device=device)
            self._ekin = torch.zeros((), dtype=torch.float64, device=device)
            self._fresh = True
            self._nsteps = 0
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

    def _evaluate(self) -> None:
        out = self.force_step(self._pos)
        f = out[AtomicDataDict.FORCE_KEY].detach()
        if tuple(f.shape) != (self.num_atoms, 3) or f.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"force_step must return float32 or float64 forces [{self.num_atoms}, 3], got {f.dtype} "
                             f"{tuple(f.shape)}")
        if f.device != self.device:
            raise ValueError(f"mixed devices: positions on {self.device}, forces on {f.device}")
        self._out, self._forces = out, f.contiguous()

    def set_temperature(self, temperature: float) -> None:
        """The bath's target from the next step on; written in place, nothing is read back."""
        self._temperature = float(temperature)
        if self._hip:
            self._rec[_G:_G + 1].fill_(self._g())

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
    def nvt_bath(self) -> float:
        return float(self._rec[_XI]) if self._hip else float(self._xi)

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

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        return {"positions": self._pos.detach().clone(), "velocities": self.velocities.detach().clone(), "nvt_bath": self.nvt_bath,
                "nsteps": self.nsteps, "timestep": self._dt, "temperature": self._temperature, "nvt_q": self._q,
                "thermostat": self.thermostat}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        pos, vel = state["positions"], state["velocities"]
        if tuple(pos.shape) != (self.num_atoms, 3) or tuple(vel.shape) != (self.num_atoms, 3):
            raise ValueError(f"the state holds {tuple(pos.shape)} positions and {tuple(vel.shape)} velocities, this run has "
                             f"{self.num_atoms} atoms")
        if bool(state["thermostat"]) != self.thermostat:
            raise ValueError("the state was saved with the thermostat " + ("on" if state["thermostat"] else "off"))
        self._pos.copy_(pos)
        self._vel.copy_(vel)
        self._dt, self._temperature, self._q = float(state["timestep"]), float(state["temperature"]), float(state["nvt_q"])
        self._write_state(xi=float(state["nvt_bath"]), nsteps=int(state["nsteps"]))
        self._evaluate()

    # ---- Atoms --------------------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model_or_step, *args, device="cuda", r_max: Optional[float] = None, chemical_symbols=None,
                   **kwargs):
        """The driver for an ``Atoms`` object (positions, velocities, masses, cell, periodicity, species); ``args`` and
        ``kwargs`` are the constructor's between ``masses`` and ``positions`` (``timestep, temperature, nvt_q``) and after
        ``velocities``.  ``model_or_step``: an eval-mode model (``torch.nn.Module`` with ``type_names``; a ``GraphedStep`` is
        built around it, which needs a periodic cell and ``r_max``) or a ready ``force_step``.  ``chemical_symbols``: as for
        ``NequIPCalculator``."""
        device = torch.device(device)
        pos = torch.as_tensor(np.asarray(atoms.get_positions(), dtype=np.float64)).to(device)
        vel = atoms.get_velocities()
        vel = None if vel is None else torch.as_tensor(np.asarray(vel, dtype=np.float64)).to(device)
        masses = torch.as_tensor(np.asarray(atoms.get_masses(), dtype=np.float64)).to(device)
        step = model_or_step
        if isinstance(model_or_step, torch.nn.Module):
            step = _graphed_step_for(atoms, model_or_step, device, r_max, chemical_symbols)
        return cls(step, masses, *args, positions=pos, velocities=vel, **kwargs)

    def write_back(self, atoms) -> None:
        """Positions and completed velocities into ``atoms`` (one copy each)."""
        atoms.set_positions(self._pos.detach().cpu().numpy())
        atoms.set_velocities(self.velocities.detach().cpu().numpy())


class VelocityVerlet(NoseHoover):
    """Velocity Verlet (NVE): ``NoseHoover`` with the thermostat off."""

    def __init__(self, force_step, masses: torch.Tensor, timestep: float, positions: torch.Tensor,
                 velocities: Optional[torch.Tensor] = None, remove_drift: bool = True, backend: str = "auto"):
        super().__init__(force_step, masses, timestep, 0.0, 1.0, positions, velocities, thermostat=False,
                         remove_drift=remove_drift, backend=backend)
