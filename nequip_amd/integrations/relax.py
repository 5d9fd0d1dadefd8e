"""Structural relaxation with the state on the device: FIRE (Bitzek et al. 2006, with ASE's defaults and step cap) for one
system or a batch of independent systems concatenated along the atom axis, as ``system_idx`` does for ``NequIPTorchSimCalc``.

Through a calculator every step of a relaxation uploads the positions, downloads energy and forces and runs the optimizer in
numpy.  Here positions, velocities and one record per system (time step, mixing factor, counters, verdict) are device tensors,
advanced between two force evaluations by three HIP launches (``csrc/relax.hip``: ``nqa_fire_reduce`` + ``nqa_fire_decide`` +
``nqa_fire_move``), so a step moves nothing to the host beyond what the force evaluation itself reads.

One step of a system, with ``F`` the force at the current positions (components of ``fixed`` atoms count as zero; the dynamics is
massless, the cell is fixed)::

    reduce   P = sum F.v,  FF = sum F.F,  VV = sum v.v,  M = max over atoms of |F|^2
    decide   fmax = sqrt(M);  converged = M < fmax_target^2;  if converged, nothing of the system changes; else
               first step (v = 0):  cv = 0, cf = 0
               P > 0:               cv = 1 - a, cf = a sqrt(VV) / sqrt(FF); if npos > nmin: dt = min(dt finc, dtmax), a = a fa; npos += 1
               otherwise:           cv = 0, cf = 0, a = astart, dt = dt fdec, npos = 0
             c = cf + dt;  VVn = cv^2 VV + 2 cv c P + c^2 FF;  normdr = dt sqrt(VVn);  scale = min(1, maxstep / normdr);  nsteps += 1
    move     v = cv v + cf F;  v = v + dt F;  x = x + scale (dt v)

The one deliberate difference from the textbook loop: the length of the step is formed in ``decide`` from the three sums of the
old velocities (``VVn`` is the squared norm of the new ones, every term non-negative) where the textbook takes the norm of the new
displacements directly.  The two differ by rounding only, and a third reduction is spared.

The verdict is taken at the start of a step, from the forces that step is handed: ``fmax`` and ``converged`` describe the
positions BEFORE the last step's move, and a converged system is left alone by every later step.

CPU tensors (and ``backend="aten"``) take an ATen form of the same equations.  Not provided: variable-cell relaxation, other
optimizers (the quasi-Newton ones need a Hessian estimate and a line search), an ``ase.optimize.Optimizer`` subclass.
"""

from __future__ import annotations

import math
from types import SimpleNamespace
from typing import Callable, Dict, Optional

import numpy as np
import torch

from ..data import AtomicDataDict
from .md import _DeviceMD, _graphed_step_for

# the 8-byte words of nqa_fire_system (include/nequip_amd.h); word 11 is two 32-bit halves: nmin, converged
_DT, _A, _NPOS, _NSTEPS, _DTMAX, _MAXSTEP, _FINC, _FDEC, _ASTART, _FA, _TARGET, _NMIN_CONVERGED, _CV, _CF, _SCALE, _FMAX = range(16)
_WORDS = 16
_CHUNK_DTYPE = np.dtype([("atom0", "<i8"), ("count", "<i4"), ("system", "<i4")])  # nqa_fire_chunk


def fire_chunk_table(counts: np.ndarray, chunk_atoms: int):
    """The chunks of systems with ``counts`` atoms each, concatenated: ``(chunks, chunk_begin)``, a structured array of
    ``nqa_fire_chunk`` (no chunk straddles two systems) and ``[S + 1]`` int64 with the chunks of system ``s`` at
    ``chunk_begin[s] .. chunk_begin[s + 1]``."""
    counts = np.asarray(counts, dtype=np.int64)
    per_system = (counts + chunk_atoms - 1) // chunk_atoms
    chunk_begin = np.concatenate([[0], np.cumsum(per_system)]).astype(np.int64)
    atom_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    system = np.repeat(np.arange(len(counts), dtype=np.int64), per_system)
    local = (np.arange(int(chunk_begin[-1]), dtype=np.int64) - chunk_begin[system]) * chunk_atoms
    chunks = np.zeros(len(system), dtype=_CHUNK_DTYPE)
    chunks["atom0"] = atom_begin[system] + local
    chunks["count"] = np.minimum(chunk_atoms, counts[system] - local)
    chunks["system"] = system
    return chunks, chunk_begin


class FIRE:
    """FIRE relaxation of a fixed set of atoms in a fixed cell, state on the device of ``positions``.

    ``force_step``: a ``GraphedStep`` or any callable ``pos [N, 3] -> {"forces": [N, 3], "total_energy": ...}`` (float32 or
    float64 forces; all tensors on the device of ``positions``), as for the MD drivers; there are no masses.  ``system_idx``
    ``[N]``: the system of every atom, non-decreasing (default: one system); every system has its own time step, mixing factor,
    counters and verdict.  ``fixed`` ``[N]`` bool: atoms that never move and do not enter ``fmax``.  ``dt, maxstep, dtmax, nmin,
    finc, fdec, astart, fa``: ASE's parameters with ASE's defaults.  ``backend``: ``"hip"`` (the kernels; the default on the
    GPU), ``"aten"`` (the default on the CPU).

    ``positions``, ``forces``, ``velocities`` are the live tensors; ``fmax``, ``converged``, ``nsteps``, ``dt``, ``a`` are ``[S]``
    device tensors as of the last step's decision; ``potential_energy`` is what ``force_step`` returned last, flattened.
    ``step`` reads nothing from the device; ``run`` reads the ``[S]`` records once every ``check_every`` steps."""

    _evaluate = _DeviceMD._evaluate

    def __init__(self, force_step: Callable[[torch.Tensor], Dict[str, torch.Tensor]], positions: torch.Tensor,
                 system_idx: Optional[torch.Tensor] = None, fixed: Optional[torch.Tensor] = None, dt: float = 0.1,
                 maxstep: float = 0.2, dtmax: float = 1.0, nmin: int = 5, finc: float = 1.1, fdec: float = 0.5,
                 astart: float = 0.1, fa: float = 0.99, backend: str = "auto"):
        if not callable(force_step):
            raise TypeError("force_step must be callable: positions [N, 3] -> {'forces', 'total_energy'}")
        if not isinstance(positions, torch.Tensor):
            raise TypeError("positions must be a tensor")
        if positions.dim() != 2 or positions.shape[1] != 3:
            raise ValueError(f"positions must have shape [N, 3], got {tuple(positions.shape)}")
        n = int(positions.shape[0])
        if n == 0:
            raise ValueError("no atoms: positions has N == 0")
        device = positions.device
        for name, t in (("system_idx", system_idx), ("fixed", fixed)):
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (n,):
                raise ValueError(f"{name} must be a tensor of shape [{n}] to match positions, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__}")
            if t.device != device:
                raise ValueError(f"mixed devices: positions on {device}, {name} on {t.device}")
        step_device = getattr(force_step, "device", None)
        if isinstance(step_device, torch.device) and step_device != device:
            raise ValueError(f"mixed devices: positions on {device}, force_step on {step_device}")
        self._params = self._check_params(dict(dt=dt, maxstep=maxstep, dtmax=dtmax, nmin=nmin, finc=finc, fdec=fdec,
                                               astart=astart, fa=fa))
        if backend not in ("auto", "hip", "aten"):
            raise ValueError(f"backend must be 'auto', 'hip' or 'aten', got {backend!r}")
        if backend == "hip" and device.type != "cuda":
            raise ValueError("backend='hip' needs device tensors: the kernels run on the GPU")
        self._hip = backend == "hip" or (backend == "auto" and device.type == "cuda")

        # the systems: one host read, here (the chunk table is built once)
        if system_idx is None:
            counts = np.array([n], dtype=np.int64)
            self._system_idx = torch.zeros(n, dtype=torch.long, device=device)
        else:
            if system_idx.dtype not in (torch.int32, torch.int64):
                raise ValueError(f"system_idx must hold integers, got {system_idx.dtype}")
            idx = system_idx.detach().cpu().numpy().astype(np.int64)
            if idx[0] < 0 or np.any(np.diff(idx) < 0):
                raise ValueError("system_idx must start at 0 or above and never decrease: the atoms of a system are contiguous")
            counts = np.bincount(idx).astype(np.int64)
            self._system_idx = system_idx.detach().to(torch.long).contiguous().clone()
        self.num_systems = int(len(counts))
        self._counts = counts

        self.force_step = force_step
        self.device = device
        self.num_atoms = n
        self._pos = positions.detach().to(torch.float64).contiguous().clone()
        self._vel = torch.zeros_like(self._pos)
        self._fixed = None if fixed is None else (fixed.detach() != 0).to(torch.uint8).contiguous().clone()
        self._out: Dict[str, torch.Tensor] = {}
        self._forces: Optional[torch.Tensor] = None
        self._fmax_target = 0.05
        S = self.num_systems
        if self._hip:
            from .. import _lib

            self._lib = _lib
            chunk_atoms = int(_lib.load().nqa_fire_chunk_atoms())
            chunks, chunk_begin = fire_chunk_table(counts, chunk_atoms)
            self._n_chunks = int(len(chunks))
            self._chunks = torch.from_numpy(chunks.view(np.int64).reshape(-1, 2).copy()).to(device)
            self._chunk_begin = torch.from_numpy(chunk_begin).to(device)
            self._partials = torch.zeros(self._n_chunks, 4, dtype=torch.float64, device=device)
            self._rec = torch.zeros(S, _WORDS, dtype=torch.float64, device=device)
            self._rec_i = self._rec.view(torch.int64)
            self._rec_h = self._rec.view(torch.int32)  # [S, 32]: nmin at 2 * 11, converged at 2 * 11 + 1
        else:
            # atom (s, k) of the padded [S, max count] layout that the per-system sums are taken over
            width = max(int(counts.max()), 1)
            begin = np.concatenate([[0], np.cumsum(counts)])[:-1]
            k = np.arange(width)[None, :]
            self._pad_mask = torch.from_numpy(k < counts[:, None]).to(device)
            self._pad_idx = torch.from_numpy(np.where(k < counts[:, None], begin[:, None] + k, 0)).to(device)
        self._write_state(torch.full((S,), self._params["dt"], dtype=torch.float64),
                          torch.full((S,), self._params["astart"], dtype=torch.float64),
                          torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64))
        self._evaluate()

    # ---- state -------------------------------------------------------------------------------------------------------------
    @staticmethod
    def _check_params(p: Dict[str, float]) -> Dict[str, float]:
        finite = lambda v: isinstance(v, (int, float)) and math.isfinite(v)  # noqa: E731
        if not (finite(p["dt"]) and p["dt"] > 0.0):
            raise ValueError(f"dt must be positive, got {p['dt']!r}")
        if not (finite(p["maxstep"]) and p["maxstep"] > 0.0):
            raise ValueError(f"maxstep must be positive, got {p['maxstep']!r}")
        if not (finite(p["dtmax"]) and p["dtmax"] > 0.0):
            raise ValueError(f"dtmax must be positive, got {p['dtmax']!r}")
        if not (finite(p["fdec"]) and 0.0 < p["fdec"] < 1.0):
            raise ValueError(f"fdec must lie in (0, 1), got {p['fdec']!r}")
        if not (finite(p["finc"]) and p["finc"] >= 1.0):
            raise ValueError(f"finc must be at least 1, got {p['finc']!r}")
        if isinstance(p["nmin"], bool) or not isinstance(p["nmin"], (int, np.integer)) or not (0 <= p["nmin"] < 2 ** 31):
            raise ValueError(f"nmin must be a non-negative integer, got {p['nmin']!r}")
        if not (finite(p["astart"]) and 0.0 <= p["astart"] <= 1.0):
            raise ValueError(f"astart must lie in [0, 1], got {p['astart']!r}")
        if not (finite(p["fa"]) and 0.0 < p["fa"] <= 1.0):
            raise ValueError(f"fa must lie in (0, 1], got {p['fa']!r}")
        out = {k: float(v) for k, v in p.items()}
        out["nmin"] = int(p["nmin"])
        return out

    def _write_state(self, dt, a, npos, nsteps) -> None:
        """The whole record of every system: the state given (``[S]`` each), the parameters, the verdict cleared."""
        S, p = self.num_systems, self._params
        if self._hip:
            words = torch.zeros(S, _WORDS, dtype=torch.float64)
            words[:, _DT], words[:, _A] = dt.cpu().double(), a.cpu().double()
            words.view(torch.int64)[:, _NPOS], words.view(torch.int64)[:, _NSTEPS] = npos.cpu().long(), nsteps.cpu().long()
            for word, key in ((_DTMAX, "dtmax"), (_MAXSTEP, "maxstep"), (_FINC, "finc"), (_FDEC, "fdec"), (_ASTART, "astart"),
                              (_FA, "fa")):
                words[:, word] = p[key]
            words[:, _TARGET] = self._fmax_target
            words.view(torch.int32)[:, 2 * _NMIN_CONVERGED] = p["nmin"]
            self._rec.copy_(words)
        else:
            dev = self.device
            self._dt_s, self._a_s = dt.to(dev).double().clone(), a.to(dev).double().clone()
            self._npos_s, self._nsteps_s = npos.to(dev).long().clone(), nsteps.to(dev).long().clone()
            self._fmax_s = torch.zeros(S, dtype=torch.float64, device=dev)
            self._converged_s = torch.zeros(S, dtype=torch.bool, device=dev)

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch(self) -> None:
        lib, L = self._lib.load(), self._lib
        f = self._forces
        dtype = L.NQA_F64 if f.dtype == torch.float64 else L.NQA_F32
        stream = L.stream_ptr(self.device)
        L.check(lib.nqa_fire_reduce(dtype, L.ptr(f), L.ptr(self._vel), L.ptr(self._fixed), L.ptr(self._chunks), self._n_chunks,
                                    L.ptr(self._partials), stream), "nqa_fire_reduce")
        L.check(lib.nqa_fire_decide(L.ptr(self._partials), L.ptr(self._chunk_begin), L.ptr(self._rec), self.num_systems, stream),
                "nqa_fire_decide")
        L.check(lib.nqa_fire_move(dtype, L.ptr(f), L.ptr(self._pos), L.ptr(self._vel), L.ptr(self._fixed), L.ptr(self._chunks),
                                  self._n_chunks, L.ptr(self._rec), stream), "nqa_fire_move")

    def _padded(self, per_atom: torch.Tensor) -> torch.Tensor:
        """``[S, max count]``: the values of every system's atoms in a row of their own, zeros behind them."""
        zero = torch.zeros((), dtype=per_atom.dtype, device=per_atom.device)
        return torch.where(self._pad_mask, per_atom[self._pad_idx], zero)

    def _aten_step(self) -> None:
        p = self._params
        f = self._forces.to(torch.float64)
        v = self._vel
        if self._fixed is not None:
            f = torch.where(self._fixed.bool()[:, None], torch.zeros_like(f), f)
        # reduce
        fv, ff, vv = f * v, f * f, v * v
        ff_atom = self._padded(ff[:, 0] + ff[:, 1] + ff[:, 2])
        P = torch.sum(self._padded(fv[:, 0] + fv[:, 1] + fv[:, 2]), dim=1)
        FF = torch.sum(ff_atom, dim=1)
        VV = torch.sum(self._padded(vv[:, 0] + vv[:, 1] + vv[:, 2]), dim=1)
        M = torch.amax(ff_atom, dim=1)
        # decide
        dt, a, npos = self._dt_s, self._a_s, self._npos_s
        converged = M < self._fmax_target * self._fmax_target
        first = self._nsteps_s == 0
        up = (P > 0.0) & ~first
        down = ~up & ~first
        grow = up & (npos > p["nmin"])
        zero, one = torch.zeros_like(dt), torch.ones_like(dt)
        cv = torch.where(up, 1.0 - a, zero)
        cf = torch.where(up, a * torch.sqrt(VV) / torch.sqrt(FF), zero)
        grown = dt * p["finc"]
        dt_new = torch.where(grow, torch.where(grown < p["dtmax"], grown, torch.full_like(dt, p["dtmax"])),
                             torch.where(down, dt * p["fdec"], dt))
        a_new = torch.where(grow, a * p["fa"], torch.where(down, torch.full_like(a, p["astart"]), a))
        npos_new = torch.where(up, npos + 1, torch.where(down, torch.zeros_like(npos), npos))
        c = cf + dt_new
        vvn = cv * cv * VV + 2.0 * cv * c * P + c * c * FF
        normdr = dt_new * torch.sqrt(vvn)
        scale = torch.where(normdr > p["maxstep"], p["maxstep"] / normdr, one)
        active = ~converged
        self._fmax_s, self._converged_s = torch.sqrt(M), converged
        self._dt_s = torch.where(active, dt_new, dt)
        self._a_s = torch.where(active, a_new, a)
        self._npos_s = torch.where(active, npos_new, npos)
        self._nsteps_s = self._nsteps_s + active.to(torch.int64)
        # move
        s = self._system_idx
        moves = active[s]
        if self._fixed is not None:
            moves = moves & ~self._fixed.bool()
        moves = moves[:, None]
        v_new = cv[s][:, None] * v + cf[s][:, None] * f
        v_new = v_new + dt_new[s][:, None] * f
        x_new = self._pos + scale[s][:, None] * (dt_new[s][:, None] * v_new)
        self._vel.copy_(torch.where(moves, v_new, v))
        self._pos.copy_(torch.where(moves, x_new, self._pos))

    # ---- interface ----------------------------------------------------------------------------------------------------------
    def step(self) -> None:
        """One FIRE step of every system that has not converged: three launches, then one force evaluation."""
        if self._hip:
            self._launch()
        else:
            self._aten_step()
        self._evaluate()

    def _set_target(self, fmax: float) -> None:
        if not (isinstance(fmax, (int, float)) and math.isfinite(fmax) and fmax > 0.0):
            raise ValueError(f"fmax must be positive and finite, got {fmax!r}")
        self._fmax_target = float(fmax)
        if self._hip:
            self._rec[:, _TARGET].fill_(self._fmax_target)

    def run(self, fmax: float = 0.05, steps: int = 1000, check_every: int = 1) -> bool:
        """Steps until every system has ``max |F_i| < fmax`` or ``steps`` steps were taken; returns whether all converged.
        The target is written in place; the ``[S]`` records are read once every ``check_every`` steps (and after the last),
        which is the only host read of the optimizer.  The verdict is taken at the start of a step, so the run ends with the step
        that found every system converged, and that step moved nothing.  Raises ``FloatingPointError`` if an ``fmax`` it reads
        is not finite."""
        steps, check_every = int(steps), int(check_every)
        if check_every < 1:
            raise ValueError(f"check_every must be at least 1, got {check_every}")
        self._set_target(fmax)
        for k in range(steps):
            self.step()
            if (k + 1) % check_every == 0 or k + 1 == steps:
                if self._read_verdict():
                    return True
        return False

    def _read_verdict(self) -> bool:
        if self._hip:
            host = self._rec.cpu()
            fmax, converged = host[:, _FMAX], host.view(torch.int32)[:, 2 * _NMIN_CONVERGED + 1] != 0
        else:
            both = torch.stack([self._fmax_s, self._converged_s.to(torch.float64)]).cpu()
            fmax, converged = both[0], both[1] != 0
        if not bool(torch.isfinite(fmax).all()):
            bad = int((~torch.isfinite(fmax)).nonzero()[0])
            raise FloatingPointError(f"fmax of system {bad} is not finite ({float(fmax[bad])}): the forces hold a NaN or an infinity")
        return bool(converged.all())

    @property
    def positions(self) -> torch.Tensor:
        return self._pos

    @property
    def velocities(self) -> torch.Tensor:
        return self._vel

    @property
    def forces(self) -> torch.Tensor:
        return self._forces

    @property
    def system_idx(self) -> torch.Tensor:
        return self._system_idx

    @property
    def potential_energy(self) -> torch.Tensor:
        """What ``force_step`` returned last as ``total_energy``, flattened (one value per system where it gives that)."""
        return self._out[AtomicDataDict.TOTAL_ENERGY_KEY].detach().reshape(-1)

    @property
    def fmax(self) -> torch.Tensor:
        return self._rec[:, _FMAX] if self._hip else self._fmax_s

    @property
    def converged(self) -> torch.Tensor:
        return self._rec_h[:, 2 * _NMIN_CONVERGED + 1] != 0 if self._hip else self._converged_s

    @property
    def nsteps(self) -> torch.Tensor:
        return self._rec_i[:, _NSTEPS] if self._hip else self._nsteps_s

    @property
    def dt(self) -> torch.Tensor:
        return self._rec[:, _DT] if self._hip else self._dt_s

    @property
    def a(self) -> torch.Tensor:
        return self._rec[:, _A] if self._hip else self._a_s

    @property
    def _npos(self) -> torch.Tensor:
        return self._rec_i[:, _NPOS] if self._hip else self._npos_s

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        return {"positions": self._pos.detach().clone(), "velocities": self._vel.detach().clone(), "dt": self.dt.detach().clone(),
                "a": self.a.detach().clone(), "npos": self._npos.detach().clone(), "nsteps": self.nsteps.detach().clone(),
                "fmax_target": self._fmax_target, "parameters": dict(self._params)}

    def load_state_dict(self, state: Dict[str, object]) -> None:
        pos, vel = state["positions"], state["velocities"]
        if tuple(pos.shape) != (self.num_atoms, 3) or tuple(vel.shape) != (self.num_atoms, 3):
            raise ValueError(f"the state holds {tuple(pos.shape)} positions and {tuple(vel.shape)} velocities, this run has "
                             f"{self.num_atoms} atoms")
        if "npos" not in state or tuple(state["dt"].shape) != (self.num_systems,):
            raise ValueError(f"the state was not saved by a FIRE run of {self.num_systems} systems")
        self._params = self._check_params(dict(state["parameters"]))
        self._fmax_target = float(state["fmax_target"])
        self._pos.copy_(pos)
        self._vel.copy_(vel)
        self._write_state(state["dt"], state["a"], state["npos"], state["nsteps"])
        self._evaluate()

    # ---- Atoms and torch-sim ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model_or_step, device="cuda", r_max: Optional[float] = None, chemical_symbols=None, **kwargs):
        """The optimizer for an ``Atoms`` object (positions, cell, periodicity, species; its constraints are NOT read: pass
        ``fixed``).  ``model_or_step``: an eval-mode model (a ``GraphedStep`` is built around it, which needs a periodic cell and
        ``r_max``) or a ready ``force_step``.  ``chemical_symbols``: as for ``NequIPCalculator``.  ``kwargs``: the constructor's."""
        device = torch.device(device)
        pos = torch.as_tensor(np.asarray(atoms.get_positions(), dtype=np.float64)).to(device)
        step = model_or_step
        if isinstance(model_or_step, torch.nn.Module):
            step = _graphed_step_for(atoms, model_or_step, device, r_max, chemical_symbols)
        return cls(step, pos, **kwargs)

    def write_back(self, atoms) -> None:
        """Positions into ``atoms`` (one copy)."""
        atoms.set_positions(self._pos.detach().cpu().numpy())

    @classmethod
    def from_torchsim(cls, calc, positions, cell, pbc, atomic_numbers, system_idx, **kwargs):
        """The optimizer of a batch around a ``NequIPTorchSimCalc``: ``force_step`` hands ``calc`` a state with ``positions``,
        ``row_vector_cell`` (``cell``, ``[S, 3, 3]``), ``pbc``, ``atomic_numbers`` and ``system_idx``, and returns its forces and
        per-system energies.  A calculator that was given the atomic numbers itself is not given them again.  The optimizer
        reads forces and energies only: set ``calc.compute_stress = False`` first where the stress is not needed."""
        numbers = None if getattr(calc, "atomic_numbers_in_init", False) else atomic_numbers
        state = SimpleNamespace(positions=None, row_vector_cell=cell, pbc=pbc, atomic_numbers=numbers, system_idx=system_idx)

        def force_step(pos):
            state.positions = pos
            res = calc(state)
            return {AtomicDataDict.FORCE_KEY: res["forces"], AtomicDataDict.TOTAL_ENERGY_KEY: res["energy"]}

        return cls(force_step, positions, system_idx=system_idx, **kwargs)
