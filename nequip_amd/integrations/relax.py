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

CPU tensors (and ``backend="aten"``) take an ATen form of the same equations.  ``CellFIRE`` (below) relaxes the cell together
with the atoms: the same FIRE over ASE's ``UnitCellFilter`` coordinates, three launches of ``csrc/relax_cell.hip``.  Not
provided: other optimizers (the quasi-Newton ones need a Hessian estimate and a line search), an ``ase.optimize.Optimizer``
subclass, the exponential cell filters.
"""

from __future__ import annotations

import math
from typing import Callable, Dict, Optional

import numpy as np
import torch

from ..data import AtomicDataDict
from ._driver import (atoms_tensors, check_cells, checked_forces, checked_stress, padded, padded_layout, select_backend,
                      state_arrays, torchsim_force_step)
from .md import _cell_following_step, _DeviceMD, _graphed_step_for

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
        self._setup(force_step, positions, system_idx, fixed, dict(dt=dt, maxstep=maxstep, dtmax=dtmax, nmin=nmin, finc=finc,
                                                                   fdec=fdec, astart=astart, fa=fa), backend, _WORDS)
        S = self.num_systems
        self._write_state(torch.full((S,), self._params["dt"], dtype=torch.float64),
                          torch.full((S,), self._params["astart"], dtype=torch.float64),
                          torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64))
        self._evaluate()

    def _setup(self, force_step, positions, system_idx, fixed, params, backend, words) -> None:
        """The checks of the arguments, the systems, the buffers and, on the kernel path, the chunk table, the partial sums and
        the record of ``words`` 8-byte words per system."""
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
        self._params = self._check_params(params)
        self._hip = select_backend(backend, device)

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
            self._rec = torch.zeros(S, words, dtype=torch.float64, device=device)
            self._rec_i = self._rec.view(torch.int64)
            self._rec_h = self._rec.view(torch.int32)  # [S, 32]: nmin at 2 * 11, converged at 2 * 11 + 1
        else:
            self._pad_mask, self._pad_idx = padded_layout(counts, device)  # (a system may have no atoms)

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

    def _record(self, dt, a, npos, nsteps) -> torch.Tensor:
        """The record of every system on the host, as wide as the device's: words 0 .. 15 (``nqa_fire_system``) filled with the
        state given (``[S]`` each) and the parameters, the verdict cleared, zeros behind them."""
        p = self._params
        words = torch.zeros(self.num_systems, self._rec.shape[1], dtype=torch.float64)
        words[:, _DT], words[:, _A] = dt.cpu().double(), a.cpu().double()
        words.view(torch.int64)[:, _NPOS], words.view(torch.int64)[:, _NSTEPS] = npos.cpu().long(), nsteps.cpu().long()
        for word, key in ((_DTMAX, "dtmax"), (_MAXSTEP, "maxstep"), (_FINC, "finc"), (_FDEC, "fdec"), (_ASTART, "astart"),
                          (_FA, "fa")):
            words[:, word] = p[key]
        words[:, _TARGET] = self._fmax_target
        words.view(torch.int32)[:, 2 * _NMIN_CONVERGED] = p["nmin"]
        return words

    def _write_state(self, dt, a, npos, nsteps) -> None:
        """The whole record of every system: the state given (``[S]`` each), the parameters, the verdict cleared."""
        S = self.num_systems
        if self._hip:
            self._rec.copy_(self._record(dt, a, npos, nsteps))
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
        return padded(per_atom, self._pad_mask, self._pad_idx)

    def _decide(self, P, FF, VV, M):
        """The decision of every system from its four ``[S]`` sums: ``fmax`` and the verdict; for a system that has not
        converged the FIRE branch, with ``dt``, ``a``, ``npos`` and ``nsteps`` updated.  Returns ``(active, cv, cf, dt, scale)``,
        the coefficients of this step's move (``active``: not converged)."""
        p = self._params
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
        return active, cv, cf, dt_new, scale

    def _aten_step(self) -> None:
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
        active, cv, cf, dt_new, scale = self._decide(P, FF, VV, M)
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
        pos, vel = state_arrays(state, self.num_atoms)
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
        pos = atoms_tensors(atoms, device, "positions")
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
        force_step = torchsim_force_step(calc, cell, pbc, atomic_numbers, system_idx, with_stress=False)
        return cls(force_step, positions, system_idx=system_idx, **kwargs)


# ---- variable cell -------------------------------------------------------------------------------------------------------------
# the 8-byte words of nqa_cellfire_system behind the sixteen of nqa_fire_system; word 18 is two 32-bit halves: hydrostatic,
# constant_volume; the five matrices are 3 x 3 row-major
_CELL_FACTOR, _PRESSURE, _HYDROSTATIC_CONSTVOL, _MASK, _C0, _D_OLD, _D_NEW, _VD = 16, 17, 18, 19, 28, 37, 46, 55
_CELL_WORDS = 64


def _mul_rows(a: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """``a [..., 3]`` times ``m [..., 3, 3]`` (row vector times matrix), the three products added left to right."""
    return a[..., 0:1] * m[..., 0, :] + a[..., 1:2] * m[..., 1, :] + a[..., 2:3] * m[..., 2, :]


def _mul_rows_t(a: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """``a [..., 3]`` times the transpose of ``m [..., 3, 3]``, the three products added left to right."""
    return a[..., 0:1] * m[..., :, 0] + a[..., 1:2] * m[..., :, 1] + a[..., 2:3] * m[..., :, 2]


def _cofactors(m: torch.Tensor) -> torch.Tensor:
    """``[S, 3, 3]``: the cofactor of every element of ``m`` (``m^-T = cofactors / det``)."""
    c = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            c[i][j] = m[:, i1, j1] * m[:, i2, j2] - m[:, i1, j2] * m[:, i2, j1]
    return torch.stack([torch.stack(row, dim=-1) for row in c], dim=-2)


def _det(m: torch.Tensor, cof: Optional[torch.Tensor] = None) -> torch.Tensor:
    cof = _cofactors(m) if cof is None else cof
    return m[:, 0, 0] * cof[:, 0, 0] + m[:, 0, 1] * cof[:, 0, 1] + m[:, 0, 2] * cof[:, 0, 2]


class CellFIRE(FIRE):
    """FIRE over the atoms and the cell together, state on the device of ``positions``: ASE's ``UnitCellFilter`` under
    ``ase.optimize.FIRE``, for one system or a batch of independent systems concatenated along the atom axis.

    Per system: ``n`` atoms, the reference cell ``C0`` (rows are the lattice vectors, taken at construction), the current cell
    ``C``, the deformation gradient ``D = (C0^-1 C)^T`` (``C = C0 D^T``, ``D = I`` at the start), ``cell_factor`` (default ``n``,
    as in ASE).  Generalised coordinates, ``n + 3`` rows of 3: ``q_i = x_i D^-T`` for the atoms (carried as state, never
    re-solved) and ``Q = cell_factor D`` for the cell.  Generalised forces, with ``F`` the force and ``sigma`` the stress that
    ``force_step`` returns (``sigma = (1/V) dE/d(strain)``, ASE's sign; ``V = |det C|``)::

        atoms   g_i = F_i D                          (rows of ``fixed`` atoms count as zero; a fixed atom keeps its q_i, so its
                                                      x_i = q_i D^T follows the cell, as a filter over FixAtoms does)
        cell    W = -V (sigma + scalar_pressure I);  G = W D^-T;  then, in this order:
                hydrostatic_strain: G = (tr G / 3) I;  mask: G = G * mask;  constant_volume: tr G / 3 off the diagonal
                finally G = G / cell_factor

    FIRE is the fixed-cell definition of this module word for word, over all ``n + 3`` rows::

        reduce   with the D at which F was evaluated:  P = sum g.v,  FF = sum g.g,  VV = sum v.v,  M = max |g_i|^2
        decide   G is formed; its 9 components are added to P, FF, VV (against the cell velocity vD), its three row norms to M
                 fmax = sqrt(M);  converged = M < fmax_target^2;  if converged nothing changes; else the FIRE branch gives
                 cv, cf, dt, a, npos, scale, nsteps += 1, and the cell moves:
                   vD = cv vD + cf G;  vD = vD + dt G;  Q = cell_factor D + scale (dt vD);  D_new = Q / cell_factor;  C = C0 D_new^T
        move     g = F D_old;  v = cv v + cf g;  v = v + dt g;  q = q + scale (dt v);  x = q D_new^T

    Three HIP launches (``csrc/relax_cell.hip``: ``nqa_cellfire_reduce`` + ``nqa_cellfire_decide`` + ``nqa_cellfire_move``), then
    one force evaluation at ``(x, C)``.  ``C`` is written by the deciding launch into ``cell``, the ``[S, 3, 3]`` float64 buffer
    that ``force_step`` is handed at every call, so nothing of a step passes through the host.

    ``fmax`` is taken over the generalised rows, as an ASE optimizer sees them through the filter: the largest of ``|g_i|`` and of
    the three row norms of ``G``.  It is NOT the atoms' own ``|F_i|``; ``stress`` holds the last stress for a pressure criterion.

    ``force_step``: ``(positions [N, 3], cell [S, 3, 3]) -> {"forces", "total_energy", "stress" [S, 3, 3]}`` (float32 or float64
    forces and stress), or a ``GraphedStep`` built with ``outputs=(total_energy, forces, stress)`` for one system in a fully
    periodic cell (its cell is set by ``set_cell_from_device``).  ``cell``: ``[3, 3]`` or ``[S, 3, 3]``; ``cell_factor``: a float or
    ``[S]``; ``mask``: ``[3, 3]`` of 0/1.  The other arguments are those of ``FIRE``.

    Not provided: ``FrechetCellFilter`` / ``ExpCellFilter`` (they need a matrix exponential and its derivative), other
    optimizers, an ``ase.optimize`` shell, reading an ``Atoms`` object's constraints, cells with non-periodic directions on the
    ``GraphedStep`` route."""

    def __init__(self, force_step, positions: torch.Tensor, cell: torch.Tensor, system_idx: Optional[torch.Tensor] = None,
                 fixed: Optional[torch.Tensor] = None, cell_factor=None, scalar_pressure: float = 0.0,
                 hydrostatic_strain: bool = False, constant_volume: bool = False, mask=None, dt: float = 0.1,
                 maxstep: float = 0.2, dtmax: float = 1.0, nmin: int = 5, finc: float = 1.1, fdec: float = 0.5,
                 astart: float = 0.1, fa: float = 0.99, backend: str = "auto"):
        force_step = _cell_following_step(force_step)
        self._setup(force_step, positions, system_idx, fixed, dict(dt=dt, maxstep=maxstep, dtmax=dtmax, nmin=nmin, finc=finc,
                                                                   fdec=fdec, astart=astart, fa=fa), backend, _CELL_WORDS)
        S, device = self.num_systems, self.device
        if not isinstance(cell, torch.Tensor) or tuple(cell.shape) not in ((3, 3), (S, 3, 3)):
            raise ValueError(f"cell must be a tensor of shape [3, 3] or [{S}, 3, 3], got "
                             f"{tuple(cell.shape) if isinstance(cell, torch.Tensor) else type(cell).__name__}")
        if cell.device != device:
            raise ValueError(f"mixed devices: positions on {device}, cell on {cell.device}")
        c0 = cell.detach().to(torch.float64).reshape(-1, 3, 3).expand(S, 3, 3).contiguous().clone()
        check_cells(c0, single=False)
        if cell_factor is None:
            factor = torch.from_numpy(self._counts.astype(np.float64))
        else:
            factor = torch.as_tensor(cell_factor, dtype=torch.float64).detach().cpu().reshape(-1)
            if factor.numel() not in (1, S):
                raise ValueError(f"cell_factor must be a number or hold one per system ([{S}]), got {factor.numel()} values")
            factor = factor.expand(S).clone()
        if not bool((torch.isfinite(factor) & (factor > 0.0)).all()):
            raise ValueError("cell_factor must be positive and finite")
        if not (isinstance(scalar_pressure, (int, float)) and math.isfinite(scalar_pressure)):
            raise ValueError(f"scalar_pressure must be finite, got {scalar_pressure!r}")
        if mask is None:
            mask_t = torch.ones(3, 3, dtype=torch.float64)
        else:
            mask_t = torch.as_tensor(mask).detach().cpu()
            if tuple(mask_t.shape) != (3, 3):
                raise ValueError(f"mask must have shape [3, 3], got {tuple(mask_t.shape)}")
            mask_t = mask_t.to(torch.float64)
            if not bool(((mask_t == 0.0) | (mask_t == 1.0)).all()):
                raise ValueError("mask must hold zeros and ones")
        self._cell_params = {"cell_factor": factor, "scalar_pressure": float(scalar_pressure),
                             "hydrostatic_strain": bool(hydrostatic_strain), "constant_volume": bool(constant_volume),
                             "mask": mask_t}
        self._c0 = c0
        self._cell = c0.clone()
        self._q = self._pos.clone()
        self._stress: Optional[torch.Tensor] = None
        eye = torch.eye(3, dtype=torch.float64).expand(S, 3, 3)
        self._write_state(torch.full((S,), self._params["dt"], dtype=torch.float64),
                          torch.full((S,), self._params["astart"], dtype=torch.float64),
                          torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64),
                          eye, eye, torch.zeros(S, 3, 3, dtype=torch.float64))
        self._evaluate()

    # ---- state -------------------------------------------------------------------------------------------------------------
    def _write_state(self, dt, a, npos, nsteps, d_old=None, d_new=None, vd=None) -> None:
        """The whole record of every system: the FIRE state, ``D`` and ``vD`` (``[S, 3, 3]``), the parameters, the verdict
        cleared."""
        S, c = self.num_systems, self._cell_params
        if self._hip:
            words = self._record(dt, a, npos, nsteps)
            words[:, _CELL_FACTOR] = c["cell_factor"]
            words[:, _PRESSURE] = c["scalar_pressure"]
            words.view(torch.int32)[:, 2 * _HYDROSTATIC_CONSTVOL] = int(c["hydrostatic_strain"])
            words.view(torch.int32)[:, 2 * _HYDROSTATIC_CONSTVOL + 1] = int(c["constant_volume"])
            words[:, _MASK:_MASK + 9] = c["mask"].reshape(1, 9)
            words[:, _C0:_C0 + 9] = self._c0.cpu().reshape(S, 9)
            words[:, _D_OLD:_D_OLD + 9] = d_old.cpu().double().reshape(S, 9)
            words[:, _D_NEW:_D_NEW + 9] = d_new.cpu().double().reshape(S, 9)
            words[:, _VD:_VD + 9] = vd.cpu().double().reshape(S, 9)
            self._rec.copy_(words)
        else:
            FIRE._write_state(self, dt, a, npos, nsteps)
            dev = self.device
            self._d_old_s = d_old.to(dev).double().reshape(S, 3, 3).clone()
            self._d_s = d_new.to(dev).double().reshape(S, 3, 3).clone()
            self._vd_s = vd.to(dev).double().reshape(S, 3, 3).clone()

    def _evaluate(self) -> None:
        out = self.force_step(self._pos, self._cell)
        self._stress = checked_stress(out, self.num_systems, self.device, f"[{self.num_systems}, 3, 3]",
                                      "([S, 3, 3]) next to the forces for a variable-cell relaxation")
        self._out, self._forces = out, checked_forces(out, self.num_atoms, self.device)

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch(self) -> None:
        lib, L = self._lib.load(), self._lib
        f, sig = self._forces, self._stress
        dtype = L.NQA_F64 if f.dtype == torch.float64 else L.NQA_F32
        sdtype = L.NQA_F64 if sig.dtype == torch.float64 else L.NQA_F32
        stream = L.stream_ptr(self.device)
        L.check(lib.nqa_cellfire_reduce(dtype, L.ptr(f), L.ptr(self._vel), L.ptr(self._fixed), L.ptr(self._chunks), self._n_chunks,
                                        L.ptr(self._rec), L.ptr(self._partials), stream), "nqa_cellfire_reduce")
        L.check(lib.nqa_cellfire_decide(L.ptr(self._partials), L.ptr(self._chunk_begin), sdtype, L.ptr(sig), L.ptr(self._rec),
                                        L.ptr(self._cell), self.num_systems, stream), "nqa_cellfire_decide")
        L.check(lib.nqa_cellfire_move(dtype, L.ptr(f), L.ptr(self._pos), L.ptr(self._q), L.ptr(self._vel), L.ptr(self._fixed),
                                      L.ptr(self._chunks), self._n_chunks, L.ptr(self._rec), stream), "nqa_cellfire_move")

    def _cell_force(self, D: torch.Tensor) -> torch.Tensor:
        """``G [S, 3, 3]`` from the last stress at the deformation gradients ``D``."""
        c, dev = self._cell_params, self.device
        cell = _mul_rows_t(self._c0, D[:, None, :, :])  # C = C0 D^T, row by row
        V = _det(cell).abs()
        cof = _cofactors(D)
        d_inv_t = cof / _det(D, cof)[:, None, None]
        W = self._stress.to(torch.float64) + c["scalar_pressure"] * torch.eye(3, dtype=torch.float64, device=dev)
        W = -V[:, None, None] * W
        G = _mul_rows(W, d_inv_t[:, None, :, :])
        eye = torch.eye(3, dtype=torch.float64, device=dev)
        if c["hydrostatic_strain"]:
            G = ((G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]) / 3.0)[:, None, None] * eye
        G = G * c["mask"].to(dev)
        if c["constant_volume"]:
            G = G - ((G[:, 0, 0] + G[:, 1, 1] + G[:, 2, 2]) / 3.0)[:, None, None] * eye
        return G / c["cell_factor"].to(dev)[:, None, None]

    def _aten_step(self) -> None:
        s = self._system_idx
        f = self._forces.to(torch.float64)
        v, D, vd = self._vel, self._d_s, self._vd_s
        if self._fixed is not None:
            f = torch.where(self._fixed.bool()[:, None], torch.zeros_like(f), f)
        g = _mul_rows(f, D[s])
        # reduce
        gv, gg, vv = g * v, g * g, v * v
        gg_atom = self._padded(gg[:, 0] + gg[:, 1] + gg[:, 2])
        P = torch.sum(self._padded(gv[:, 0] + gv[:, 1] + gv[:, 2]), dim=1)
        FF = torch.sum(gg_atom, dim=1)
        VV = torch.sum(self._padded(vv[:, 0] + vv[:, 1] + vv[:, 2]), dim=1)
        M = torch.amax(gg_atom, dim=1)
        # decide: the cell's rows join the sums
        G = self._cell_force(D)
        P = P + (G * vd).reshape(-1, 9).sum(1)
        FF = FF + (G * G).reshape(-1, 9).sum(1)
        VV = VV + (vd * vd).reshape(-1, 9).sum(1)
        M = torch.maximum(M, torch.amax((G * G).sum(2), dim=1))  # (both keep a NaN)
        active, cv, cf, dt_new, scale = self._decide(P, FF, VV, M)
        # the cell move
        m3 = lambda t: t[:, None, None]  # noqa: E731
        factor = m3(self._cell_params["cell_factor"].to(self.device))
        vd_new = m3(cv) * vd + m3(cf) * G
        vd_new = vd_new + m3(dt_new) * G
        Q = factor * D
        Q = Q + m3(scale) * (m3(dt_new) * vd_new)
        d_new = Q / factor
        act3 = m3(active)
        self._d_old_s = torch.where(act3, D, self._d_old_s)
        self._d_s = torch.where(act3, d_new, D)
        self._vd_s = torch.where(act3, vd_new, vd)
        self._cell.copy_(torch.where(act3, _mul_rows_t(self._c0, d_new[:, None, :, :]), self._cell))
        # move
        moves = active[s][:, None]
        free = moves if self._fixed is None else moves & ~self._fixed.bool()[:, None]
        v_new = cv[s][:, None] * v + cf[s][:, None] * g
        v_new = v_new + dt_new[s][:, None] * g
        q_new = torch.where(free, self._q + scale[s][:, None] * (dt_new[s][:, None] * v_new), self._q)
        self._vel.copy_(torch.where(free, v_new, v))
        self._q.copy_(q_new)
        self._pos.copy_(torch.where(moves, _mul_rows_t(q_new, d_new[s]), self._pos))

    # ---- interface ----------------------------------------------------------------------------------------------------------
    @property
    def cell(self) -> torch.Tensor:
        """``[S, 3, 3]`` float64, rows are the lattice vectors: the live buffer that ``force_step`` reads."""
        return self._cell

    @property
    def deform_grad(self) -> torch.Tensor:
        return self._rec[:, _D_NEW:_D_NEW + 9].view(-1, 3, 3) if self._hip else self._d_s

    @property
    def cell_velocities(self) -> torch.Tensor:
        return self._rec[:, _VD:_VD + 9].view(-1, 3, 3) if self._hip else self._vd_s

    @property
    def _d_old(self) -> torch.Tensor:
        return self._rec[:, _D_OLD:_D_OLD + 9].view(-1, 3, 3) if self._hip else self._d_old_s

    @property
    def stress(self) -> torch.Tensor:
        """``[S, 3, 3]``: the stress ``force_step`` returned last, at the current positions and cell."""
        return self._stress

    @property
    def volume(self) -> torch.Tensor:
        return _det(self._cell).abs()

    @property
    def reference_cell(self) -> torch.Tensor:
        return self._c0

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        state = FIRE.state_dict(self)
        state.update({"q": self._q.detach().clone(), "D": self.deform_grad.detach().clone(), "D_old": self._d_old.detach().clone(),
                      "vD": self.cell_velocities.detach().clone(), "C0": self._c0.detach().clone(),
                      "cell": self._cell.detach().clone(),
                      "cell_parameters": {k: (v.clone() if isinstance(v, torch.Tensor) else v)
                                          for k, v in self._cell_params.items()}})
        return state

    def load_state_dict(self, state: Dict[str, object]) -> None:
        pos, vel = state_arrays(state, self.num_atoms)
        if "vD" not in state or "npos" not in state or tuple(state["dt"].shape) != (self.num_systems,):
            raise ValueError(f"the state was not saved by a CellFIRE run of {self.num_systems} systems")
        self._params = self._check_params(dict(state["parameters"]))
        self._cell_params = {k: (v.clone() if isinstance(v, torch.Tensor) else v) for k, v in state["cell_parameters"].items()}
        self._fmax_target = float(state["fmax_target"])
        self._pos.copy_(pos)
        self._vel.copy_(vel)
        self._q.copy_(state["q"])
        self._c0.copy_(state["C0"])
        self._cell.copy_(state["cell"])
        self._write_state(state["dt"], state["a"], state["npos"], state["nsteps"], state["D_old"], state["D"], state["vD"])
        self._evaluate()

    # ---- Atoms and torch-sim ------------------------------------------------------------------------------------------------
    @classmethod
    def from_atoms(cls, atoms, model_or_step, device="cuda", r_max: Optional[float] = None, chemical_symbols=None, **kwargs):
        """The optimizer for an ``Atoms`` object (positions, cell, periodicity, species; its constraints are NOT read: pass
        ``fixed``).  ``model_or_step``: an eval-mode model (a ``GraphedStep`` with energy, forces and stress is built around
        it, which needs ``r_max`` and all three directions periodic) or a ready ``force_step``.  ``kwargs``: the constructor's."""
        device = torch.device(device)
        pos, cell = atoms_tensors(atoms, device, "positions", "cell")
        step = model_or_step
        if isinstance(model_or_step, torch.nn.Module):
            if not all(bool(b) for b in np.asarray(atoms.get_pbc(), dtype=bool).reshape(3)):
                raise ValueError("a variable-cell relaxation around a GraphedStep needs all three directions periodic")
            K = AtomicDataDict
            step = _graphed_step_for(atoms, model_or_step, device, r_max, chemical_symbols,
                                     outputs=(K.TOTAL_ENERGY_KEY, K.FORCE_KEY, K.STRESS_KEY))
        return cls(step, pos, cell, **kwargs)

    def write_back(self, atoms) -> None:
        """Cell and positions into ``atoms`` (one copy each; the atoms are not rescaled with the cell: the positions follow)."""
        atoms.set_cell(self._cell[0].detach().cpu().numpy(), scale_atoms=False)
        atoms.set_positions(self._pos.detach().cpu().numpy())

    @classmethod
    def from_torchsim(cls, calc, positions, cell, pbc, atomic_numbers, system_idx, **kwargs):
        """The optimizer of a batch around a ``NequIPTorchSimCalc``: ``force_step`` hands ``calc`` a state with ``positions``,
        ``row_vector_cell`` (the live cell buffer), ``pbc``, ``atomic_numbers`` and ``system_idx``, and returns its forces,
        per-system energies and stresses.  ``calc.compute_stress`` is switched on."""
        force_step = torchsim_force_step(calc, cell, pbc, atomic_numbers, system_idx, with_stress=True)
        return cls(force_step, positions, cell, system_idx=system_idx, **kwargs)
