"""Langevin NVT and NPT dynamics of a batch of independent systems with the state on the device: ``BatchedLangevin`` and
``BatchedLangevinNPT`` are ``Langevin`` and ``LangevinNPT`` (``integrations/md.py``) for ``S`` systems concatenated along the atom
axis, as ``system_idx`` does for ``NequIPTorchSimCalc`` and for the batched ``FIRE``.  Every system has its own temperature,
friction, time step, seed and, under NPT, pressure, barostat and cell; the whole batch advances by the two (NVT) or three (NPT)
HIP launches that one system takes (``csrc/md_batched.hip``), then one batched force evaluation.

The contract: system ``s`` of a batch, with seed ``seeds[s]``, has bit for bit the positions, stored and completed velocities,
kinetic energy and (NPT) cell, ``mu``, pressure and volume that ``Langevin`` / ``LangevinNPT`` produce for that system alone with
``seed=seeds[s]`` and the same forces (and stresses), at every step.  The kernels of both are the same device functions
(``csrc/md_device.h``); the noise of a component is a function of ``(seeds[s], nsteps[s], j)`` with ``j`` the component's index
inside its own system; and the kinetic-energy sum of a system has the partition and the order of the single-system launches
(``md_chunk_table``: no chunk of 256 components straddles two systems).

CPU tensors (and ``backend="aten"``) take an ATen form of the same equations: element-wise on the concatenated arrays with
per-atom parameters, the per-system sums over the padded ``[S, max count]`` layout that ``FIRE`` uses.

Not provided: batched Nose-Hoover, anisotropic cells, systems entering or leaving a running batch (torch-sim's autobatching), an
active mask, a batched ``GraphedStep``.
"""

from __future__ import annotations

import math
from typing import Dict, List, Optional

import numpy as np
import torch

from ..data import AtomicDataDict
from ._driver import (_det3, _philox_numpy, check_cells, checked_forces, checked_stress, padded, padded_layout, select_backend,
                      state_arrays, torchsim_force_step)
from .md import (_C1, _C2, _DT, _EKIN_OBSERVED, _FRESH, _KT, _MD_FINISH_ONLY, _NPT_A, _NPT_FAILED, _NPT_INDEX, _NPT_MU, _NPT_P,
                 _NPT_P0, _NSTEPS, _SEED, _aten_barostat, _check_u64, _DeviceMD, _normals_numpy, _remove_drift, _sqrt, units)

MD_THREADS = 256  # NQA_MD_THREADS (include/nequip_amd.h)
_CHUNK_DTYPE = np.dtype([("component0", "<i8"), ("local0", "<i8"), ("count", "<i4"), ("system", "<i4")])  # nqa_md_chunk


def md_chunk_table(counts, threads: int = MD_THREADS):
    """The chunks of systems with ``counts`` atoms each, concatenated: ``(chunks, chunk_begin)``, a structured array of
    ``nqa_md_chunk`` and ``[S + 1]`` int64 with the chunks of system ``s`` at ``chunk_begin[s] .. chunk_begin[s + 1]``.  Chunk
    ``k`` of system ``s`` covers its flat components ``[threads k, min(threads (k + 1), 3 n_s))``: a chunk may straddle two atoms,
    never two systems, and a system has the ``ceil(3 n_s / threads)`` chunks that it has alone."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    n3 = 3 * counts
    per_system = (n3 + threads - 1) // threads
    chunk_begin = np.concatenate([[0], np.cumsum(per_system)]).astype(np.int64)
    component_begin = np.concatenate([[0], np.cumsum(n3)]).astype(np.int64)
    system = np.repeat(np.arange(len(counts), dtype=np.int64), per_system)
    local = (np.arange(int(chunk_begin[-1]), dtype=np.int64) - chunk_begin[system]) * threads
    chunks = np.zeros(len(system), dtype=_CHUNK_DTYPE)
    chunks["component0"] = component_begin[system] + local
    chunks["local0"] = local
    chunks["count"] = np.minimum(threads, n3[system] - local)
    chunks["system"] = system
    return chunks, chunk_begin


def batch_seeds(seed, num_systems: int) -> List[int]:
    """The seeds of the systems: an int gives ``(seed + s) mod 2^64`` for system ``s``; a sequence of ``num_systems`` ints, each
    in [0, 2^64), is taken as given."""
    if isinstance(seed, (int, np.integer)) and not isinstance(seed, bool):
        first = _check_u64("seed", seed)
        return [(first + s) % 2 ** 64 for s in range(num_systems)]
    if isinstance(seed, torch.Tensor):
        seed = seed.detach().cpu().tolist()
    try:
        seeds = list(seed)
    except TypeError:
        raise ValueError(f"seed must be an integer or a sequence of {num_systems} integers, got {seed!r}") from None
    if len(seeds) != num_systems:
        raise ValueError(f"seed must be an integer or hold one per system ([{num_systems}]), got {len(seeds)} values")
    return [_check_u64(f"seed of system {s}", v) for s, v in enumerate(seeds)]


def _per_system(name: str, value, num_systems: int) -> np.ndarray:
    """``value`` (a number, or a sequence / array / tensor of one value per system) as float64 ``[S]``."""
    if isinstance(value, torch.Tensor):
        value = value.detach().cpu().numpy()
    try:
        arr = np.asarray(value, dtype=np.float64).reshape(-1)
    except (TypeError, ValueError):
        raise ValueError(f"{name} must be a number or hold one value per system ([{num_systems}]), got {value!r}") from None
    if arr.size == 1:
        arr = np.full(num_systems, arr[0], dtype=np.float64)
    if arr.size != num_systems:
        raise ValueError(f"{name} must be a number or hold one value per system ([{num_systems}]), got {arr.size} values")
    return arr.copy()


class BatchedLangevin:
    """Langevin NVT dynamics (BAOAB, the scheme of ``Langevin``) of ``S`` independent systems, state on the device of
    ``positions``.

    ``force_step``: any callable ``pos [N, 3] -> {"forces": [N, 3], "total_energy": [S]}`` over the concatenated atoms (float32
    or float64 forces; all tensors on the device of ``positions``).  ``masses`` ``[N]`` in amu.  ``system_idx`` ``[N]``: the
    system of every atom, starting at 0, never decreasing and without gaps (one host read, here).  ``timestep`` (ASE's time
    unit), ``temperature`` (K) and ``friction`` (1/time): each a number for all systems or a sequence / tensor of ``S`` values.
    ``seed``: an int gives ``seeds[s] = (seed + s) mod 2^64``; a sequence of ``S`` ints in [0, 2^64) is taken as given.  System
    ``s`` takes, bit for bit, the steps of ``Langevin(..., seed=seeds[s])`` for that system alone.  ``remove_drift``: once,
    here, per system, centre-of-mass momentum and angular momentum are set to zero.  ``backend``: ``"hip"`` (the kernels; the
    default on the GPU), ``"aten"`` (the default on the CPU).

    ``positions`` and ``forces`` are the live tensors; ``velocities`` are the completed ``v(t)`` in a buffer of their own that the
    next read overwrites.  ``kinetic_energy``, ``temperature``, ``potential_energy`` and ``nsteps`` are ``[S]`` device tensors.
    ``set_temperature``, ``set_friction`` and ``set_timestep`` take a number or ``S`` values and write in place.  ``step`` and
    ``run`` read nothing on the host."""

    _evaluate = _DeviceMD._evaluate

    def __init__(self, force_step, masses: torch.Tensor, timestep, temperature, friction, positions: torch.Tensor,
                 system_idx: torch.Tensor, velocities: Optional[torch.Tensor] = None, seed=0, remove_drift: bool = False,
                 backend: str = "auto"):
        self._setup(force_step, masses, timestep, temperature, friction, positions, system_idx, velocities, seed, remove_drift,
                    backend)
        self._write_state(np.zeros(self.num_systems, dtype=np.int64))
        self._evaluate()

    # ---- construction ------------------------------------------------------------------------------------------------------
    def _setup(self, force_step, masses, timestep, temperature, friction, positions, system_idx, velocities, seed, remove_drift,
               backend) -> None:
        _DeviceMD._check_system(self, force_step, masses, positions, velocities, 1.0)
        n, device = int(positions.shape[0]), positions.device
        if not isinstance(system_idx, torch.Tensor) or tuple(system_idx.shape) != (n,):
            raise ValueError(f"system_idx must be a tensor of shape [{n}] to match positions, got "
                             f"{tuple(system_idx.shape) if isinstance(system_idx, torch.Tensor) else type(system_idx).__name__}")
        if system_idx.device != device:
            raise ValueError(f"mixed devices: positions on {device}, system_idx on {system_idx.device}")
        if system_idx.dtype not in (torch.int32, torch.int64):
            raise ValueError(f"system_idx must hold integers, got {system_idx.dtype}")
        idx = system_idx.detach().cpu().numpy().astype(np.int64)  # the one host read: the chunk table is built once
        steps_up = np.diff(idx)
        if idx[0] != 0 or np.any(steps_up < 0) or np.any(steps_up > 1):
            raise ValueError("system_idx must start at 0, never decrease and leave no system without atoms: the atoms of a "
                             "system are contiguous")
        counts = np.bincount(idx).astype(np.int64)
        S = int(len(counts))
        self.num_systems, self.num_atoms, self._counts = S, n, counts
        self._atom_begin = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        self._dt_h = self._checked("timestep", timestep)
        self._temperature_h = self._checked("temperature", temperature)
        self._friction_h = self._checked("friction", friction)
        self.seeds = batch_seeds(seed, S)

        self._hip = select_backend(backend, device)
        self.force_step, self.device = force_step, device
        self._system_idx = system_idx.detach().to(torch.long).contiguous().clone()
        self._m = masses.detach().to(torch.float64).contiguous().clone()
        self._pos = positions.detach().to(torch.float64).contiguous().clone()
        vel = torch.zeros_like(self._pos) if velocities is None else velocities.detach().to(torch.float64).clone()
        if remove_drift:
            b = self._atom_begin
            for s in range(S):
                vel[b[s]:b[s + 1]] = _remove_drift(self._pos[b[s]:b[s + 1]], vel[b[s]:b[s + 1]], self._m[b[s]:b[s + 1]])
        self._vel = vel.contiguous().clone()  # v(t) while `fresh`, the O-step velocities v2 between two steps
        self._vel_out = torch.empty_like(self._vel)
        self._out: Dict[str, torch.Tensor] = {}
        self._forces: Optional[torch.Tensor] = None
        # 3 n_s kB per system, in the host's float64: the divisor of `temperature`
        self._dof_kb = torch.tensor([3 * int(c) * units.kB for c in counts], dtype=torch.float64, device=device)
        if self._hip:
            from .. import _lib

            self._lib = _lib
            chunks, chunk_begin = md_chunk_table(counts, MD_THREADS)
            self._n_chunks = int(len(chunks))
            self._chunks = torch.from_numpy(chunks.view(np.int64).reshape(-1, 3).copy()).to(device)
            self._chunk_begin = torch.from_numpy(chunk_begin).to(device)
            self._partials = torch.zeros(self._n_chunks, 2, dtype=torch.float64, device=device)
            self._partials_observed = torch.zeros_like(self._partials)
            self._rec = torch.zeros(S, 8, dtype=torch.float64, device=device)  # nqa_md_state[S]
            self._rec_i = self._rec.view(torch.int64)
            self._par = torch.zeros(S, 4, dtype=torch.float64, device=device)  # nqa_md_langevin_params[S]
        else:
            self._pad_mask, self._pad_idx = padded_layout(counts, device)
            # the system and the local index of every flat component: what the noise is drawn for
            self._component_system = np.repeat(np.arange(S), 3 * counts)
            self._component_local = (np.arange(3 * n) - 3 * self._atom_begin[self._component_system]).astype(np.uint64)
            self._fresh = True
            self._nsteps_h = np.zeros(S, dtype=np.int64)

    _CHECKS = {
        "timestep": (lambda a: a > 0.0, "timestep must be positive"),
        "temperature": (lambda a: a >= 0.0, "temperature must be non-negative and finite"),
        "friction": (lambda a: a >= 0.0, "friction must be non-negative and finite"),
        "pressure": (lambda a: a == a, "pressure must be finite"),
        "compressibility": (lambda a: a >= 0.0, "compressibility must be non-negative and finite"),
        "taup": (lambda a: a > 0.0, "taup must be positive and finite"),
    }

    def _checked(self, name: str, value) -> np.ndarray:
        arr = _per_system(name, value, self.num_systems)
        accept, message = self._CHECKS[name]
        with np.errstate(invalid="ignore"):
            good = np.isfinite(arr) & accept(arr)
        if not good.all():
            bad = int(np.flatnonzero(~good)[0])
            raise ValueError(f"{message}, got {float(arr[bad])!r} for system {bad}")
        return arr

    # ---- state -------------------------------------------------------------------------------------------------------------
    def _spread(self, per_system: np.ndarray) -> torch.Tensor:
        """``[N, 1]`` float64 on the device: the value of every atom's system."""
        return torch.from_numpy(np.ascontiguousarray(per_system, dtype=np.float64)).to(self.device)[self._system_idx][:, None]

    def _write_params(self) -> None:
        """``c1``, ``c2`` (the host's ``math.exp`` and ``math.sqrt``: the bits ``Langevin`` writes) and ``kB T`` of every system."""
        c1 = np.array([math.exp(-f * dt) for f, dt in zip(self._friction_h.tolist(), self._dt_h.tolist())], dtype=np.float64)
        c2 = np.array([math.sqrt(1.0 - c * c) for c in c1.tolist()], dtype=np.float64)
        kt = np.array([units.kB * t for t in self._temperature_h.tolist()], dtype=np.float64)
        self._c1_h, self._c2_h, self._kt_h = c1, c2, kt
        if self._hip:
            words = torch.zeros(self.num_systems, 4, dtype=torch.float64)
            words[:, _C1], words[:, _C2], words[:, _KT] = torch.from_numpy(c1), torch.from_numpy(c2), torch.from_numpy(kt)
            words.view(torch.int64)[:, _SEED] = torch.tensor([s - 2 ** 64 if s >= 2 ** 63 else s for s in self.seeds],
                                                             dtype=torch.int64)  # (the same 64 bits)
            self._par.copy_(words)  # (no launch writes this record)
        else:
            self._hdt_a = self._spread(0.5 * self._dt_h)
            self._c1_a, self._c2_a, self._kt_a = self._spread(c1), self._spread(c2), self._spread(kt)

    def _write_state(self, nsteps: np.ndarray) -> None:
        """Both records of every system, with ``velocities`` taken as completed."""
        nsteps = np.asarray(nsteps, dtype=np.int64).reshape(self.num_systems)
        if self._hip:
            words = torch.zeros(self.num_systems, 8, dtype=torch.float64)
            words[:, _DT] = torch.from_numpy(self._dt_h)
            words.view(torch.int64)[:, _NSTEPS] = torch.from_numpy(nsteps)
            words.view(torch.int64)[:, _FRESH] = 1
            self._rec.copy_(words)
        else:
            self._fresh, self._nsteps_h = True, nsteps.copy()
        self._write_params()

    def set_temperature(self, temperature) -> None:
        """The targets (a number or ``S`` values) from the next step on; ``kB T`` is written in place, nothing is read back."""
        self._temperature_h = self._checked("temperature", temperature)
        self._write_params()

    def set_friction(self, friction) -> None:
        """The frictions (a number or ``S`` values, 1/time) from the next step on; ``c1`` and ``c2`` are written in place."""
        self._friction_h = self._checked("friction", friction)
        self._write_params()

    def set_timestep(self, timestep) -> None:
        """The time steps (a number or ``S`` values) from the next step on, ``c1`` and ``c2`` with them.  The step that is under
        way is completed with the step it began with (the arithmetic the next step would have carried out: a system whose time
        step does not change keeps its trajectory bit for bit)."""
        dt = self._checked("timestep", timestep)
        self._vel.copy_(self.velocities)
        self._dt_h = dt
        if self._hip:
            self._rec_i[:, _FRESH].fill_(1)
            self._rec[:, _DT].copy_(torch.from_numpy(dt))
        else:
            self._fresh = True
        self._write_params()

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch_step(self, finish_only: bool):
        lib, L = self._lib.load(), self._lib
        f = self._forces
        mode = _MD_FINISH_ONLY if finish_only else 0
        partials = self._partials_observed if finish_only else self._partials
        stream = L.stream_ptr(self.device)
        L.check(lib.nqa_md_batched_langevin_step(L.NQA_F64 if f.dtype == torch.float64 else L.NQA_F32, L.ptr(f), L.ptr(self._m),
                                                 L.ptr(self._pos), L.ptr(self._vel), L.ptr(self._vel_out), L.ptr(self._chunks),
                                                 self._n_chunks, L.ptr(self._rec), L.ptr(self._par), L.ptr(partials), mode,
                                                 stream), "nqa_md_batched_langevin_step")
        return partials, mode, stream

    def _launch(self, finish_only: bool, bath: bool = True) -> None:
        partials, mode, stream = self._launch_step(finish_only)
        if bath:
            lib, L = self._lib.load(), self._lib
            L.check(lib.nqa_md_batched_bath(L.ptr(partials), L.ptr(self._chunk_begin), L.ptr(self._rec), self.num_systems, mode,
                                            stream), "nqa_md_batched_bath")

    def _per_system_sum(self, per_atom: torch.Tensor) -> torch.Tensor:
        """``[S]``: the sum of ``per_atom [N]`` over the atoms of every system (the padded layout of ``FIRE``)."""
        return torch.sum(padded(per_atom, self._pad_mask, self._pad_idx), dim=1)

    def _kinetic(self, v: torch.Tensor) -> torch.Tensor:
        mvv = self._m[:, None] * v * v
        return 0.5 * self._per_system_sum(mvv[:, 0] + mvv[:, 1] + mvv[:, 2])

    def _aten_finished(self) -> torch.Tensor:
        if self._fresh:
            return self._vel
        fm = self._forces.to(torch.float64) / self._m[:, None]
        return self._vel + self._hdt_a * fm

    def _aten_noise(self, index: np.ndarray, system: np.ndarray) -> np.ndarray:
        """The normals of the components ``index`` (local to their systems ``system``) at the step counts of those systems."""
        seeds = np.array(self.seeds, dtype=np.uint64)[system]
        steps = self._nsteps_h.astype(np.uint64)[system]
        return _normals_numpy(_philox_numpy(seeds, steps, index))

    def _aten_step(self) -> None:
        mc, hdt = self._m[:, None], self._hdt_a
        v = self._aten_finished()
        fm = self._forces.to(torch.float64) / mc
        z = torch.from_numpy(self._aten_noise(self._component_local, self._component_system)).to(self.device).reshape(-1, 3)
        v1 = v + hdt * fm
        x = self._pos + hdt * v1
        v2 = self._c1_a * v1 + (self._c2_a * _sqrt(self._kt_a.expand_as(mc) / mc)) * z
        self._pos.copy_(x + hdt * v2)
        self._ekin = self._kinetic(v)
        self._vel.copy_(v2)
        self._fresh = False
        self._nsteps_h = self._nsteps_h + 1

    # ---- interface ----------------------------------------------------------------------------------------------------------
    def step(self) -> None:
        """One MD step of every system: the launches, then one force evaluation at the new positions."""
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
    def system_idx(self) -> torch.Tensor:
        return self._system_idx

    @property
    def velocities(self) -> torch.Tensor:
        """The completed velocities ``v(t)`` at the current positions; leaves the trajectory alone."""
        if self._hip:
            self._launch(finish_only=True, bath=False)
        else:
            self._vel_out.copy_(self._aten_finished())
        return self._vel_out

    @property
    def kinetic_energy(self) -> torch.Tensor:
        """``[S]``: ``1/2 sum m v(t)^2`` of every system's completed velocities at the current positions (eV)."""
        if self._hip:
            self._launch(finish_only=True)
            return self._rec[:, _EKIN_OBSERVED].clone()
        return self._kinetic(self._aten_finished())

    @property
    def temperature(self) -> torch.Tensor:
        """``[S]``: the kinetic temperature ``2 K / (3 n_s kB)`` of every system (K)."""
        return 2.0 * self.kinetic_energy / self._dof_kb

    @property
    def potential_energy(self) -> torch.Tensor:
        """What ``force_step`` returned last as ``total_energy``, flattened (``[S]`` where it gives one value per system)."""
        return self._out[AtomicDataDict.TOTAL_ENERGY_KEY].detach().reshape(-1)

    @property
    def nsteps(self) -> torch.Tensor:
        if self._hip:
            return self._rec_i[:, _NSTEPS]
        return torch.from_numpy(self._nsteps_h.copy()).to(self.device)

    @property
    def target_temperature(self) -> np.ndarray:
        return self._temperature_h.copy()

    @property
    def friction(self) -> np.ndarray:
        return self._friction_h.copy()

    @property
    def timestep(self) -> np.ndarray:
        return self._dt_h.copy()

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        return {"positions": self._pos.detach().clone(), "velocities": self.velocities.detach().clone(),
                "nsteps": BatchedLangevin.nsteps.fget(self).detach().cpu().clone(), "timestep": self._dt_h.copy(),
                "temperature": self._temperature_h.copy(), "friction": self._friction_h.copy(), "seeds": list(self.seeds)}

    def _load_common(self, state: Dict[str, object]) -> np.ndarray:
        pos, vel = state_arrays(state, self.num_atoms)
        if "friction" not in state or "seeds" not in state or len(state["seeds"]) != self.num_systems:
            raise ValueError(f"the state was not saved by a batched Langevin run of {self.num_systems} systems")
        nsteps = np.asarray(torch.as_tensor(state["nsteps"]).cpu().numpy(), dtype=np.int64).reshape(-1)
        if nsteps.shape != (self.num_systems,) or np.any(nsteps < 0):
            raise ValueError(f"the state must hold one non-negative step count per system ([{self.num_systems}])")
        dt = self._checked("timestep", state["timestep"])
        temperature = self._checked("temperature", state["temperature"])
        friction = self._checked("friction", state["friction"])
        seeds = batch_seeds(list(state["seeds"]), self.num_systems)
        self._pos.copy_(pos)
        self._vel.copy_(vel)
        self._dt_h, self._temperature_h, self._friction_h, self.seeds = dt, temperature, friction, seeds
        return nsteps

    def load_state_dict(self, state: Dict[str, object]) -> None:
        if "compressibility" in state:
            raise ValueError("the state was saved by a BatchedLangevinNPT run (it holds a cell and a barostat)")
        self._write_state(self._load_common(state))
        self._evaluate()

    # ---- torch-sim ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_torchsim(cls, calc, positions, cell, pbc, atomic_numbers, system_idx, masses, timestep, temperature, friction,
                      **kwargs):
        """The driver of a batch around a ``NequIPTorchSimCalc``: ``force_step`` hands ``calc`` a state with ``positions``,
        ``row_vector_cell`` (``cell``, ``[S, 3, 3]``), ``pbc``, ``atomic_numbers`` and ``system_idx``, and returns its forces and
        per-system energies.  A calculator that was given the atomic numbers itself is not given them again.  The driver reads
        forces and energies only: set ``calc.compute_stress = False`` first where the stress is not needed.  ``kwargs``: the
        constructor's (``velocities``, ``seed``, ``remove_drift``, ``backend``)."""
        force_step = torchsim_force_step(calc, cell, pbc, atomic_numbers, system_idx, with_stress=False)
        return cls(force_step, masses, timestep, temperature, friction, positions, system_idx, **kwargs)


class BatchedLangevinNPT(BatchedLangevin):
    """Isotropic NPT dynamics (the scheme of ``LangevinNPT``: BAOAB, then stochastic cell rescaling) of ``S`` independent systems,
    state and cells on the device of ``positions``.  Three HIP launches per step for the whole batch
    (``nqa_md_batched_langevin_step`` + ``nqa_md_batched_npt_bath`` + ``nqa_md_batched_npt_scale``); the second writes every
    system's cell into ``cell``, the ``[S, 3, 3]`` float64 buffer that ``force_step`` is handed at every call.

    ``force_step``: ``(positions [N, 3], cell [S, 3, 3]) -> {"forces", "total_energy" [S], "stress" [S, 3, 3]}`` (float32 or
    float64 forces and stress, ``(1/V) dE/d(strain)``: ASE's sign, what ``CellFIRE`` takes).  ``pressure`` (eV/A^3),
    ``compressibility`` (A^3/eV) and ``taup`` (time): each a number or ``S`` values.  The other arguments and the interface are
    those of ``BatchedLangevin``; added are ``cell`` (live), ``volume``, ``pressure`` (the ``P`` that drove the last step),
    ``stress``, ``target_pressure``, ``failed`` (all per system), ``set_pressure`` and ``set_barostat``.  System ``s`` takes, bit
    for bit, the steps of ``LangevinNPT(..., seed=seeds[s])`` alone; ``compressibility = 0`` for a system gives it the
    ``BatchedLangevin`` trajectory bit for bit.  A scaling factor that is not finite or a cell without volume leaves ``mu = 1``
    for that system and sets its flag, the other systems go on; the next read of ``nsteps``, ``pressure`` or ``volume`` raises
    ``RuntimeError`` and names the systems."""

    def __init__(self, force_step, masses: torch.Tensor, timestep, temperature, friction, pressure, compressibility, taup,
                 positions: torch.Tensor, cell: torch.Tensor, system_idx: torch.Tensor,
                 velocities: Optional[torch.Tensor] = None, seed=0, remove_drift: bool = False, backend: str = "auto"):
        self._setup(force_step, masses, timestep, temperature, friction, positions, system_idx, velocities, seed, remove_drift,
                    backend)
        S, device = self.num_systems, self.device
        self._p0_h = self._checked("pressure", pressure)
        self._compressibility_h = self._checked("compressibility", compressibility)
        self._taup_h = self._checked("taup", taup)
        shapes = ((S, 3, 3), (3, 3)) if S == 1 else ((S, 3, 3),)
        if not isinstance(cell, torch.Tensor) or tuple(cell.shape) not in shapes:
            raise ValueError(f"cell must be a tensor of shape [{S}, 3, 3], got "
                             f"{tuple(cell.shape) if isinstance(cell, torch.Tensor) else type(cell).__name__}")
        if cell.device != device:
            raise ValueError(f"mixed devices: positions on {device}, cell on {cell.device}")
        self._cell = cell.detach().to(torch.float64).reshape(S, 3, 3).contiguous().clone()
        check_cells(self._cell, single=False)
        self._stress: Optional[torch.Tensor] = None
        if self._hip:
            self._npt = torch.zeros(S, 8, dtype=torch.float64, device=device)  # nqa_md_npt_state[S]
            self._npt_i = self._npt.view(torch.int64)
        self._write_state(np.zeros(S, dtype=np.int64))
        self._evaluate()

    # ---- state -------------------------------------------------------------------------------------------------------------
    def _write_params(self) -> None:
        """The thermostat's records and the two words of the barostat's that the host owns beside the noise index."""
        super()._write_params()
        self._a_h = np.array([c * dt / tau for c, dt, tau in zip(self._compressibility_h.tolist(), self._dt_h.tolist(),
                                                                 self._taup_h.tolist())], dtype=np.float64)
        if self._hip:
            self._npt[:, _NPT_A].copy_(torch.from_numpy(self._a_h))
            self._npt[:, _NPT_P0].copy_(torch.from_numpy(self._p0_h))
        else:
            on = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(self.device)  # noqa: E731
            self._a_t, self._p0_t, self._kt_t = on(self._a_h), on(self._p0_h), on(self._kt_h)

    def _write_state(self, nsteps: np.ndarray) -> None:
        """All three records of every system, with ``velocities`` taken as completed, ``mu = 1`` and the flags cleared."""
        S = self.num_systems
        if self._hip:
            words = torch.zeros(S, 8, dtype=torch.float64)
            words[:, _NPT_MU] = 1.0
            words.view(torch.int64)[:, _NPT_INDEX] = torch.from_numpy(3 * self._counts)
            self._npt.copy_(words)
        else:
            self._mu = torch.ones(S, dtype=torch.float64, device=self.device)
            self._pressure = torch.zeros(S, dtype=torch.float64, device=self.device)
            self._failed = torch.zeros(S, dtype=torch.bool, device=self.device)
        super()._write_state(nsteps)

    def set_pressure(self, pressure) -> None:
        """The target pressures (a number or ``S`` values, eV/A^3) from the next step on; written in place."""
        self._p0_h = self._checked("pressure", pressure)
        self._write_params()

    def set_barostat(self, compressibility, taup) -> None:
        """Compressibilities (A^3/eV) and relaxation times (each a number or ``S`` values) from the next step on; ``a`` is
        written in place."""
        compressibility, taup = self._checked("compressibility", compressibility), self._checked("taup", taup)
        self._compressibility_h, self._taup_h = compressibility, taup
        self._write_params()

    def _evaluate(self) -> None:
        out = self.force_step(self._pos, self._cell)
        S = self.num_systems
        self._stress = checked_stress(out, S, self.device, f"[{S}, 3, 3]", f"([{S}, 3, 3]) next to the forces for NPT")
        self._out, self._forces = out, checked_forces(out, self.num_atoms, self.device)

    # ---- the two forms of a step --------------------------------------------------------------------------------------------
    def _launch(self, finish_only: bool, bath: bool = True) -> None:
        if finish_only:
            return super()._launch(finish_only, bath)
        partials, _, stream = self._launch_step(False)
        lib, L = self._lib.load(), self._lib
        sig = self._stress
        L.check(lib.nqa_md_batched_npt_bath(L.ptr(partials), L.ptr(self._chunk_begin), L.ptr(self._rec), L.ptr(self._par),
                                            L.ptr(self._npt), L.NQA_F64 if sig.dtype == torch.float64 else L.NQA_F32, L.ptr(sig),
                                            L.ptr(self._cell), self.num_systems, stream), "nqa_md_batched_npt_bath")
        L.check(lib.nqa_md_batched_npt_scale(L.ptr(self._pos), L.ptr(self._vel), L.ptr(self._chunks), self._n_chunks,
                                             L.ptr(self._npt), stream), "nqa_md_batched_npt_scale")

    def _aten_step(self) -> None:
        systems = np.arange(self.num_systems)
        xi = torch.from_numpy(self._aten_noise((3 * self._counts).astype(np.uint64), systems)).to(self.device)
        sig = self._stress.to(torch.float64)
        super()._aten_step()
        mu, p, bad = _aten_barostat(self._ekin, self._cell, sig, xi, self._a_t, self._p0_t, self._kt_t)
        self._failed = self._failed | bad
        mu_atom = mu[self._system_idx][:, None]
        self._cell.copy_(mu[:, None, None] * self._cell)
        self._pos.copy_(mu_atom * self._pos)
        self._vel.copy_(self._vel / mu_atom)
        self._mu, self._pressure = mu, p

    # ---- interface ----------------------------------------------------------------------------------------------------------
    @property
    def failed(self) -> torch.Tensor:
        """``[S]`` bool: the systems whose barostat met a scaling factor that is not finite or a cell without volume."""
        return self._npt_i[:, _NPT_FAILED] != 0 if self._hip else self._failed

    def _check_failed(self) -> None:
        bad = self.failed.cpu().nonzero().reshape(-1).tolist()
        if bad:
            raise RuntimeError(f"the barostat of system(s) {bad} met a scaling factor that is not finite or a cell without "
                               "volume: their run is invalid from that step on (smaller compressibility / taup or time step)")

    @property
    def nsteps(self) -> torch.Tensor:
        self._check_failed()
        return BatchedLangevin.nsteps.fget(self)

    @property
    def cell(self) -> torch.Tensor:
        """``[S, 3, 3]`` float64, rows are the lattice vectors: the live buffer that ``force_step`` reads."""
        return self._cell

    @property
    def stress(self) -> torch.Tensor:
        """``[S, 3, 3]``: the stress ``force_step`` returned last, at the current positions and cells."""
        return self._stress

    @property
    def target_pressure(self) -> np.ndarray:
        return self._p0_h.copy()

    @property
    def compressibility(self) -> np.ndarray:
        return self._compressibility_h.copy()

    @property
    def taup(self) -> np.ndarray:
        return self._taup_h.copy()

    @property
    def pressure(self) -> torch.Tensor:
        """``[S]``: the ``P`` that drove the last step of every system (eV/A^3; 0 before the first)."""
        self._check_failed()
        return self._npt[:, _NPT_P].clone() if self._hip else self._pressure

    @property
    def scaling(self) -> torch.Tensor:
        """``[S]``: the ``mu`` of the last step of every system (1 before the first)."""
        return self._npt[:, _NPT_MU].clone() if self._hip else self._mu

    @property
    def volume(self) -> torch.Tensor:
        """``[S]``: ``|det C|`` of the current cells (A^3)."""
        self._check_failed()
        return _det3(self._cell).abs()

    # ---- checkpoints --------------------------------------------------------------------------------------------------------
    def state_dict(self) -> Dict[str, object]:
        state = BatchedLangevin.state_dict(self)
        state.update({"cell": self._cell.detach().clone(), "pressure": self._p0_h.copy(),
                      "compressibility": self._compressibility_h.copy(), "taup": self._taup_h.copy()})
        return state

    def load_state_dict(self, state: Dict[str, object]) -> None:
        """The cells are taken as they are: one without volume is met by the barostat (``failed``), not refused here."""
        if "compressibility" not in state or "cell" not in state:
            raise ValueError("the state was not saved by a BatchedLangevinNPT run (it holds no cell and no barostat)")
        cell = state["cell"]
        if tuple(cell.shape) != (self.num_systems, 3, 3):
            raise ValueError(f"the state holds cells of shape {tuple(cell.shape)}, this run has {self.num_systems} systems")
        p0 = self._checked("pressure", state["pressure"])
        compressibility, taup = self._checked("compressibility", state["compressibility"]), self._checked("taup", state["taup"])
        nsteps = self._load_common(state)
        self._cell.copy_(cell)
        self._p0_h, self._compressibility_h, self._taup_h = p0, compressibility, taup
        self._write_state(nsteps)
        self._evaluate()

    # ---- torch-sim ----------------------------------------------------------------------------------------------------------
    @classmethod
    def from_torchsim(cls, calc, positions, cell, pbc, atomic_numbers, system_idx, masses, timestep, temperature, friction,
                      pressure, compressibility, taup, **kwargs):
        """The driver of a batch around a ``NequIPTorchSimCalc``: ``force_step`` hands ``calc`` a state with ``positions``,
        ``row_vector_cell`` (the live cell buffer), ``pbc``, ``atomic_numbers`` and ``system_idx``, and returns its forces,
        per-system energies and stresses (ASE's sign, as ``CellFIRE.from_torchsim`` takes them).  ``calc.compute_stress`` is
        switched on."""
        force_step = torchsim_force_step(calc, cell, pbc, atomic_numbers, system_idx, with_stress=True)
        return cls(force_step, masses, timestep, temperature, friction, pressure, compressibility, taup, positions, cell,
                   system_idx, **kwargs)
