"""The host layer that the device-resident drivers share (``md.py``, ``md_batched.py``, ``relax.py``): the backend choice, the
checks of what ``force_step`` returned and of a cell, the ``Atoms`` and torch-sim adapters, the padded per-system layout, the noise
generator in numpy and the 3 x 3 determinant.  One statement of every rule and of every message."""

from __future__ import annotations

from types import SimpleNamespace
from typing import Dict, Tuple

import numpy as np
import torch

from ..data import AtomicDataDict

_M32 = 0xFFFFFFFF
_FLOATS = (torch.float32, torch.float64)


def select_backend(backend: str, device: torch.device) -> bool:
    """Whether the HIP kernels run: ``"hip"``, or ``"auto"`` on the GPU."""
    if backend not in ("auto", "hip", "aten"):
        raise ValueError(f"backend must be 'auto', 'hip' or 'aten', got {backend!r}")
    if backend == "hip" and device.type != "cuda":
        raise ValueError("backend='hip' needs device tensors: the kernels run on the GPU")
    return backend == "hip" or (backend == "auto" and device.type == "cuda")


def checked_forces(out, num_atoms: int, device: torch.device) -> torch.Tensor:
    """The forces of ``out`` (what ``force_step`` returned), detached and contiguous: ``[num_atoms, 3]`` float32 or float64."""
    f = out[AtomicDataDict.FORCE_KEY].detach()
    if tuple(f.shape) != (num_atoms, 3) or f.dtype not in _FLOATS:
        raise ValueError(f"force_step must return float32 or float64 forces [{num_atoms}, 3], got {f.dtype} {tuple(f.shape)}")
    if f.device != device:
        raise ValueError(f"mixed devices: positions on {device}, forces on {f.device}")
    return f.contiguous()


def checked_stress(out, num_systems: int, device: torch.device, what: str, where: str) -> torch.Tensor:
    """The stress of ``out``, detached and contiguous, as ``[num_systems, 3, 3]`` float32 or float64 (one system may give
    ``[3, 3]``).  ``what``: the shapes as the refusal names them; ``where``: how the refusal of a missing stress ends."""
    stress = out.get(AtomicDataDict.STRESS_KEY) if hasattr(out, "get") else None
    if stress is None:
        raise ValueError(f"stress: force_step must return it {where}")
    stress = stress.detach()
    if num_systems == 1 and tuple(stress.shape) == (3, 3):
        stress = stress.reshape(1, 3, 3)
    if tuple(stress.shape) != (num_systems, 3, 3) or stress.dtype not in _FLOATS:
        raise ValueError(f"stress: force_step must return float32 or float64 {what}, got {stress.dtype} {tuple(stress.shape)}")
    if stress.device != device:
        raise ValueError(f"mixed devices: positions on {device}, stress on {stress.device}")
    return stress.contiguous()


def check_cells(cells: torch.Tensor, single: bool) -> None:
    """Refuses a cell of ``cells`` (``[S, 3, 3]``; one host read) whose lattice vectors are not finite or span no volume."""
    host = cells.detach().to(torch.float64).reshape(-1, 3, 3).cpu().numpy()
    for s, c in enumerate(host):
        scale = float(np.prod(np.linalg.norm(c, axis=1)))
        if not np.isfinite(c).all() or not abs(float(np.linalg.det(c))) > 1e-12 * max(scale, 1e-300):
            raise ValueError(("cell" if single else f"cell of system {s}") + " is singular: its lattice vectors do not span a volume")


def state_arrays(state: Dict[str, object], num_atoms: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """``positions`` and ``velocities`` of a saved state, both ``[num_atoms, 3]``."""
    pos, vel = state["positions"], state["velocities"]
    if tuple(pos.shape) != (num_atoms, 3) or tuple(vel.shape) != (num_atoms, 3):
        raise ValueError(f"the state holds {tuple(pos.shape)} positions and {tuple(vel.shape)} velocities, this run has "
                         f"{num_atoms} atoms")
    return pos, vel


def atoms_tensors(atoms, device: torch.device, *names: str):
    """Float64 tensors on ``device`` read from an ``Atoms`` object, in the order of ``names``: ``"positions"``, ``"velocities"``
    (``None`` where the object holds none), ``"masses"``, ``"cell"`` (``[3, 3]``)."""
    out = []
    for name in names:
        value = getattr(atoms, "get_" + name)()
        if value is not None:
            value = np.asarray(value, dtype=np.float64)
            value = torch.as_tensor(value.reshape(3, 3) if name == "cell" else value).to(device)
        out.append(value)
    return out[0] if len(out) == 1 else tuple(out)


def torchsim_force_step(calc, cell, pbc, atomic_numbers, system_idx, with_stress: bool):
    """The ``force_step`` of a batch around a ``NequIPTorchSimCalc``: it hands ``calc`` a state with ``positions``,
    ``row_vector_cell``, ``pbc``, ``atomic_numbers`` and ``system_idx`` and returns its forces and per-system energies.  A
    calculator that was given the atomic numbers itself is not given them again.  ``with_stress``: a ``(positions, cell buffer)``
    callable that also returns the stresses (``calc.compute_stress`` is switched on); otherwise the cell is ``cell`` throughout."""
    if with_stress:
        calc.compute_stress = True
    numbers = None if getattr(calc, "atomic_numbers_in_init", False) else atomic_numbers
    state = SimpleNamespace(positions=None, row_vector_cell=None if with_stress else cell, pbc=pbc, atomic_numbers=numbers,
                            system_idx=system_idx)

    def force_step(pos, cell_buffer=None):
        state.positions = pos
        if with_stress:
            state.row_vector_cell = cell_buffer
        res = calc(state)
        out = {AtomicDataDict.FORCE_KEY: res["forces"], AtomicDataDict.TOTAL_ENERGY_KEY: res["energy"]}
        if with_stress:
            out[AtomicDataDict.STRESS_KEY] = res.get("stress")
        return out

    return force_step


def padded_layout(counts: np.ndarray, device: torch.device) -> Tuple[torch.Tensor, torch.Tensor]:
    """``(mask, idx)``, both ``[S, max count]`` (at least one column): atom ``k`` of system ``s`` is ``idx[s, k]`` where
    ``mask[s, k]``, for the per-system sums of the ATen forms."""
    width = max(int(counts.max()), 1)
    begin = np.concatenate([[0], np.cumsum(counts)])[:-1]
    k = np.arange(width)[None, :]
    inside = k < counts[:, None]
    return torch.from_numpy(inside).to(device), torch.from_numpy(np.where(inside, begin[:, None] + k, 0)).to(device)


def padded(per_atom: torch.Tensor, mask: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """``[S, max count]``: the values of every system's atoms in a row of their own, zeros behind them."""
    return torch.where(mask, per_atom[idx], torch.zeros((), dtype=per_atom.dtype, device=per_atom.device))


def _philox_numpy(seed, step, index) -> np.ndarray:
    """Philox4x32-10 in uint64 arithmetic (a product of two 32-bit words fits): the words ``[count, 4]`` for counter
    ``(index lo, index hi, step lo, step hi)`` and key ``(seed lo, seed hi)``.  Each argument is a Python int or a ``uint64``
    array; ints are spread over the arrays' length (``count = 1`` without an array)."""
    u = np.uint64
    mask, s32 = u(_M32), u(32)
    seed, step, index = np.broadcast_arrays(*(np.atleast_1d(np.asarray(t, dtype=np.uint64)) for t in (seed, step, index)))
    c0, c1, c2, c3 = index & mask, index >> s32, step & mask, step >> s32
    k0, k1 = seed & mask, seed >> s32
    for _ in range(10):
        p0, p1 = u(0xD2511F53) * c0, u(0xCD9E8D57) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0, k1 = (k0 + u(0x9E3779B9)) & mask, (k1 + u(0xBB67AE85)) & mask
    return np.stack([c0, c1, c2, c3], axis=1)


def _det3(c: torch.Tensor) -> torch.Tensor:
    """``[S]`` determinants of ``[S, 3, 3]`` by cofactors along the first row, in the order of the kernels."""
    return (c[:, 0, 0] * (c[:, 1, 1] * c[:, 2, 2] - c[:, 1, 2] * c[:, 2, 1])
            - c[:, 0, 1] * (c[:, 1, 0] * c[:, 2, 2] - c[:, 1, 2] * c[:, 2, 0])
            + c[:, 0, 2] * (c[:, 1, 0] * c[:, 2, 1] - c[:, 1, 1] * c[:, 2, 0]))
