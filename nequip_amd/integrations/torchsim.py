"""torch-sim calculator on top of the MI355X path (mirror of ``nequip/integrations/torchsim.py``, ``NequIPTorchSimCalc``).

``NequIPTorchSimCalc(model, device, transforms, atomic_numbers, system_idx)`` follows the reference's model interface: the
same constructor meaning, the same ``compute_forces`` / ``compute_stress`` switches, ``setup_from_system_idx``, the same
input validation errors and ``forward(state) -> {"energy": [S], "forces": [N, 3], "stress": [S, 3, 3]}`` for a state of S
systems.  What differs is the data path before the model: atomic numbers become type indices through a lookup table on
the device, and the whole batch gets its neighbour list from one batched device cell list
(``nqa_neighbor_list_batched_count/fill``, ``csrc/neighbor_list.hip``), with one host read per call (the edge count) where
the reference builds the graph of every system on its own.

torch-sim itself is optional: with ``torch_sim`` installed the class derives from its ``ModelInterface``; without it a
minimal stand-in base class (the properties the class below relies on) keeps it usable with any state object that has
``positions``, ``row_vector_cell``, ``pbc``, ``atomic_numbers`` and ``system_idx``.
"""

from __future__ import annotations

from typing import Callable, Dict, Optional, Sequence, Union

import torch

from ..data import AtomicDataDict
from ..data._nl import compute_neighborlist_
from ..data.chemistry import chemical_symbols, chemical_symbols_to_atomic_numbers_dict

try:  # pragma: no cover - torch_sim is not installed in the build container
    from torch_sim.models.interface import ModelInterface

    HAVE_TORCH_SIM = True
except Exception:  # noqa: BLE001
    HAVE_TORCH_SIM = False

    class ModelInterface(torch.nn.Module):  # minimal stand-in with the part of torch-sim's interface used below
        @property
        def device(self) -> torch.device:
            return self._device

        @property
        def dtype(self) -> torch.dtype:
            return self._dtype

        @property
        def compute_forces(self) -> bool:
            return self._compute_forces

        @property
        def compute_stress(self) -> bool:
            return self._compute_stress

        @property
        def memory_scales_with(self) -> str:
            return self._memory_scales_with


class NequIPTorchSimCalc(ModelInterface):
    """Energies, forces and stresses of a batch of systems through the HIP kernels (one GPU, all systems in one call).

    Args:
        model: an eager ``nequip_amd`` model (``NequIPGNNModel`` and the other builders), in eval mode
        device: a GPU device (there is no CPU path)
        transforms: data transforms applied to the input dict before the neighbour list
        atomic_numbers: ``[n_atoms]``; if given here, it cannot be given again in ``forward``
        system_idx: ``[n_atoms]`` system of every atom; with ``atomic_numbers`` and without it, all atoms are one system
        chemical_species_to_atom_type_map: chemical symbol -> model type name (dict), or the chemical symbols of the
            model's types in type order (list); default: the model's type names are chemical symbols
        r_max: neighbour-list cutoff; default: the model's ``r_max``
        prune_neighborlist: a model with per-edge-type cutoffs gets the typed (pruned) batched list; ``False``: the full
            ``r_max`` list (the same numbers, more edges)
    """

    def __init__(
        self,
        model: torch.nn.Module,
        device: Union[str, torch.device] = "cuda",
        transforms: Sequence[Callable] = (),
        atomic_numbers: Optional[torch.Tensor] = None,
        system_idx: Optional[torch.Tensor] = None,
        chemical_species_to_atom_type_map: Optional[Union[Dict[str, str], Sequence[str]]] = None,
        r_max: Optional[float] = None,
        prune_neighborlist: bool = True,
    ) -> None:
        super().__init__()
        if isinstance(device, str):
            device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("nequip_amd's torch-sim calculator runs on the GPU only (HIP kernels; there is no CPU path)")
        self._device = device
        self._dtype = torch.float64
        self._compute_forces = True
        self._compute_stress = True
        self._memory_scales_with = "n_atoms_x_density"

        if not isinstance(model, torch.nn.Module):
            raise TypeError("Invalid model type. Must be a torch.nn.Module.")
        if type(model).__name__ == "DictInputOutputWrapper":
            raise NotImplementedError("NequIPTorchSimCalc runs the eager nequip_amd model: compiled packages hold one frame")
        from ..nn.embedding.node import refuse_categorical_graph_fields

        refuse_categorical_graph_fields(model, "NequIPTorchSimCalc")
        r_max = r_max if r_max is not None else getattr(model, "r_max", None)
        if r_max is None:
            raise ValueError("no cutoff: pass r_max or a model with an r_max attribute")
        self.r_max = float(r_max)
        self.prune_neighborlist = bool(prune_neighborlist)
        from ..data.transforms import cutoff_table_from_model

        self._cutoff_table = cutoff_table_from_model(model, self.r_max) if self.prune_neighborlist else None

        # atomic number -> type index on the device (-1: not a species of the model)
        type_names = list(getattr(model, "type_names", []) or [])
        species = chemical_species_to_atom_type_map
        if species is None:
            species = type_names
        if isinstance(species, dict):
            type_of_symbol = {sym: type_names.index(name) for sym, name in species.items()}
        else:
            type_of_symbol = {sym: i for i, sym in enumerate(species)}
        if not type_of_symbol:
            raise ValueError("no chemical species mapping: pass chemical_species_to_atom_type_map or a model with type_names")
        lut = torch.full((len(chemical_symbols),), -1, dtype=torch.int64)
        for sym, t in type_of_symbol.items():
            if sym not in chemical_symbols_to_atomic_numbers_dict:
                raise ValueError(f"{sym!r} is not a chemical symbol")
            lut[chemical_symbols_to_atomic_numbers_dict[sym]] = t
        self._species = sorted(type_of_symbol)
        self.model = model.to(self._device)
        self.transforms = [t.to(self._device) if isinstance(t, torch.nn.Module) else t for t in transforms]
        self.register_buffer("type_of_atomic_number", lut.to(self._device), persistent=False)

        self.atomic_numbers_in_init = atomic_numbers is not None
        self.n_systems = 1
        if atomic_numbers is not None:
            if system_idx is None:
                system_idx = torch.zeros(len(atomic_numbers), dtype=torch.long, device=self._device)
            self.setup_from_system_idx(atomic_numbers, system_idx)

    @ModelInterface.compute_forces.setter
    def compute_forces(self, value: bool) -> None:
        self._compute_forces = value

    @ModelInterface.compute_stress.setter
    def compute_stress(self, value: bool) -> None:
        self._compute_stress = value

    @classmethod
    def from_compiled_model(cls, compile_path, device: Union[str, torch.device] = "cuda", **kwargs):
        raise NotImplementedError(
            "NequIPTorchSimCalc.from_compiled_model is not supported yet: loading a multi-system AOTInductor package "
            "(aot_export_model with batch_map={'graph': Dim} and the batch / num_atoms inputs) has not been tested with this "
            "calculator, and the default export takes one frame; build the calculator on the eager model instead")

    def setup_from_system_idx(self, atomic_numbers: torch.Tensor, system_idx: torch.Tensor) -> None:
        """Atomic numbers ``[n_atoms]`` and system indices ``[n_atoms]`` of the atoms: maps the numbers to type indices
        (one host read: the number of systems and the species check, as the reference reads the number of systems)."""
        atomic_numbers = atomic_numbers.to(self._device)
        system_idx = system_idx.to(device=self._device, dtype=torch.long)
        if atomic_numbers.numel() != system_idx.numel():
            raise ValueError("atomic_numbers and system_idx must have one entry per atom")
        z = atomic_numbers.view(-1).to(torch.long)
        lut = self.type_of_atomic_number
        if z.numel() > 0:
            zc = z.clamp(0, lut.numel() - 1)
            bad = (z != zc) | (lut[zc] < 0)
            first_bad = torch.where(bad, torch.arange(z.numel(), device=z.device), z.numel()).min()
            n_sys_m1, first = torch.stack([system_idx.max(), first_bad]).tolist()
            if first < z.numel():
                zbad = int(z[first])
                name = chemical_symbols[zbad] if 0 <= zbad < len(chemical_symbols) else str(zbad)
                raise ValueError(f"chemical species {name!r} (Z = {zbad}) is not among the model's types {self._species}")
            self.n_systems = int(n_sys_m1) + 1
            self.atom_types = lut[zc]
        else:
            self.n_systems = 1
            self.atom_types = z.clone()
        self.atomic_numbers = atomic_numbers
        self.system_idx = system_idx
        self.total_atoms = atomic_numbers.shape[0]

    def _numbers_changed(self, atomic_numbers: torch.Tensor) -> bool:
        known = getattr(self, "atomic_numbers", None)
        if known is None:
            return True
        if atomic_numbers is known:
            return False
        return atomic_numbers.shape != known.shape or not torch.equal(atomic_numbers.to(known.device), known)

    def forward(self, state) -> Dict[str, torch.Tensor]:
        """``{"energy": [S], "forces": [N, 3], "stress": [S, 3, 3]}`` of a state of S systems (forces / stress as
        ``compute_forces`` / ``compute_stress`` ask)."""
        atomic_numbers = getattr(state, "atomic_numbers", None)
        if atomic_numbers is None and not self.atomic_numbers_in_init:
            raise ValueError("Atomic numbers must be provided in either the constructor or forward.")
        if atomic_numbers is not None and self.atomic_numbers_in_init:
            raise ValueError("Atomic numbers cannot be provided in both the constructor and forward.")
        system_idx = getattr(state, "system_idx", None)
        if system_idx is None:
            if not hasattr(self, "system_idx"):
                raise ValueError("System indices must be provided if not set during initialization")
            system_idx = self.system_idx
        if atomic_numbers is not None and self._numbers_changed(atomic_numbers):
            self.setup_from_system_idx(atomic_numbers, system_idx)

        K = AtomicDataDict
        dev = self._device
        pos = state.positions.to(dev)
        cell = getattr(state, "row_vector_cell", None)
        S = cell.shape[0] if cell is not None and cell.dim() == 3 else self.n_systems
        pbc = state.pbc
        if isinstance(pbc, bool):
            pbc = torch.tensor([pbc] * 3, dtype=torch.bool, device=dev)
        pbc = pbc.to(device=dev, dtype=torch.bool)
        pbc = pbc.view(1, 3).expand(S, 3) if pbc.numel() == 3 else pbc.view(S, 3)
        system_idx = system_idx.to(device=dev, dtype=torch.long)
        num_nodes = torch.zeros(S, dtype=torch.long, device=dev).index_add_(0, system_idx, torch.ones_like(system_idx))
        data: Dict[str, torch.Tensor] = {
            K.POSITIONS_KEY: pos,
            K.PBC_KEY: pbc.contiguous(),
            K.BATCH_KEY: system_idx,
            K.NUM_NODES_KEY: num_nodes,
            K.ATOM_TYPE_KEY: self.atom_types,
            "atomic_numbers": self.atomic_numbers,
        }
        if cell is not None:
            data[K.CELL_KEY] = cell.to(dev).reshape(S, 3, 3).contiguous()
        for t in self.transforms:
            data = t(data)
        if K.EDGE_INDEX_KEY not in data:
            compute_neighborlist_(data, self.r_max, per_edge_type_cutoff=self._cutoff_table)
        data = {k: (v.contiguous() if torch.is_tensor(v) else v) for k, v in data.items()}

        out = self.model(data)

        results: Dict[str, torch.Tensor] = {}
        energy = out.get(K.TOTAL_ENERGY_KEY)
        results["energy"] = energy.view(-1).detach() if energy is not None else torch.zeros(S, device=dev)
        if self.compute_forces and out.get(K.FORCE_KEY) is not None:
            results["forces"] = out[K.FORCE_KEY].detach()
        if self.compute_stress and out.get(K.STRESS_KEY) is not None:
            results["stress"] = out[K.STRESS_KEY].detach()
        self.save_extra_outputs(out, results)
        return results

    def save_extra_outputs(self, out: Dict[str, torch.Tensor], results: Dict[str, torch.Tensor]) -> None:
        """Hook for subclasses (as in the reference)."""
