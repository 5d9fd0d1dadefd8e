"""ZBL core-repulsion pair term (mirror of ``nequip/nn/pair_potential.py:230-389``, ``ZBL``): same constructor, irreps contract,
buffers (``atomic_numbers`` in the default dtype, ``_qqr2exesquare`` float64 and already halved) and ``cutoff`` submodule, so
state dicts load either way.  The arithmetic is the HIP kernels of ``csrc/pair_potential.hip`` (``_pair_potential_ops.py``):
one pass over the centre-atom CSR per direction instead of ~15 ATen kernels and an atomic ``index_add``.

The reference reads ``normed_edge_lengths``; the native ``EdgeLengthNormalizer`` leaves the reciprocal cutoffs instead
(``_nqa_rmax_recip``, and ``_nqa_rmax_recip_edge`` with per-edge-type cutoffs) and the kernel forms ``r / rmax`` itself."""

from typing import List

import torch

from ..data import AtomicDataDict
from ..data.chemistry import chemical_symbols_to_atomic_numbers_dict
from ..o3.irreps import Irreps
from ..utils.tracing import traceable
from ._graph_mixin import GraphModuleMixin
from .embedding.cutoffs import PolynomialCutoff
from .utils import with_edge_vectors_

_QQR2E = {"metal": 14.399645 * (1.0) ** 2, "real": 332.06371 * (1.0) ** 2}  # LAMMPS force->qqr2e * qelectron^2


class ZBL(GraphModuleMixin, torch.nn.Module):
    """`ZBL <https://docs.lammps.org/pair_zbl.html>`_ pair potential energy term, added to ``per_atom_energy_field``.

    Args:
        type_names: type names known by the model
        chemical_species: chemical symbol of each type, e.g. ``[C, H, O]``
        units: LAMMPS units of the data, ``metal`` or ``real``
        polynomial_cutoff_p: exponent of the polynomial cutoff (default ``6``)
    """

    def __init__(self, type_names: List[str], chemical_species: List[str], units: str, polynomial_cutoff_p: float = 6.0,
                 per_atom_energy_field: str = AtomicDataDict.PER_ATOM_ENERGY_KEY, irreps_in=None):
        super().__init__()
        num_types = len(type_names)
        self.per_atom_energy_field = per_atom_energy_field
        self._init_irreps(irreps_in=irreps_in, required_irreps_in=[AtomicDataDict.NORM_LENGTH_KEY],
                          irreps_out={self.per_atom_energy_field: "0e"})
        if self.per_atom_energy_field in self.irreps_in:
            energy_irreps = Irreps(self.irreps_in[self.per_atom_energy_field])
            assert all(ir.l == 0 for _, ir in energy_irreps), (
                f"{self.per_atom_energy_field} must be scalar irreps, found {energy_irreps}")
            self.irreps_out[self.per_atom_energy_field] = energy_irreps

        assert len(chemical_species) == num_types
        atomic_numbers = [chemical_symbols_to_atomic_numbers_dict[chemical_species[t]] for t in range(num_types)]
        if min(atomic_numbers) < 1:
            raise ValueError(
                f"Your chemical symbols don't seem valid (minimum atomic number is {min(atomic_numbers)} < 1); did you try "
                "to use fake chemical symbols for arbitrary atom types?")
        self.register_buffer("atomic_numbers", torch.as_tensor(atomic_numbers, dtype=torch.get_default_dtype()))
        # half the energy on each of (i <- j), (j <- i)
        self.register_buffer("_qqr2exesquare", torch.as_tensor(_QQR2E[units], dtype=torch.float64) * 0.5)
        self.cutoff = PolynomialCutoff(polynomial_cutoff_p)
        self.model_dtype = torch.get_default_dtype()

    def _z_table(self) -> torch.Tensor:
        """``[T, 2]`` float64 (Z, Z^0.23), both formed in the buffer's dtype on its device as the reference's
        ``torch.pow(Zi, 0.23)`` does.  Eagerly cached per buffer state (``load_state_dict``, ``.to()`` and in-place changes
        all change the key); a traced graph forms it from the buffer."""
        z = self.atomic_numbers
        if traceable():
            return torch.stack([z, torch.pow(z, 0.23)], dim=-1).to(torch.float64)
        key = (z.data_ptr(), z._version, z.device, z.dtype)
        cached = self.__dict__.get("_zt_cache")
        if cached is None or cached[0] != key:
            if z.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("ZBL: evaluate the model once before capturing it (its constant table is built eagerly)")
            with torch.no_grad():
                zt = torch.stack([z, torch.pow(z, 0.23)], dim=-1).to(torch.float64).contiguous()
            cached = self.__dict__["_zt_cache"] = (key, zt)
        return cached[1]

    def forward(self, data: AtomicDataDict.Type) -> AtomicDataDict.Type:
        K = AtomicDataDict
        data = with_edge_vectors_(data, with_lengths=False)
        if "_nqa_rmax_recip" not in data:
            raise RuntimeError("ZBL reads the reciprocal cutoffs that nequip_amd's EdgeLengthNormalizer leaves in the data "
                               "(`_nqa_rmax_recip`): put that module before it")
        # (with per-atom energies already present, their row count is the number of centres: local atoms of a local-ghost
        # list, nequip/nn/pair_potential.py:360-363)
        args = (data[K.EDGE_VECTORS_KEY], data.get(self.per_atom_energy_field), data[K.EDGE_INDEX_KEY],
                data[K.ATOM_TYPE_KEY].view(-1), self._z_table(), self._qqr2exesquare, data.get("_nqa_rmax_recip_edge"),
                float(data["_nqa_rmax_recip"]), float(self.cutoff.p), self.model_dtype == torch.float32)
        if traceable():
            from ._pair_potential_ops import zbl_op

            data[self.per_atom_energy_field] = zbl_op(*args)
        else:
            from ._pair_potential_ops import zbl

            data[self.per_atom_energy_field] = zbl(*args)
        return data
