#!/usr/bin/env python3
"""Golden vectors of the ZBL pair term produced by the REFERENCE's own module (``nequip/nn/pair_potential.py:230-389``,
``ZBL`` after the reference's ``EdgeLengthNormalizer``), imported with the stand-ins of ``make_reference_golden.py``.

A seeded periodic box of five species (H, C, O, Cu, Au), its edge list taken a little beyond ``r_max`` (so that edges beyond
the cutoff are in it), with a plain cutoff and with per-edge-type cutoffs, in a float32 and a float64 model dtype.  Recorded
per case: the per-atom energies without and with incoming per-atom energies (``pe_in``), ``d(sum_n w_n E_n) / d edge_vec``
for random per-atom weights ``w``, the state-dict keys, buffer dtypes and values.

    python tests/golden/make_zbl_golden.py     # needs the reference tree; rewrites tests/golden/ref_zbl.npz

``zbl_lammps.npy`` next to it is the reference's LAMMPS ``pair_style zbl`` output (``tests/unit/model/test_pair/zbl.npy``
there, produced by its ``zbl_data.lmps``), copied as data: rows ``r, Zi, Zj, pe, fx_i, fx_j`` for two atoms at distance r
along x, Z in {1, 6, 7, 8, 29, 79}.
"""

import itertools
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_reference_golden as mrg  # noqa: E402

SPECIES = ["H", "C", "O", "Cu", "Au"]
R_MAX = 3.0
PER_EDGE_TYPE = {"H": 2.0, "C": {"O": 2.5, "Cu": 2.2}, "Au": 2.8}


def box(seed: int = 20261016, n: int = 40, L: float = 7.0, r_min: float = 0.45, r_list: float = R_MAX + 0.75):
    g = np.random.default_rng(seed)
    pos = []
    while len(pos) < n:
        p = g.uniform(0, L, 3)
        if all(np.linalg.norm((p - q + L / 2) % L - L / 2) > r_min for q in pos):
            pos.append(p)
    pos = np.array(pos)
    cell = np.eye(3) * L
    types = g.integers(0, len(SPECIES), n)
    ei, sh = [], []
    for i, j in itertools.product(range(n), range(n)):
        for s in itertools.product((-1, 0, 1), repeat=3):
            if i == j and s == (0, 0, 0):
                continue
            if np.linalg.norm(pos[j] - pos[i] + np.array(s) @ cell) < r_list:
                ei.append((i, j))
                sh.append(s)
    return pos, cell, types, np.array(ei).T.copy(), np.array(sh, dtype=np.float64)


def main():
    K = mrg._import_reference()[0]
    from nequip.nn.embedding._edge import EdgeLengthNormalizer
    from nequip.nn.pair_potential import ZBL

    pos, cell, types, ei, sh = box()
    vec0 = torch.from_numpy(pos[ei[1]] - pos[ei[0]] + sh @ cell)
    g = torch.Generator().manual_seed(7)
    w = torch.rand(len(pos), 1, generator=g, dtype=torch.float64) + 0.5
    pe_in = torch.randn(len(pos), 1, generator=g, dtype=torch.float64)
    out = dict(pos=pos, cell=cell, atom_types=types, edge_index=ei, edge_cell_shift=sh, weights=w.numpy(),
               pe_in=pe_in.numpy(), species=np.array(SPECIES), r_max=np.float64(R_MAX))
    for dtype, per in itertools.product((torch.float32, torch.float64), (False, True)):
        tag = f"{str(dtype)[6:]}_{'per' if per else 'plain'}"
        prev = torch.get_default_dtype()
        torch.set_default_dtype(dtype)
        try:
            norm = EdgeLengthNormalizer(r_max=R_MAX, type_names=SPECIES, per_edge_type_cutoff=PER_EDGE_TYPE if per else None)
            zbl = ZBL(type_names=SPECIES, chemical_species=SPECIES, units="metal", polynomial_cutoff_p=6,
                      irreps_in=norm.irreps_out)
        finally:
            torch.set_default_dtype(prev)
        for with_pe in (False, True):
            vec = vec0.clone().requires_grad_(True)
            data = {K.EDGE_VECTORS_KEY: vec, K.EDGE_INDEX_KEY: torch.from_numpy(ei),
                    K.ATOM_TYPE_KEY: torch.from_numpy(types), K.POSITIONS_KEY: torch.from_numpy(pos)}
            if with_pe:
                data[K.PER_ATOM_ENERGY_KEY] = pe_in.clone()
            data = zbl(norm(data))
            pe = data[K.PER_ATOM_ENERGY_KEY]
            (gvec,) = torch.autograd.grad((pe * w).sum(), [vec])
            key = f"{tag}_{'pe' if with_pe else 'nope'}"
            out[f"{key}_energy"] = pe.detach().numpy()
            out[f"{key}_g_edge_vec"] = gvec.numpy()
        if per:
            out[f"{tag}_rmax_recip"] = norm._rmax_recip.detach().double().numpy()
        sd = zbl.state_dict()
        out[f"{tag}_state_keys"] = np.array(list(sd.keys()))
        out[f"{tag}_state_dtypes"] = np.array([str(v.dtype) for v in sd.values()])
        for k, v in sd.items():
            out[f"{tag}_state_{k}"] = v.detach().double().numpy()
    np.savez_compressed(os.path.join(HERE, "ref_zbl.npz"), **out)
    print("wrote", os.path.join(HERE, "ref_zbl.npz"), "edges:", ei.shape[1])


if __name__ == "__main__":
    main()
