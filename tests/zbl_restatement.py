"""A float64 ATen restatement of the ZBL pair term (nequip/nn/pair_potential.py:230-389; LAMMPS pair_style zbl), written
from the formula with the reference's dtype rule: Z and Z^0.23 (and their sum) in the model dtype, the cutoff polynomial
rounded to the model dtype, everything else float64.  Differentiable to any order; runs on any device."""
import torch

QQR2E = {"metal": 14.399645, "real": 332.06371}
PSI = ((0.02817, -0.20162), (0.28022, -0.40290), (0.50986, -0.94229), (0.18175, -3.19980))
A0 = 0.46850


def edge_energy(vec, z_i, z_j, rmax_recip, p: float = 6.0, model_dtype=torch.float64, units: str = "metal"):
    """[E] float64 energy of each directed edge (half of the pair's).  ``z_i`` / ``z_j``: [E] atomic numbers;
    ``rmax_recip``: float or [E] float64."""
    zi, zj = z_i.to(model_dtype), z_j.to(model_dtype)
    r = vec.square().sum(-1).sqrt()
    x = ((zi.pow(0.23) + zj.pow(0.23)) * r) / A0
    psi = sum(c * (d * x).exp() for c, d in PSI)
    eng = (0.5 * QQR2E[units]) * ((zi * zj) / r) * psi
    u = r * rmax_recip
    cut = 1.0 - ((p + 1.0) * (p + 2.0) / 2.0) * u.pow(p) + p * (p + 2.0) * u.pow(p + 1.0) \
        - (p * (p + 1.0) / 2) * u.pow(p + 2.0)
    cut = (cut * (u < 1.0)).to(model_dtype)
    return eng * cut


def atom_energy(vec, edge_index, z_of_atom, rmax_recip, num_nodes: int, **kw):
    """[N, 1] float64 per-atom sums over the centre atom ``edge_index[0]``."""
    e = edge_energy(vec, z_of_atom[edge_index[0]], z_of_atom[edge_index[1]], rmax_recip, **kw)
    return torch.zeros(num_nodes, dtype=torch.float64, device=vec.device).index_add(0, edge_index[0], e).unsqueeze(-1)
