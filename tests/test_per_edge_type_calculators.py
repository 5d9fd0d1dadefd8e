"""Calculators on the pruned (typed) neighbour list of a model with per-edge-type cutoffs.

A small ``NequIPGNNModel`` with the water table (and an asymmetric one), with and without ZBL, through the ASE calculator, the
torch-sim calculator (boxes with different cells) and ``graphed_md=True``: energy, forces and stress on the pruned list against
``prune_neighborlist=False`` directly, and both against the float64 oracle (with ZBL: oracle of the same weights without the term, plus
the ATen restatement of the term) within the tolerances of ``tests/test_model_parity.py`` for this model class (energy
5e-5 x atoms / 5e-5, forces 5e-5 x max(1, max|F|) / 5e-5 and 1e-4 x max(1, max|F|) absolute, virial 5e-5 x atoms x max(1, max|F|) /
5e-4; stress = -virial / volume).  The pruned edge count is strictly smaller than the full one and equals a brute-force
count; a model without a table gets the identical list with either setting.
"""

import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch

from oracle import model as omodel

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import zbl_restatement as zr  # noqa: E402

R_MAX = 4.5
TABLES = {
    "water": {"H": {"H": 3.0, "O": 3.5}, "O": {"H": 3.5, "O": 4.5}},
    "asym": {"H": {"H": 3.0, "O": 4.0}, "O": {"H": 3.5}},
}
TOL = 5e-5


class FakeAtoms:
    def __init__(self, symbols, positions, cell, pbc=True):
        self._s, self._p = list(symbols), np.asarray(positions, dtype=np.float64)
        self._c = np.asarray(cell, dtype=np.float64)
        self._pbc = np.array([pbc] * 3, dtype=bool)

    def get_chemical_symbols(self):
        return self._s

    def get_positions(self):
        return self._p

    def get_cell(self):
        return self._c

    def get_pbc(self):
        return self._pbc

    def __len__(self):
        return len(self._s)


@dataclass
class SimState:
    positions: torch.Tensor
    row_vector_cell: torch.Tensor
    pbc: object
    atomic_numbers: Optional[torch.Tensor] = None
    system_idx: Optional[torch.Tensor] = None


def _cfg():
    return dict(r_max=R_MAX, num_layers=2, l_max=2, parity=False, num_features=8, radial_mlp_depth=1, radial_mlp_width=16,
                num_bessels=8, polynomial_cutoff_p=6, avg_num_neighbors=17.0, model_dtype="float32")


def _models(device, table, zbl):
    """(model under test, the same weights without ZBL for the oracle)."""
    from nequip_amd.model import NequIPGNNModel

    c = _cfg()
    args = dict(seed=4, model_dtype="float32", r_max=R_MAX, type_names=["H", "O"], num_layers=c["num_layers"], l_max=c["l_max"],
                parity=False, num_features=c["num_features"], radial_mlp_depth=1, radial_mlp_width=c["radial_mlp_width"],
                avg_num_neighbors=c["avg_num_neighbors"], per_edge_type_cutoff=table)
    plain = NequIPGNNModel(**args).to(device).eval()
    if not zbl:
        return plain, plain
    pp = {"_target_": "nequip.nn.pair_potential.ZBL", "chemical_species": ["H", "O"], "units": "metal"}
    return NequIPGNNModel(pair_potential=pp, **args).to(device).eval(), plain


def _weights(model):
    return {k.replace("model.func.", ""): v.detach().cpu() for k, v in model.state_dict().items()}


def _table_tensor(table):
    from nequip_amd.nn.embedding import cutoff_partialdict_to_tensor

    return None if table is None else cutoff_partialdict_to_tensor(table, ["H", "O"], R_MAX)


def _reference(pos, types, cell, table, plain, zbl):
    """float64 oracle on the full host-built r_max list: energy, forces [N, 3], virial [3, 3]."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.utils import synthetic as syn

    data = syn.make_data(pos, types, R_MAX, cell)
    cfg = _cfg()
    tt = _table_tensor(table)
    if tt is not None:
        cfg["per_edge_type_cutoff_table"] = tt
    ref = omodel.energy_forces(data, cfg, _weights(plain), with_virial=True)
    e, f, w = ref["total_energy"].view(()).clone(), ref["forces"].clone(), ref["virial"].view(3, 3).clone()
    if zbl:
        p = data[K.POSITIONS_KEY].clone().requires_grad_(True)
        eps = torch.zeros(3, 3, dtype=torch.float64, requires_grad=True)
        sym = 0.5 * (eps + eps.t())
        c = data[K.CELL_KEY].view(3, 3)
        ei, t = data[K.EDGE_INDEX_KEY], data[K.ATOM_TYPE_KEY]
        p2 = p + p @ sym
        vec = p2[ei[1]] - p2[ei[0]] + data[K.EDGE_CELL_SHIFT_KEY] @ (c + c @ sym)
        recip = 1.0 / R_MAX if tt is None else tt.reciprocal()[t[ei[0]], t[ei[1]]]
        zt = torch.tensor([1.0, 8.0], dtype=torch.float64)
        ez = zr.atom_energy(vec, ei, zt[t], recip, len(t), model_dtype=torch.float32).sum()
        gp, ge = torch.autograd.grad(ez, [p, eps])
        e, f, w = e + ez.detach(), f - gp, w - ge
    return e, f, w


def _brute_count(pos, types, cell, table_tensor):
    """Edges with r < r_max and r <= rc[t_i][t_j], by enumeration over images (float64); asserts that no distance lies
    within 1e-9 A of a cutoff."""
    import itertools

    pos, cell, rc = np.asarray(pos), np.asarray(cell), table_tensor.numpy()
    heights = 1.0 / np.linalg.norm(np.linalg.inv(cell), axis=0)
    reach = [int(np.ceil(R_MAX / h)) + 1 for h in heights]
    count, gap = 0, np.inf
    bounds = np.unique(np.concatenate([[R_MAX], rc.reshape(-1)]))
    for S in itertools.product(*[range(-r, r + 1) for r in reach]):
        d = pos[None, :, :] + (np.array(S, dtype=np.float64) @ cell)[None, None, :] - pos[:, None, :]
        r = np.sqrt((d * d).sum(-1))
        if S == (0, 0, 0):
            np.fill_diagonal(r, np.inf)
        near = r[r < R_MAX + 1e-6]
        if near.size:
            gap = min(gap, np.abs(near[:, None] - bounds[None, :]).min())
        count += int(((r < R_MAX) & (r <= rc[types[:, None], types[None, :]])).sum())
    assert gap > 1e-9, f"a distance lies within {gap:.2e} A of a cutoff: choose another seed"
    return count


def _check(what, e, f, w_or_none, ref, n, vol=None, stress=None):
    re, rf, rw = ref
    fscale = float(rf.abs().max())
    de, df = float(abs(e - re)), float((f - rf).abs().max())
    print(f"[{what}] N={n} |dE|={de:.3e} max|dF|={df:.3e} (max|F|={fscale:.3e})")
    torch.testing.assert_close(torch.as_tensor(e, dtype=torch.float64).view(()), re, atol=TOL * n, rtol=TOL)
    torch.testing.assert_close(f.to(torch.float64), rf, atol=TOL * max(1.0, fscale), rtol=TOL)
    assert df < 1e-4 * max(1.0, fscale)
    if stress is not None:
        torch.testing.assert_close(stress.to(torch.float64).view(3, 3), -rw / vol, atol=TOL * n * max(1.0, fscale) / vol,
                                   rtol=10 * TOL)


def _check_pruned_vs_full(what, pruned, full, n, vol):
    """``(energy, forces [N, 3], stress [3, 3])`` on the pruned list against the full list, directly.  The two differ only
    by edges whose every contribution is an exact zero, so float32 summation order is all that separates them: the
    model-parity tolerances (energy 5e-5 x atoms / 5e-5, forces 5e-5 x max(1, max|F|) / 5e-5, stress the virial's 5e-5 x atoms
    x max(1, max|F|) / volume, 5e-4 relative) bound it with room to spare."""
    (e1, f1, s1), (e0, f0, s0) = pruned, full
    f1, f0, s1, s0 = f1.to(torch.float64), f0.to(torch.float64), s1.to(torch.float64).view(3, 3), s0.to(torch.float64).view(3, 3)
    fscale = float(f0.abs().max())
    print(f"[{what}] pruned vs full: |dE|={abs(e1 - e0):.3e} max|dF|={float((f1 - f0).abs().max()):.3e} "
          f"max|dS|={float((s1 - s0).abs().max()):.3e}")
    torch.testing.assert_close(torch.tensor(e1, dtype=torch.float64), torch.tensor(e0, dtype=torch.float64), atol=TOL * n,
                               rtol=TOL)
    torch.testing.assert_close(f1, f0, atol=TOL * max(1.0, fscale), rtol=TOL)
    torch.testing.assert_close(s1, s0, atol=TOL * n * max(1.0, fscale) / vol, rtol=10 * TOL)


def _box(n_side, seed, scale=1.0):
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side, seed=seed)
    assert list(names) == ["H", "O"]
    return np.asarray(pos) * scale, np.asarray(types), np.asarray(cell, dtype=np.float64).reshape(3, 3) * scale


def _voigt_to_full(v):
    return torch.tensor([[v[0], v[5], v[4]], [v[5], v[1], v[3]], [v[4], v[3], v[2]]], dtype=torch.float64)


@pytest.mark.gpu
@pytest.mark.parametrize("zbl", [False, True], ids=["plain", "zbl"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_ase_calculator_pruned_vs_full_vs_oracle(device, table, zbl):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.integrations.ase import NequIPCalculator

    pos, types, cell = _box(3, 11)
    model, plain = _models(device, TABLES[table], zbl)
    atoms = FakeAtoms([["H", "O"][t] for t in types], pos, cell)
    ref = _reference(pos, types, cell, TABLES[table], plain, zbl)
    vol = abs(np.linalg.det(cell))
    res, counts = {}, {}
    for prune in (True, False):
        calc = NequIPCalculator(model, device, r_max=R_MAX, prune_neighborlist=prune)
        counts[prune] = int(calc.atoms_to_data(atoms)[K.EDGE_INDEX_KEY].shape[1])
        e, f, s = calc.get_potential_energy(atoms), calc.get_forces(atoms), calc.get_stress(atoms)
        res[prune] = (float(e), torch.as_tensor(f), _voigt_to_full(s))
        _check(f"ase {table} zbl={zbl} prune={prune}", res[prune][0], res[prune][1], None, ref, len(pos), vol, res[prune][2])
    _check_pruned_vs_full(f"ase {table} zbl={zbl}", res[True], res[False], len(pos), vol)
    assert counts[True] < counts[False]
    assert counts[True] == _brute_count(pos, types, cell, _table_tensor(TABLES[table]))
    assert counts[False] == _brute_count(pos, types, cell, torch.full((2, 2), R_MAX, dtype=torch.float64))


@pytest.mark.gpu
@pytest.mark.parametrize("zbl", [False, True], ids=["plain", "zbl"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_torchsim_calculator_pruned_vs_full_vs_oracle(device, table, zbl, monkeypatch):
    from nequip_amd.data import _nl
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc

    boxes = [_box(2, 21), _box(3, 22, scale=1.03), _box(2, 23, scale=0.98)]
    model, plain = _models(device, TABLES[table], zbl)
    refs = [_reference(p, t, c, TABLES[table], plain, zbl) for p, t, c in boxes]
    state = SimState(
        positions=torch.tensor(np.concatenate([b[0] for b in boxes]), dtype=torch.float64, device=device),
        row_vector_cell=torch.tensor(np.stack([b[2] for b in boxes]), dtype=torch.float64, device=device), pbc=True,
        atomic_numbers=torch.tensor(np.concatenate([[[1, 8][t] for t in b[1]] for b in boxes]), device=device),
        system_idx=torch.repeat_interleave(torch.arange(3), torch.tensor([len(b[0]) for b in boxes])).to(device))
    seen = []
    real = _nl._compute_neighborlist_batched

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append(int(out[0].shape[1]))
        return out

    monkeypatch.setattr(_nl, "_compute_neighborlist_batched", spy)
    monkeypatch.delenv("NQA_NL_PER_FRAME", raising=False)
    counts, res = {}, {}
    for prune in (True, False):
        calc = NequIPTorchSimCalc(model, device=device, prune_neighborlist=prune)
        out = calc(state)
        counts[prune] = seen[-1]
        off, res[prune] = 0, []
        for s, (b, ref) in enumerate(zip(boxes, refs)):
            n = len(b[0])
            res[prune].append((float(out["energy"][s]), out["forces"][off:off + n].cpu().clone(), out["stress"][s].cpu().clone()))
            _check(f"torchsim {table} zbl={zbl} prune={prune} system {s}", *res[prune][-1][:2], None, ref, n,
                   abs(np.linalg.det(b[2])), res[prune][-1][2])
            off += n
    for s, b in enumerate(boxes):
        _check_pruned_vs_full(f"torchsim {table} zbl={zbl} system {s}", res[True][s], res[False][s], len(b[0]),
                              abs(np.linalg.det(b[2])))
    assert counts[True] < counts[False]
    assert counts[True] == sum(_brute_count(p, t, c, _table_tensor(TABLES[table])) for p, t, c in boxes)


@pytest.mark.gpu
@pytest.mark.parametrize("zbl", [False, True], ids=["plain", "zbl"])
@pytest.mark.parametrize("table", sorted(TABLES))
def test_graphed_md_pruned_vs_full_vs_oracle(device, table, zbl):
    from nequip_amd.integrations.ase import NequIPCalculator

    pos, types, cell = _box(3, 31)
    model, plain = _models(device, TABLES[table], zbl)
    atoms = FakeAtoms([["H", "O"][t] for t in types], pos, cell)
    ref = _reference(pos, types, cell, TABLES[table], plain, zbl)
    vol = abs(np.linalg.det(cell))
    counts, res = {}, {}
    for prune in (True, False):
        calc = NequIPCalculator(model, device, r_max=R_MAX, graphed_md=True, prune_neighborlist=prune)
        for _ in range(2):  # capture, then a replay
            e, f, s = calc.get_potential_energy(atoms), calc.get_forces(atoms), calc.get_stress(atoms)
        step = calc._graphed[1]
        assert step.num_captures >= 1 and step.num_eager_fallbacks == 0
        counts[prune] = step.last_num_edges
        res[prune] = (float(e), torch.as_tensor(f).clone(), _voigt_to_full(s))
        _check(f"graphed {table} zbl={zbl} prune={prune}", *res[prune][:2], None, ref, len(pos), vol, res[prune][2])
    _check_pruned_vs_full(f"graphed {table} zbl={zbl}", res[True], res[False], len(pos), vol)
    tt = _table_tensor(TABLES[table])
    assert counts[True] < counts[False]
    assert counts[True] == _brute_count(pos, types, cell, torch.maximum(tt, tt.t()))  # (the padded list symmetrises)


@pytest.mark.gpu
def test_model_without_table_gets_the_same_list_either_way(device):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.integrations.ase import NequIPCalculator

    pos, types, cell = _box(3, 41)
    model, _ = _models(device, None, False)
    atoms = FakeAtoms([["H", "O"][t] for t in types], pos, cell)
    lists = []
    for prune in (True, False):
        calc = NequIPCalculator(model, device, r_max=R_MAX, prune_neighborlist=prune)
        assert calc._cutoff_table is None
        d = calc.atoms_to_data(atoms)
        lists.append((d[K.EDGE_INDEX_KEY], d[K.EDGE_CELL_SHIFT_KEY]))
    assert torch.equal(lists[0][0], lists[1][0]) and torch.equal(lists[0][1], lists[1][1])
