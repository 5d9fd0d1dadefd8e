"""ZBL pair term, CPU side: the ATen restatement the GPU tests compare against is anchored to LAMMPS (`zbl_lammps.npy`) and
to the reference's own module (`ref_zbl.npz`); the native module keeps the reference's state dict, irreps contract and
errors; the builders place it where the reference does; `enable_NequipAMD_full` converts it; the kernels compile without
spills."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "scripts"))
import zbl_restatement as zr  # noqa: E402

SPECIES = ["H", "C", "O", "Cu", "Au"]
Z = {"H": 1, "C": 6, "N": 7, "O": 8, "Cu": 29, "Au": 79}


def lammps_pairs(rmax: float = 9.0, p: float = 80.0):
    """(rows, pe, f_i, f_j) of the restatement for the two-atom LAMMPS configurations with r < 8 (the reference test's
    setup: r_max 9, p 80, so that the cutoff is irrelevant)."""
    d = np.load(os.path.join(GOLDEN, "zbl_lammps.npy"))
    d = d[d[:, 0] < 8.0]
    r = torch.tensor(d[:, 0], dtype=torch.float64)
    vec = torch.stack([r, torch.zeros_like(r), torch.zeros_like(r)], -1).requires_grad_(True)  # x_j - x_i
    zi, zj = torch.tensor(d[:, 1], dtype=torch.float64), torch.tensor(d[:, 2], dtype=torch.float64)
    # both directed edges of the pair: (i <- j) with vec, (j <- i) with -vec
    e = zr.edge_energy(vec, zi, zj, 1.0 / rmax, p) + zr.edge_energy(-vec, zj, zi, 1.0 / rmax, p)
    (g,) = torch.autograd.grad(e.sum(), [vec])
    return d, e.detach().numpy(), g[:, 0].numpy(), -g[:, 0].numpy()  # f_i = -dE/dx_i = +dE/dvec_x


def test_restatement_reproduces_lammps():
    d, pe, fi, fj = lammps_pairs()
    assert len(d) > 1500
    np.testing.assert_allclose(pe, d[:, 3], atol=1e-4)
    np.testing.assert_allclose(fi, d[:, 4], atol=1e-5)
    np.testing.assert_allclose(fj, d[:, 5], atol=1e-5)


def _golden():
    return np.load(os.path.join(GOLDEN, "ref_zbl.npz"))


def restated_case(g, dtype: str, per: bool, with_pe: bool, device="cpu"):
    """(per-atom energies, d(sum w E)/d edge_vec) of the restatement on the fixture's graph."""
    types = torch.tensor(g["atom_types"], device=device)
    ei = torch.tensor(g["edge_index"], device=device)
    vec = torch.tensor(g["pos"][g["edge_index"][1]] - g["pos"][g["edge_index"][0]] + g["edge_cell_shift"] @ g["cell"],
                       device=device).requires_grad_(True)
    zt = torch.tensor([Z[s] for s in SPECIES], dtype=torch.float64, device=device)
    rmax = 1.0 / float(g["r_max"])
    if per:
        rmax = torch.tensor(g[f"{dtype}_per_rmax_recip"], device=device)[types[ei[0]] * len(SPECIES) + types[ei[1]]]
    pe = zr.atom_energy(vec, ei, zt[types], rmax, len(types), model_dtype=getattr(torch, dtype))
    if with_pe:
        pe = pe + torch.tensor(g["pe_in"], device=device)
    (gv,) = torch.autograd.grad((pe * torch.tensor(g["weights"], device=device)).sum(), [vec])
    return pe.detach(), gv


CASES = [(dt, per, pe) for dt in ("float32", "float64") for per in (False, True) for pe in (False, True)]


@pytest.mark.parametrize("dtype,per,with_pe", CASES)
def test_restatement_reproduces_reference_module(dtype, per, with_pe):
    g = _golden()
    key = f"{dtype}_{'per' if per else 'plain'}_{'pe' if with_pe else 'nope'}"
    pe, gv = restated_case(g, dtype, per, with_pe)
    np.testing.assert_allclose(pe.numpy(), g[f"{key}_energy"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(gv.numpy(), g[f"{key}_g_edge_vec"], rtol=1e-9, atol=1e-11)
    # the fixture has edges beyond the cutoff (and per-edge-type cutoffs below r_max): their gradient rows are zero
    assert (np.abs(g[f"{key}_g_edge_vec"]).sum(-1) == 0).sum() > 10


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_native_module_state_dict_matches_reference(dtype):
    from nequip_amd.model.nequip_models import torch_default_dtype
    from nequip_amd.nn import ZBL

    g = _golden()
    with torch_default_dtype(getattr(torch, dtype)):
        m = ZBL(type_names=SPECIES, chemical_species=SPECIES, units="metal", polynomial_cutoff_p=6,
                irreps_in={"normed_edge_lengths": "1x0e"})
    sd = m.state_dict()
    tag = f"{dtype}_plain"
    assert list(sd.keys()) == list(g[f"{tag}_state_keys"])
    assert [str(v.dtype) for v in sd.values()] == list(g[f"{tag}_state_dtypes"])
    for k, v in sd.items():
        np.testing.assert_array_equal(v.double().numpy(), g[f"{tag}_state_{k}"])
    assert m.irreps_out["atomic_energy"] is not None and float(m.cutoff.p) == 6.0


def test_native_module_errors_and_irreps_contract():
    from nequip_amd.nn import ZBL

    irr = {"normed_edge_lengths": "1x0e"}
    with pytest.raises(ValueError, match="minimum atomic number is 0"):
        ZBL(type_names=["A", "B"], chemical_species=["X", "H"], units="metal", irreps_in=irr)
    with pytest.raises(KeyError):
        ZBL(type_names=["A"], chemical_species=["Qq"], units="metal", irreps_in=irr)
    with pytest.raises(KeyError):
        ZBL(type_names=["H"], chemical_species=["H"], units="lj", irreps_in=irr)
    with pytest.raises(ValueError, match="normed_edge_lengths"):
        ZBL(type_names=["H"], chemical_species=["H"], units="metal", irreps_in={})
    m = ZBL(type_names=["H", "O"], chemical_species=["H", "O"], units="real", irreps_in=irr)
    assert float(m._qqr2exesquare) == 332.06371 * 0.5 and m.atomic_numbers.tolist() == [1.0, 8.0]


def _model(pair_potential=None, **kw):
    from nequip_amd.model import NequIPGNNModel

    args = dict(seed=0, model_dtype="float32", r_max=4.0, type_names=["H", "O"], num_layers=2, l_max=1, num_features=16,
                avg_num_neighbors=20.0, per_type_energy_shifts={"H": -1.0, "O": -2.0})
    args.update(kw)
    return NequIPGNNModel(pair_potential=pair_potential, **args)


ZBL_CFG = {"_target_": "nequip.nn.pair_potential.ZBL", "chemical_species": ["H", "O"], "units": "metal"}


def test_builder_appends_pair_potential_where_the_reference_does():
    from nequip_amd.nn import ZBL

    m = _model(ZBL_CFG)
    seq = m.model.func
    names = list(seq._modules.keys())
    assert names[-3:] == ["per_type_energy_scale_shift", "pair_potential", "total_energy_sum"]
    assert isinstance(seq.pair_potential, ZBL) and seq.pair_potential.atomic_numbers.dtype == torch.float32
    # the fused energy head is planned as without the term: readout and scale / shift stay adjacent
    assert seq.per_atom_energy_readout.__dict__["_scale_shift"] == [seq.per_type_energy_scale_shift]
    assert seq.layer1_convnet.defer_gate
    # the only new state-dict entries are the term's buffers; the other weights are the plain model's
    plain = _model(None).state_dict()
    sd = m.state_dict()
    assert set(sd) - set(plain) == {"model.func.pair_potential.atomic_numbers", "model.func.pair_potential._qqr2exesquare"}
    assert all(torch.equal(plain[k], sd[k]) for k in plain)
    assert m.model._energy_seed_allowed()
    native = _model(dict(ZBL_CFG, _target_="nequip_amd.nn.pair_potential.ZBL", type_names=["ignored"]))
    assert native.model.func.pair_potential.atomic_numbers.tolist() == [1.0, 8.0]


def test_builder_rejects_other_pair_potentials():
    with pytest.raises(NotImplementedError, match="LennardJones"):
        _model({"_target_": "nequip.nn.pair_potential.LennardJones", "lj_sigma": 1.0})


def test_zbl_pair_potential_builder():
    from nequip_amd.model import ZBLPairPotential

    m = ZBLPairPotential(r_max=4.0, type_names=["H", "O"], chemical_species=["H", "O"], units="metal", model_dtype="float64",
                         per_edge_type_cutoff={"H": 3.0})
    assert list(m.model.func._modules.keys()) == ["edge_norm", "pair_potential", "total_energy_sum"]
    assert m.model.func.pair_potential.atomic_numbers.dtype == torch.float64
    assert m.model._energy_seed_allowed()


def test_full_modifier_converts_a_reference_zbl():
    from nequip_amd.integrations.nequip_full import convert
    from nequip_amd.nn import ZBL
    from nequip_amd.nn.embedding import PolynomialCutoff

    class _Cutoff(torch.nn.Module):
        def __init__(self, p):
            super().__init__()
            self.p = float(p)

    def ref_zbl(z, q, p):
        # a module shaped like nequip.nn.pair_potential.ZBL: its buffers, cutoff, fields and irreps
        mod = type("ZBL", (torch.nn.Module,), {"__module__": "nequip.nn.pair_potential"})()
        mod.register_buffer("atomic_numbers", torch.tensor(z, dtype=torch.float32))
        mod.register_buffer("_qqr2exesquare", torch.tensor(q, dtype=torch.float64))
        mod.cutoff = _Cutoff(p)
        mod.per_atom_energy_field = "atomic_energy"
        mod.irreps_in = {"normed_edge_lengths": "1x0e", "atomic_energy": "1x0e"}
        return mod

    holder = torch.nn.Sequential()
    holder.add_module("pair_potential", ref_zbl([8.0, 1.0], 0.5 * 14.399645, 7))
    holder.add_module("scaled", ref_zbl([29.0], 0.5 * 14.399645 * 1.25, 6))  # a rescaled prefactor survives
    keys = {k: v.clone() for k, v in holder.state_dict().items()}
    out = convert(holder)
    assert isinstance(out.pair_potential, ZBL) and isinstance(out.scaled, ZBL)
    assert isinstance(out.pair_potential.cutoff, PolynomialCutoff) and out.pair_potential.cutoff.p == 7.0
    sd = out.state_dict()
    assert list(sd.keys()) == list(keys.keys())
    for k, v in keys.items():
        assert sd[k].dtype == v.dtype and torch.equal(sd[k], v), k


def test_zbl_kernels_compile_without_spills():
    import kernel_resources as kr

    objs = glob.glob(os.path.join(kr.BUILD, "pair_potential.o"))
    if not objs or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("build objects / ROCm LLVM tools not present (run python -m nequip_amd.csrc.build)")
    ks = {n: r for n, r in kr.kernels_of(objs[0]).items() if "zbl_kernel" in n}
    assert len(ks) == 3, list(ks)
    for name, r in ks.items():  # 79 / 107 / 120 VGPRs
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["lds"] == 0, (name, r)
        assert kr.waves_per_simd(r["vgpr"]) >= 4, (name, r)
