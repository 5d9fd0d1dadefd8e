"""ZBL pair term on the MI355X: the kernels against the ATen restatement (`tests/zbl_restatement.py`, itself anchored to
LAMMPS and to the reference's module in test_zbl.py) and against the reference fixture; derivatives to second order;
determinism; the term inside whole models (eval, train, seed switch, Morton order, graphed MD step, LAMMPS local / ghost
evaluation, traced ops, the C++-registered ops)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import zbl_restatement as zr  # noqa: E402
from test_zbl import CASES, SPECIES, Z, _golden, restated_case  # noqa: E402

pytestmark = pytest.mark.gpu


def _zbl_module(dtype, species=SPECIES, p=6, units="metal"):
    from nequip_amd.model.nequip_models import torch_default_dtype
    from nequip_amd.nn import ZBL

    with torch_default_dtype(dtype):
        return ZBL(type_names=list(species), chemical_species=list(species), units=units, polynomial_cutoff_p=p,
                   irreps_in={"normed_edge_lengths": "1x0e"})


def _fixture_data(g, device, per: bool, dtype):
    """The fixture graph as the native chain sees it after EdgeLengthNormalizer (edge vectors as a float64 leaf)."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.model.nequip_models import torch_default_dtype
    from nequip_amd.nn.embedding import EdgeLengthNormalizer

    with torch_default_dtype(dtype):
        per_cut = {"H": 2.0, "C": {"O": 2.5, "Cu": 2.2}, "Au": 2.8} if per else None
        norm = EdgeLengthNormalizer(r_max=float(g["r_max"]), type_names=SPECIES, per_edge_type_cutoff=per_cut).to(device)
    vec = torch.tensor(g["pos"][g["edge_index"][1]] - g["pos"][g["edge_index"][0]] + g["edge_cell_shift"] @ g["cell"],
                       device=device).requires_grad_(True)
    data = {K.EDGE_VECTORS_KEY: vec, K.EDGE_INDEX_KEY: torch.tensor(g["edge_index"], device=device),
            K.ATOM_TYPE_KEY: torch.tensor(g["atom_types"], device=device)}
    return norm(data), vec


@pytest.mark.parametrize("dtype,per,with_pe", CASES)
def test_kernels_match_reference_fixture_and_restatement(device, dtype, per, with_pe):
    from nequip_amd.data import AtomicDataDict as K

    g = _golden()
    key = f"{dtype}_{'per' if per else 'plain'}_{'pe' if with_pe else 'nope'}"
    tdt = getattr(torch, dtype)
    data, vec = _fixture_data(g, device, per, tdt)
    if with_pe:
        data[K.PER_ATOM_ENERGY_KEY] = torch.tensor(g["pe_in"], device=device)
    pe = _zbl_module(tdt).to(device)(data)[K.PER_ATOM_ENERGY_KEY]
    (gv,) = torch.autograd.grad((pe * torch.tensor(g["weights"], device=device)).sum(), [vec])
    ref_pe, ref_gv = restated_case(g, dtype, per, with_pe, device=device)
    assert pe.dtype == torch.float64 and pe.shape == ref_pe.shape
    scale = float(ref_pe.abs().max())
    torch.testing.assert_close(pe, ref_pe, atol=1e-12 * scale, rtol=1e-12)
    gscale = float(ref_gv.abs().max())
    torch.testing.assert_close(gv, ref_gv, atol=1e-11 * gscale, rtol=1e-10)
    # against the fixture the reference computed on the CPU: in a float32 model its float32 roundings (the cutoff value, and
    # autograd's float32 gradient of it) land on the neighbouring float32 here and there when the float64 operands differ
    # in the last bit between CPU and GPU arithmetic -- the restatement evaluated on the GPU (above) agrees to 1e-10
    tol = 1e-7 if dtype == "float32" else 1e-12
    torch.testing.assert_close(pe.detach().cpu().numpy(), g[f"{key}_energy"], atol=tol * scale, rtol=tol)
    torch.testing.assert_close(gv.cpu().numpy(), g[f"{key}_g_edge_vec"], atol=max(tol, 1e-11) * gscale,
                               rtol=max(tol, 1e-10))
    # edges at or beyond their cutoff: exact zeros
    dead = torch.from_numpy(np.abs(g[f"{key}_g_edge_vec"]).sum(-1) == 0).to(device)
    assert int(dead.sum()) > 10 and bool((gv[dead] == 0).all())


def test_padding_edges_are_exact_zeros_and_evaluations_are_bitwise_repeatable(device):
    from nequip_amd.data import AtomicDataDict as K

    g = _golden()
    data, vec = _fixture_data(g, device, False, torch.float32)
    n = len(g["atom_types"])
    # padding edges as the padded list writes them: self edges of every atom, longer than r_max, appended
    far = torch.tensor([[3 * float(g["r_max"]), 0.0, 0.0]], dtype=torch.float64, device=device).expand(n, 3)
    pvec = torch.cat([vec.detach(), far]).requires_grad_(True)
    idx = torch.arange(n, device=device)
    padded = dict(data)
    padded[K.EDGE_VECTORS_KEY] = pvec
    padded[K.EDGE_INDEX_KEY] = torch.cat([data[K.EDGE_INDEX_KEY], torch.stack([idx, idx])], 1)
    m = _zbl_module(torch.float32).to(device)
    outs = []
    for _ in range(2):
        d = dict(padded)
        pe = m(d)[K.PER_ATOM_ENERGY_KEY]
        (gv,) = torch.autograd.grad(pe.sum(), [pvec], create_graph=True)
        (gg,) = torch.autograd.grad((gv * torch.ones_like(gv)).sum(), [pvec])
        outs.append((pe.detach(), gv.detach(), gg))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)
    E = vec.shape[0]
    pe, gv, gg = outs[0]
    assert bool(torch.isfinite(gv).all()) and bool((gv[E:] == 0).all()) and bool((gg[E:] == 0).all())
    ref = m(dict(data))[K.PER_ATOM_ENERGY_KEY].detach()
    torch.testing.assert_close(pe, ref, atol=0, rtol=1e-14)


def test_gradcheck_and_gradgradcheck(device):
    from nequip_amd.nn._pair_potential_ops import zbl

    torch.manual_seed(0)
    n = 6
    pos = torch.rand(n, 3, dtype=torch.float64, device=device) * 2.2
    ii, jj = torch.meshgrid(torch.arange(n), torch.arange(n), indexing="ij")
    keep = ii != jj
    ei = torch.stack([ii[keep], jj[keep]]).to(device)
    vec = (pos[ei[1]] - pos[ei[0]]).detach().requires_grad_(True)
    types = torch.tensor([0, 1, 2, 0, 1, 2], device=device)
    zt = torch.tensor([[1.0, 1.0], [8.0, 8.0 ** 0.23], [29.0, 29.0 ** 0.23]], dtype=torch.float64, device=device)
    qq = torch.tensor(0.5 * 14.399645, dtype=torch.float64, device=device)
    pe_in = torch.randn(n, 1, dtype=torch.float64, device=device, requires_grad=True)
    assert float((vec.norm(dim=-1) < 2.5).double().mean()) > 0.3

    def f(v, p):
        return zbl(v, p, ei, types, zt, qq, None, 1.0 / 2.5, 6.0, False)

    assert torch.autograd.gradcheck(f, (vec, pe_in), eps=1e-6, atol=1e-6, rtol=1e-5)
    assert torch.autograd.gradgradcheck(f, (vec, pe_in), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_two_atom_lammps_reproduction(device):
    """The reference's test_lammps_repro (float64 model, r_max 9, p 80) on every row with r < 8, all rows at once as frames
    of one batch, through the eval fast path and through the training path."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.model import ZBLPairPotential

    d = np.load(os.path.join(HERE, "golden", "zbl_lammps.npy"))
    d = d[d[:, 0] < 8.0]
    F = len(d)
    species = ["H", "O", "C", "N", "Cu", "Au"]
    tix = {Z[s]: i for i, s in enumerate(species)}
    model = ZBLPairPotential(seed=123, model_dtype="float64", r_max=9.0, polynomial_cutoff_p=80, type_names=species,
                             chemical_species=species, units="metal").to(device)
    pos = torch.zeros(2 * F, 3, dtype=torch.float64)
    pos[1::2, 0] = torch.tensor(d[:, 0])
    types = torch.tensor([[tix[int(a)], tix[int(b)]] for a, b in d[:, 1:3]]).view(-1)
    a = torch.arange(F) * 2
    ei = torch.stack([torch.stack([a, a + 1], 1).view(-1), torch.stack([a + 1, a], 1).view(-1)])
    for training in (False, True):
        model.train(training)
        data = {K.POSITIONS_KEY: pos.to(device), K.ATOM_TYPE_KEY: types.to(device), K.EDGE_INDEX_KEY: ei.to(device),
                K.BATCH_KEY: torch.arange(F).repeat_interleave(2).to(device),
                K.NUM_NODES_KEY: torch.full((F,), 2, dtype=torch.long, device=device)}
        out = model(data)
        e = out[K.TOTAL_ENERGY_KEY].detach().view(-1).cpu().numpy()
        f = out[K.FORCE_KEY].detach().cpu().numpy()
        np.testing.assert_allclose(e, d[:, 3], atol=1e-4)
        np.testing.assert_allclose(f[0::2, 0], d[:, 4], atol=1e-5)
        np.testing.assert_allclose(f[1::2, 0], d[:, 5], atol=1e-5)


# ---- whole models -----------------------------------------------------------------------------------------------------------
def _models(device, dtype="float32", **kw):
    from nequip_amd.model import NequIPGNNModel

    args = dict(seed=3, model_dtype=dtype, r_max=4.5, type_names=["H", "O"], num_layers=2, l_max=2, parity=False,
                num_features=16, radial_mlp_depth=1, radial_mlp_width=32, avg_num_neighbors=38.0,
                per_type_energy_scales={"H": 1.2, "O": 0.8}, per_type_energy_shifts={"H": -0.5, "O": 1.5})
    args.update(kw)
    cfg = {"_target_": "nequip.nn.pair_potential.ZBL", "chemical_species": ["H", "O"], "units": "metal"}
    with_zbl = NequIPGNNModel(pair_potential=cfg, **args).to(device)
    plain = NequIPGNNModel(**args).to(device)
    return with_zbl, plain


def _restated_terms(data, device, model_dtype=torch.float32):
    """Energy [1, 1], forces [N, 3], virial [1, 3, 3] of the ZBL term alone (ATen restatement, autograd)."""
    from nequip_amd.data import AtomicDataDict as K

    pos = data[K.POSITIONS_KEY].to(device).detach().requires_grad_(True)
    eps = torch.zeros(3, 3, dtype=torch.float64, device=device, requires_grad=True)
    sym = 0.5 * (eps + eps.t())
    cell = data[K.CELL_KEY].to(device).view(3, 3)
    ei = data[K.EDGE_INDEX_KEY].to(device)
    p2 = pos + pos @ sym
    vec = p2[ei[1]] - p2[ei[0]] + data[K.EDGE_CELL_SHIFT_KEY].to(device) @ (cell + cell @ sym)
    zt = torch.tensor([1.0, 8.0], dtype=torch.float64, device=device)
    types = data[K.ATOM_TYPE_KEY].to(device)
    e = zr.atom_energy(vec, ei, zt[types], 1.0 / 4.5, len(types), model_dtype=model_dtype).sum()
    gp, ge = torch.autograd.grad(e, [pos, eps])
    return e.detach(), -gp, -ge


@pytest.mark.parametrize("mode", ["eval", "train", "no_energy_seed", "spatial_order"])
def test_model_with_zbl_is_model_without_plus_the_term(device, mode, monkeypatch):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.nn._topology import topology_cache
    from nequip_amd.utils import synthetic as syn

    if mode == "no_energy_seed":
        monkeypatch.setenv("NQA_NO_ENERGY_SEED", "1")
    pos, types, cell, names = syn.water_box(n_side=3, seed=8)
    if mode == "spatial_order":  # atoms in a shuffled order, so that the Morton permutation is far from the identity
        monkeypatch.setenv("NQA_SPATIAL_ORDER", "1")
        monkeypatch.setenv("NQA_SPATIAL_ORDER_MIN", "1")
        shuffle = np.random.default_rng(0).permutation(len(pos))
        pos, types = np.asarray(pos)[shuffle], np.asarray(types)[shuffle]
    data = syn.make_data(pos, types, 4.5, cell)
    with_zbl, plain = _models(device)
    outs = []
    for m in (with_zbl, plain):
        m.train(mode == "train")
        topology_cache.clear()
        d = {k: v.clone().to(device) for k, v in data.items()}
        outs.append(m(d))
        if mode == "spatial_order":
            ei = d[K.EDGE_INDEX_KEY]
            sp = getattr(topology_cache.get(ei[0], ei[1], len(pos)), "_spatial", None)
            assert sp is not None and not torch.equal(sp.perm.cpu(), torch.arange(len(pos))), "Morton path not taken"
    e_z, f_z, w_z = _restated_terms(data, device)
    a, b = outs
    assert float(e_z) > 1.0
    torch.testing.assert_close(a[K.TOTAL_ENERGY_KEY].detach().view(-1), (b[K.TOTAL_ENERGY_KEY].detach() + e_z).view(-1),
                               atol=1e-4, rtol=1e-6)
    fscale = float(f_z.abs().max())
    torch.testing.assert_close(a[K.FORCE_KEY].detach(), b[K.FORCE_KEY].detach() + f_z, atol=2e-5 * fscale, rtol=1e-5)
    torch.testing.assert_close(a[K.VIRIAL_KEY].detach().view(3, 3), (b[K.VIRIAL_KEY].detach().view(3, 3) + w_z),
                               atol=1e-4 * float(w_z.abs().max()), rtol=1e-5)
    vol = float(np.abs(np.linalg.det(np.asarray(cell).reshape(3, 3))))
    torch.testing.assert_close(a[K.STRESS_KEY].detach().view(3, 3), b[K.STRESS_KEY].detach().view(3, 3) - w_z / vol,
                               atol=1e-4 * float(w_z.abs().max()) / vol, rtol=1e-5)


class _AtenZBL(torch.nn.Module):
    """The ATen restatement in the place of the native module (same inputs, same output field)."""

    def forward(self, data):
        from nequip_amd.data import AtomicDataDict as K

        vec, ei, types = data[K.EDGE_VECTORS_KEY], data[K.EDGE_INDEX_KEY], data[K.ATOM_TYPE_KEY].view(-1)
        zt = torch.tensor([1.0, 8.0], dtype=torch.float64, device=vec.device)
        e = zr.atom_energy(vec, ei, zt[types], float(data["_nqa_rmax_recip"]), len(types), model_dtype=torch.float32)
        data[K.PER_ATOM_ENERGY_KEY] = data[K.PER_ATOM_ENERGY_KEY] + e
        return data


def test_force_and_stress_matching_step_matches_aten_restatement(device):
    """Training differentiates the forces again: the second-order kernel runs in loss.backward()."""
    import copy

    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=3, seed=9)
    data = syn.make_data(pos, types, 4.5, cell)
    native, _ = _models(device)
    aten = copy.deepcopy(native)
    aten.model.func.pair_potential = _AtenZBL()
    torch.manual_seed(1)
    f_target = torch.randn(len(pos), 3, dtype=torch.float64, device=device)
    s_target = torch.randn(1, 3, 3, dtype=torch.float64, device=device) * 1e-2
    res = []
    for m in (native, aten):
        m.train()
        d = {k: v.to(device) for k, v in data.items()}
        d[K.POSITIONS_KEY].requires_grad_(True)
        out = m(d)
        loss = ((out[K.FORCE_KEY] - f_target) ** 2).mean() + ((out[K.STRESS_KEY] - s_target) ** 2).mean() * 10 \
            + 1e-3 * out[K.TOTAL_ENERGY_KEY].sum() ** 2
        (g_pos,) = torch.autograd.grad(loss, [d[K.POSITIONS_KEY]], retain_graph=True)
        m.zero_grad()
        loss.backward()
        res.append((loss.detach(), g_pos.detach(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    (l0, gp0, pg0), (l1, gp1, pg1) = res
    torch.testing.assert_close(l0, l1, atol=0, rtol=1e-6)
    torch.testing.assert_close(gp0, gp1, atol=1e-6 * float(gp1.abs().max()), rtol=1e-5)
    assert set(pg0) == set(pg1) and len(pg0) > 5
    for n in pg0:
        torch.testing.assert_close(pg0[n], pg1[n], atol=1e-5 * max(1e-3, float(pg1[n].abs().max())), rtol=1e-4, msg=n)


def test_graphed_step_on_padded_list_equals_eager(device):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data._nl import compute_neighborlist_
    from nequip_amd.integrations.graphed_step import GraphedStep
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=3, seed=2)
    model, _ = _models(device)
    model.eval()
    pos_t = torch.as_tensor(pos, dtype=torch.float64, device=device)
    types_t = torch.as_tensor(types, device=device)
    cell_t = torch.as_tensor(np.asarray(cell).reshape(3, 3), dtype=torch.float64, device=device)
    step = GraphedStep(model, types_t, cell_t, True, 4.5, headroom=1.1)
    for it in range(3):
        p = pos_t + 0.02 * it
        out = {k: v.clone() for k, v in step(p).items()}
        d = {K.POSITIONS_KEY: p, K.ATOM_TYPE_KEY: types_t, K.CELL_KEY: cell_t.view(1, 3, 3),
             K.PBC_KEY: torch.tensor([[True, True, True]], device=device)}
        ref = model(compute_neighborlist_(d, 4.5))
        torch.testing.assert_close(out[K.TOTAL_ENERGY_KEY], ref[K.TOTAL_ENERGY_KEY].detach(), atol=1e-4, rtol=1e-6)
        fscale = float(ref[K.FORCE_KEY].abs().max())
        torch.testing.assert_close(out[K.FORCE_KEY], ref[K.FORCE_KEY].detach(), atol=5e-6 * fscale, rtol=1e-5)
    assert step.num_captures >= 1 and step.num_eager_fallbacks == 0


def test_lammps_local_ghost_evaluation_matches_periodic(device):
    import copy

    import test_ghost_exchange as tge
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.nn import NoOpGhostExchangeModule, with_edge_vectors_
    from nequip_amd.utils import synthetic as syn

    pos, types, cell, names = syn.water_box(n_side=3, seed=8)
    data = syn.make_data(pos, types, 4.5, cell)
    n = len(pos)
    model, _ = _models(device)
    model.eval()
    edge_vec = with_edge_vectors_(dict(data))[K.EDGE_VECTORS_KEY]
    a = {K.EDGE_VECTORS_KEY: edge_vec.to(device).requires_grad_(True), K.EDGE_INDEX_KEY: data["edge_index"].to(device),
         K.ATOM_TYPE_KEY: data["atom_types"].to(device)}
    out_a = model(a)
    ei_l, types_l, owner = tge._ghost_representation(data)
    lmp = tge.FakeLammpsData(n, owner.to(device))
    model_l = NoOpGhostExchangeModule.enable_LAMMPSMLIAPGhostExchange(copy.deepcopy(model))
    b = {K.EDGE_VECTORS_KEY: edge_vec.to(device).requires_grad_(True), K.EDGE_INDEX_KEY: ei_l.to(device),
         K.ATOM_TYPE_KEY: types_l.to(device), K.LMP_MLIAP_DATA_KEY: lmp,
         K.NUM_LOCAL_GHOST_NODES_KEY: torch.tensor([n, owner.numel()], device=device)}
    out_b = model_l(b)
    e_a, e_b = out_a[K.PER_ATOM_ENERGY_KEY].detach(), out_b[K.PER_ATOM_ENERGY_KEY].detach()
    assert e_b.shape[0] == n
    torch.testing.assert_close(e_b, e_a, atol=2e-5, rtol=1e-5)
    f_a, f_b = out_a[K.EDGE_FORCE_KEY].detach(), out_b[K.EDGE_FORCE_KEY].detach()
    torch.testing.assert_close(f_b, f_a, atol=2e-5 * max(1.0, float(f_a.abs().max())), rtol=1e-5)
    # the periodic evaluation's forces, folded from the edge forces
    ref = model({k: v.to(device) for k, v in data.items()})
    f_atoms = tge._edge_forces_to_atoms(f_b, data["edge_index"], n)
    fscale = float(ref[K.FORCE_KEY].abs().max())
    torch.testing.assert_close(f_atoms.to(device).to(torch.float64), ref[K.FORCE_KEY].detach(), atol=5e-5 * fscale,
                               rtol=1e-5)


def test_traced_ops_equal_eager(device):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.utils import synthetic as syn
    from nequip_amd.utils.tracing import traceable_forms

    pos, types, cell, names = syn.water_box(n_side=3, seed=4)
    data = syn.make_data(pos, types, 4.5, cell)
    model, _ = _models(device)
    model.eval()
    ref = model({k: v.to(device) for k, v in data.items()})
    with traceable_forms():
        out = model({k: v.to(device) for k, v in data.items()})
    torch.testing.assert_close(out[K.TOTAL_ENERGY_KEY].detach(), ref[K.TOTAL_ENERGY_KEY].detach(), atol=1e-4, rtol=1e-6)
    fscale = float(ref[K.FORCE_KEY].abs().max())
    torch.testing.assert_close(out[K.FORCE_KEY], ref[K.FORCE_KEY], atol=2e-5 * fscale, rtol=1e-5)


_OP_REPLAY = """
import sys, torch
torch.ops.load_library(sys.argv[1])
assert "nequip_amd" not in sys.modules
rec = torch.load(sys.argv[2])
bad = []
for name, args, ref in rec:
    out = getattr(torch.ops.nequip_amd, name)(*[a.cuda() if isinstance(a, torch.Tensor) else a for a in args])
    if out.shape != ref.shape or out.dtype != ref.dtype or not torch.equal(out.cpu(), ref):
        bad.append((name, tuple(out.shape), tuple(ref.shape)))
print("BAD", bad)
sys.exit(1 if bad else 0)
"""


def test_cpp_registered_ops_reproduce_python_ops_bitwise(device, tmp_path):
    import nequip_amd  # noqa: F401

    lib = os.path.join(ROOT, "nequip_amd", "csrc", "libnequip_amd_torch.so")
    if not os.path.exists(lib):
        from nequip_amd.csrc import build as _build

        _build.build_torch_ops(force=False, verbose=False)
    g = _golden()
    ops = torch.ops.nequip_amd
    rec = []
    for dtype, per in ((torch.float32, False), (torch.float64, True)):
        data, vec = _fixture_data(g, device, per, dtype)
        m = _zbl_module(dtype).to(device)
        ei, types = data["edge_index"], data["atom_types"]
        rme = data.get("_nqa_rmax_recip_edge")
        cfg = (float(data["_nqa_rmax_recip"]), 6.0, dtype == torch.float32)
        zt = m._z_table()
        pe_in = torch.tensor(g["pe_in"], device=device)
        for pe in (None, pe_in):
            args = (vec.detach(), pe, ei, types, zt, m._qqr2exesquare, rme) + cfg
            rec.append(("zbl_fwd", [a.cpu() if isinstance(a, torch.Tensor) else a for a in args], ops.zbl_fwd(*args).cpu()))
        gp = torch.rand(len(types), 1, dtype=torch.float64, device=device)
        args = (gp, vec.detach(), ei, types, zt, m._qqr2exesquare, rme) + cfg
        rec.append(("zbl_bwd", [a.cpu() if isinstance(a, torch.Tensor) else a for a in args], ops.zbl_bwd(*args).cpu()))
    path = tmp_path / "zbl_ops.pt"
    torch.save(rec, path)
    r = subprocess.run([sys.executable, "-c", _OP_REPLAY, lib, str(path)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, PYTHONPATH=""), cwd="/tmp")
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
