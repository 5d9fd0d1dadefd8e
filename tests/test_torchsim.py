"""torch-sim calculator (``nequip_amd.integrations.torchsim.NequIPTorchSimCalc``) and the batched neighbour list's C ABI.

CPU: the module imports without ``torch_sim`` and validates its arguments; the batched entry points are exported and
declared; their kernels compile for gfx950 without spills.  GPU: ``forward`` on a state of three systems (one of them not
periodic) matches three single-frame evaluations of the same eager model; the reference's input errors; a short
velocity-Verlet run through the calculator."""

import glob
import os
import sys
from dataclasses import dataclass
from typing import Optional

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
BATCHED_SYMBOLS = ("nqa_neighbor_list_batched_workspace_bytes", "nqa_neighbor_list_batched_count",
                   "nqa_neighbor_list_batched_fill")


@dataclass
class SimState:
    """Stand-in for ``torch_sim.SimState`` with the fields the calculator reads."""
    positions: torch.Tensor
    row_vector_cell: torch.Tensor
    pbc: object
    atomic_numbers: Optional[torch.Tensor] = None
    system_idx: Optional[torch.Tensor] = None


def test_module_imports_without_torch_sim_and_validates_arguments():
    from nequip_amd.integrations import torchsim as ts

    assert ts.HAVE_TORCH_SIM is False or ts.HAVE_TORCH_SIM is True
    with pytest.raises(TypeError):
        ts.NequIPTorchSimCalc(object(), device="cuda")
    with pytest.raises(RuntimeError):
        ts.NequIPTorchSimCalc(torch.nn.Linear(1, 1), device="cpu")
    with pytest.raises(NotImplementedError):
        ts.NequIPTorchSimCalc.from_compiled_model("model.nequip.pt2", device="cuda")
    with pytest.raises(ValueError):  # no cutoff
        ts.NequIPTorchSimCalc(torch.nn.Linear(1, 1), device="cuda")
    with pytest.raises(ValueError):  # no species mapping
        ts.NequIPTorchSimCalc(torch.nn.Linear(1, 1), device="cuda", r_max=4.0)


def test_batched_symbols_are_exported_and_declared():
    from nequip_amd import _lib

    header = open(os.path.join(ROOT, "include", "nequip_amd.h")).read()
    for name in BATCHED_SYMBOLS:
        assert name in _lib.SIGNATURES, name
        assert f" {name}(" in header, name
    lib_path = getattr(_lib, "LIB_PATH", None) or os.path.join(ROOT, "nequip_amd", "csrc", "libnequip_amd.so")
    if not os.path.exists(lib_path):
        pytest.skip("libnequip_amd.so not built")
    lib = _lib.load()
    for name in BATCHED_SYMBOLS:
        assert hasattr(lib, name), name
    assert lib.nqa_neighbor_list_batched_workspace_bytes(100, 0) == -1
    assert lib.nqa_neighbor_list_batched_workspace_bytes(100, 4) > lib.nqa_neighbor_list_workspace_bytes(100)


def test_batched_kernels_compile_without_spills():
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as kr

    objs = glob.glob(os.path.join(kr.BUILD, "neighbor_list.o"))
    if not objs or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("build objects / ROCm LLVM tools not present (run python -m nequip_amd.csrc.build)")
    ks = {n: r for n, r in kr.kernels_of(objs[0]).items() if "nl_batched_" in n}
    assert len(ks) == 4, list(ks)
    for name, r in ks.items():
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert kr.waves_per_simd(r["vgpr"]) >= 4, (name, r)


# ---- GPU -------------------------------------------------------------------------------------------------------------

Z_OF = {"H": 1, "O": 8}


def _model(device, names):
    from nequip_amd.model import NequIPGNNModel

    return NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.5, type_names=names, num_layers=2, l_max=1,
                          parity=False, num_features=8, radial_mlp_width=64, radial_mlp_depth=1,
                          avg_num_neighbors=20.0).to(device).eval()


def _systems():
    """Three water systems: two periodic boxes and one cluster in a box that is not periodic."""
    from nequip_amd.utils import synthetic as syn

    out = []
    for seed, n_side, periodic in ((0, 2, True), (1, 3, True), (2, 2, False)):
        pos, types, cell, names = syn.water_box(n_side, seed=seed)
        if not periodic:
            cell = cell * 3.0  # a box well beyond the cutoff around the cluster
        out.append((pos, types, cell, periodic))
    return out, names


def _state(systems, names, device, pbc_rows=True):
    pos = torch.tensor(np.concatenate([s[0] for s in systems]), dtype=torch.float64, device=device)
    z = torch.tensor(np.concatenate([[Z_OF[names[t]] for t in s[1]] for s in systems]), dtype=torch.long, device=device)
    sidx = torch.repeat_interleave(torch.arange(len(systems)), torch.tensor([len(s[0]) for s in systems])).to(device)
    cell = torch.tensor(np.stack([s[2] for s in systems]), dtype=torch.float64, device=device)
    pbc = torch.tensor([[s[3]] * 3 for s in systems], device=device) if pbc_rows else True
    return SimState(positions=pos, row_vector_cell=cell, pbc=pbc, atomic_numbers=z, system_idx=sidx)


@pytest.mark.gpu
def test_forward_matches_single_frame_evaluations(device):
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.data._nl import compute_neighborlist_
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc

    systems, names = _systems()
    model = _model(device, names)
    calc = NequIPTorchSimCalc(model, device=device)
    state = _state(systems, names, device)
    res = calc(state)
    S, N = len(systems), state.positions.shape[0]
    assert res["energy"].shape == (S,) and res["forces"].shape == (N, 3) and res["stress"].shape == (S, 3, 3)
    off = 0
    for s, (pos, types, cell, periodic) in enumerate(systems):
        data = {K.POSITIONS_KEY: torch.tensor(pos, dtype=torch.float64, device=device),
                K.ATOM_TYPE_KEY: torch.tensor(types, dtype=torch.long, device=device),
                K.CELL_KEY: torch.tensor(cell, dtype=torch.float64, device=device).view(1, 3, 3),
                K.PBC_KEY: torch.tensor([[periodic] * 3], device=device)}
        out = model(compute_neighborlist_(data, 4.5))
        n = len(pos)
        torch.testing.assert_close(res["energy"][s], out[K.TOTAL_ENERGY_KEY].view(-1)[0].to(res["energy"].dtype),
                                   atol=1e-5, rtol=1e-5)
        torch.testing.assert_close(res["forces"][off:off + n], out[K.FORCE_KEY].to(res["forces"].dtype), atol=5e-5, rtol=5e-5)
        torch.testing.assert_close(res["stress"][s], out[K.STRESS_KEY].view(3, 3).to(res["stress"].dtype), atol=5e-5,
                                   rtol=5e-5)
        off += n
    calc.compute_stress = False
    calc.compute_forces = False
    res2 = calc(state)
    assert set(res2) == {"energy"}
    torch.testing.assert_close(res2["energy"], res["energy"])


@pytest.mark.gpu
def test_input_errors_as_in_the_reference(device):
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc

    systems, names = _systems()
    model = _model(device, names)
    state = _state(systems, names, device)
    with_numbers = NequIPTorchSimCalc(model, device=device, atomic_numbers=state.atomic_numbers,
                                      system_idx=state.system_idx)
    with pytest.raises(ValueError, match="both"):
        with_numbers(state)
    no_numbers = SimState(state.positions, state.row_vector_cell, state.pbc, None, state.system_idx)
    assert with_numbers(no_numbers)["energy"].shape == (len(systems),)
    with pytest.raises(ValueError, match="either"):
        NequIPTorchSimCalc(model, device=device)(no_numbers)
    carbon = state.atomic_numbers.clone()
    carbon[5] = 6
    bad = SimState(state.positions, state.row_vector_cell, state.pbc, carbon, state.system_idx)
    with pytest.raises(ValueError, match="not among the model's types"):
        NequIPTorchSimCalc(model, device=device)(bad)


@pytest.mark.gpu
def test_short_velocity_verlet_run(device):
    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc

    systems, names = _systems()
    systems = [s[:3] + (True,) for s in systems]
    model = _model(device, names)
    calc = NequIPTorchSimCalc(model, device=device)
    state = _state(systems, names, device, pbc_rows=False)  # one periodicity for the state, as torch-sim passes it
    mass = torch.where(state.atomic_numbers == 1, 1.008, 15.999).to(torch.float64).unsqueeze(-1)
    vel = torch.zeros_like(state.positions)
    dt = 0.5e-3 * 10.18  # 0.5 fs in eV-Angstrom-amu time units
    res = calc(state)
    for _ in range(5):
        vel = vel + 0.5 * dt * res["forces"].to(torch.float64) / mass
        state.positions = state.positions + dt * vel
        res = calc(state)
        vel = vel + 0.5 * dt * res["forces"].to(torch.float64) / mass
    for k in ("energy", "forces", "stress"):
        assert torch.isfinite(res[k]).all(), k
    assert torch.isfinite(state.positions).all()
