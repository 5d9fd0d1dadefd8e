"""``DataStatisticsManager`` on the CPU: the interface of ``nequip/data/stats_manager.py`` and the ATen form of the fused
reduction (``nequip_amd/data/_stats_ops.py::_aten_update``) against ``tests/stats_restatement.py``.

The reference (nequip/data/stats.py, stats_manager.py) cannot be imported here -- it needs ``torchmetrics``, which is not
installed -- so there are no reference-generated fixtures for this feature.

Tolerance against the restatement: rtol 1e-10, atol 0, NaN equal to NaN.  Both sides are float64 reductions of fewer than 1e5
well-conditioned terms in different orders, which differ by at most about n * 2^-53.
"""
import math
import os
import re
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import stats_cases as sc
import stats_restatement as sr
from nequip_amd.data import (CommonDataStatisticsManager, Count, DataStatisticsManager, EdgeLengths,
                             EnergyOnlyDataStatisticsManager, Max, Mean, MeanAbsolute, Min, NumNeighbors, PerAtomModifier,
                             RootMeanSquare, StandardDeviation, _stats_ops)

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TYPES = sc.TYPES
F32, F64 = torch.float32, torch.float64


# ---- interface ---------------------------------------------------------------------------------------------------------------
def test_metric_strings_are_the_references():
    got = [str(m) for m in (Mean(), MeanAbsolute(), RootMeanSquare(), StandardDeviation(), StandardDeviation(squared=True),
                            Max(), Max(abs=True), Min(), Min(abs=True), Count())]
    assert got == ["mean", "mean_abs", "rms", "std", "var", "max", "absmax", "min", "absmin", "count"]
    assert str(NumNeighbors()) == "num_neighbors" and NumNeighbors().type == "node"
    assert str(EdgeLengths()) == "edge_lengths" and EdgeLengths().type == "edge"


def test_default_and_custom_names():
    m = DataStatisticsManager([
        {"field": "forces", "metric": RootMeanSquare()},
        {"field": "total_energy", "metric": StandardDeviation(squared=True)},
        {"field": PerAtomModifier("total_energy"), "metric": Mean()},
        {"field": NumNeighbors(), "metric": Max()},
        {"field": EdgeLengths(), "metric": Min(abs=True)},
        {"field": "forces", "metric": Mean(), "name": "mine", "per_type": True}], type_names=TYPES)
    assert m.names == ["F_rms", "E_var", "per_atom_E_mean", "num_neighbors_max", "edge_lengths_absmin", "mine"]
    assert m.per_type == [False] * 5 + [True] and m.ignore_nans == [False] * 6


def test_the_references_assertions():
    entry = {"field": "forces", "metric": Mean()}
    with pytest.raises(AssertionError):
        DataStatisticsManager([])
    with pytest.raises(AssertionError, match="Repeated names"):
        DataStatisticsManager([dict(entry), dict(entry)])
    with pytest.raises(AssertionError, match="type_names"):
        DataStatisticsManager([dict(entry, per_type=True)])
    with pytest.raises(AssertionError, match="only apply to node or edge fields"):
        DataStatisticsManager([{"field": "total_energy", "metric": Mean(), "per_type": True}], type_names=TYPES)
    with pytest.raises(AssertionError, match="only apply to node or edge fields"):
        DataStatisticsManager([{"field": PerAtomModifier("total_energy"), "metric": Mean(), "per_type": True}],
                              type_names=TYPES)
    for key in ("dataset", "generator", "collate_fn"):
        with pytest.raises(AssertionError):
            DataStatisticsManager([dict(entry)], dataloader_kwargs={key: None})
    with pytest.raises(AssertionError):
        DataStatisticsManager([dict(entry, ignore_nan=1)])
    m = DataStatisticsManager([dict(entry)], dataloader_kwargs={"batch_size": 7})
    assert m.dataloader_kwargs == {"batch_size": 7}
    with pytest.raises(TypeError, match="nequip_amd.data"):
        DataStatisticsManager([{"field": "forces", "metric": torch.nn.Identity()}])


def test_builders_have_the_references_entries():
    c = CommonDataStatisticsManager(type_names=TYPES, dataloader_kwargs={"batch_size": 5})
    assert c.names == ["num_neighbors_mean", "per_type_num_neighbors_mean", "per_atom_energy_mean", "forces_rms",
                       "per_type_forces_rms"]
    assert [str(f) for f in c.fields] == ["num_neighbors", "num_neighbors", "per_atom_E", "F", "F"]
    assert [str(x) for x in c.metrics] == ["mean", "mean", "mean", "rms", "rms"]
    assert c.per_type == [False, True, False, False, True] and c.dataloader_kwargs == {"batch_size": 5}
    e = EnergyOnlyDataStatisticsManager(type_names=TYPES)
    assert e.names == ["num_neighbors_mean", "per_type_num_neighbors_mean", "per_atom_energy_mean", "per_atom_energy_std",
                       "total_energy_std"]
    assert [str(f) for f in e.fields] == ["num_neighbors", "num_neighbors", "per_atom_E", "per_atom_E", "E"]
    assert [str(x) for x in e.metrics] == ["mean", "mean", "mean", "std", "std"]
    assert e.per_type == [False, True, False, False, False]
    # entries on one field share one read: three streams each
    assert len(c._stream_fields) == 3 and len(e._stream_fields) == 3


def test_running_state_is_in_no_state_dict():
    m = CommonDataStatisticsManager(type_names=TYPES)
    m(sc.make_batch([3, 4], 0))
    assert len(m.state_dict()) == 0 and not list(m.parameters()) and not list(m.buffers())


def test_caps_raise_value_errors_that_name_the_cap():
    from nequip_amd import _lib

    many = [f"T{i}" for i in range(_lib.NQA_STATS_MAX_NODE_TYPES + 1)]
    with pytest.raises(ValueError, match="NQA_STATS_MAX_NODE_TYPES"):
        DataStatisticsManager([{"field": "forces", "metric": Mean(), "per_type": True}], type_names=many)
    with pytest.raises(ValueError, match="NQA_STATS_MAX_EDGE_TYPES"):
        DataStatisticsManager([{"field": EdgeLengths(), "metric": Mean(), "per_type": True}],
                              type_names=many[:_lib.NQA_STATS_MAX_EDGE_TYPES + 1])
    with pytest.raises(ValueError, match="NQA_STATS_MAX_TERMS"):
        DataStatisticsManager([{"field": "forces", "metric": Mean(), "name": str(i)}
                               for i in range(_lib.NQA_STATS_MAX_TERMS + 1)])
    with pytest.raises(ValueError, match="NQA_STATS_MAX_STREAMS"):
        DataStatisticsManager([{"field": PerAtomModifier("total_energy", factor=float(i)), "metric": Mean(), "name": str(i)}
                               for i in range(_lib.NQA_STATS_MAX_STREAMS + 1)])
    with pytest.raises(ValueError, match="NQA_STATS_MAX_SLOTS"):
        DataStatisticsManager([{"field": EdgeLengths(), "metric": m, "per_type": True, "name": str(i)}
                               for i, m in enumerate([Mean(), Max(), Min(), Count(), RootMeanSquare()])],
                              type_names=many[:_lib.NQA_STATS_MAX_EDGE_TYPES])


# ---- the ATen form against the restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("fields", [("forces",), ("total_energy", "per_atom:total_energy"), ("edge_lengths",),
                                    ("num_neighbors",)])
def test_every_metric_against_the_restatement(fields, dtype):
    """Every metric class, plain and (node / edge fields) per type, over three batches of unequal sizes and an empty one; ``O``
    is absent from one batch, ``Cs`` from all (the reference's 0 / 0 = NaN for the means and the biased deviation, 0 / -1 = -0
    for the unbiased one, -inf / +inf for ``max`` / ``min``, 0 for ``count``; no exception).  T = 3: nine type pairs for the
    edge lengths."""
    entries = sc.entries_for(fields, per_type=fields[0] not in ("total_energy",))
    batches = sc.three_batches(dtype)
    m = DataStatisticsManager(sc.to_dicts(entries), type_names=TYPES)
    got = m.get_statistics([dict(b) for b in batches])
    ref = sr.evaluate(entries, batches, TYPES)
    sc.assert_stats_close(got, ref)
    if fields[0] in ("forces", "num_neighbors"):
        mean, extreme = ref[f"{fields[0]}|mean|pt|keep"], ref[f"{fields[0]}|max|pt|keep"]
        assert math.isnan(mean["Cs"]) and not math.isnan(mean["O"]) and extreme["Cs"] == -math.inf
        assert ref[f"{fields[0]}|count|pt|keep"]["Cs"] == 0.0 and math.isnan(ref[f"{fields[0]}|std_biased|pt|keep_Cs"])
    if fields[0] == "edge_lengths":
        assert math.isnan(ref["edge_lengths|mean|pt|keep"]["Cs_H"]) and ref["edge_lengths|count|pt|keep"]["H_Cs"] == 0.0
        assert len(ref["edge_lengths|mean|pt|keep"]) == 9 and "edge_lengths|mean|pt|keep_HO" in ref
        assert ref["edge_lengths|mean|pt|keep"]["H_O"] != ref["edge_lengths|mean|pt|keep"]["O_H"]  # (an asymmetric list)


@pytest.mark.parametrize("dtype", [F32, F64])
def test_nan_elements_are_dropped_or_propagate(dtype):
    """A quarter of the elements NaN: with ``ignore_nan`` they are dropped (and not counted), without it every value of the
    groups that hold one is NaN -- ``max`` and ``min`` too."""
    entries = sc.entries_for(("fnan",), kinds=["mean", "rms", "std", "max", "absmin", "count"], ignore_nan=(False, True))
    batches = sc.three_batches(dtype)
    got = DataStatisticsManager(sc.to_dicts(entries), type_names=TYPES).get_statistics([dict(b) for b in batches])
    ref = sr.evaluate(entries, batches, TYPES)
    sc.assert_stats_close(got, ref)
    for kind in ("mean", "rms", "std", "max", "absmin"):
        assert math.isnan(got[f"fnan|{kind}|all|keep"]) and math.isnan(got[f"fnan|{kind}|pt|keep"]["H"])
        assert math.isfinite(got[f"fnan|{kind}|all|drop"]) and math.isfinite(got[f"fnan|{kind}|pt|drop"]["H"])
    n_all = sum(b["fnan"].numel() for b in batches)
    n_nan = sum(int(torch.isnan(b["fnan"]).sum()) for b in batches)
    assert got["fnan|count|all|keep"] == n_all and got["fnan|count|all|drop"] == n_all - n_nan and n_nan > 0


def test_reset_and_a_second_pass():
    entries = sc.entries_for(("forces",), kinds=["mean", "std", "max"])
    batches = sc.three_batches()
    m = DataStatisticsManager(sc.to_dicts(entries), type_names=TYPES)
    first = dict(m.get_statistics(batches))
    m.reset()
    assert math.isnan(m.compute()["forces|mean|all|keep"]) and m.compute()["forces|max|all|keep"] == -math.inf
    sc.assert_stats_close(m.get_statistics(batches), first, rtol=0.0)


# ---- NumNeighbors ------------------------------------------------------------------------------------------------------------
def test_num_neighbors_with_an_isolated_atom_in_the_middle():
    """Atom 1 of 5 has no edge.  True counts [2, 0, 1, 3, 1]; the reference would pad the compacted counts to [2, 1, 3, 1, 0]
    and report H: 1.5, O: 4/3.  Here H (atoms 0, 1): 1.0, O (atoms 2, 3, 4): 5/3; the mean over all atoms is E / N."""
    data = {"pos": torch.zeros(5, 3, dtype=F64), "atom_types": torch.tensor([0, 0, 1, 1, 1]),
            "edge_index": torch.tensor([[3, 0, 4, 3, 2, 0, 3], [0, 3, 3, 4, 3, 2, 2]])}  # (unsorted)
    assert NumNeighbors()(data).tolist() == [2, 0, 1, 3, 1]
    m = DataStatisticsManager([{"field": NumNeighbors(), "metric": Mean(), "name": "nn"},
                               {"field": NumNeighbors(), "metric": Mean(), "name": "nn_pt", "per_type": True},
                               {"field": NumNeighbors(), "metric": Max(), "name": "nn_max", "per_type": True}],
                              type_names=["H", "O"])
    got = m.get_statistics([data])
    assert got["nn"] == pytest.approx(7 / 5, rel=1e-14)
    assert got["nn_pt"] == pytest.approx({"H": 1.0, "O": 5 / 3}, rel=1e-14) and got["nn_pt_H"] == got["nn_pt"]["H"]
    assert got["nn_max"] == {"H": 2.0, "O": 3.0}
    ref = sr.evaluate([{"name": "nn", "field": "num_neighbors", "kind": "mean"},
                       {"name": "nn_pt", "field": "num_neighbors", "kind": "mean", "per_type": True},
                       {"name": "nn_max", "field": "num_neighbors", "kind": "max", "per_type": True}], [data], ["H", "O"])
    sc.assert_stats_close(got, ref)


# ---- cancellation ------------------------------------------------------------------------------------------------------------
def test_variance_does_not_cancel():
    """Measured (CPU, ATen form): std e_ref = 3.6e-10, e_new = 0.0; mean e_ref = 1.2e-16, e_new = 0.0.  The restatement -- the
    reference's algorithm -- loses digits in ``delta = batch_mean - mean`` of Chan's merge (both means carry 1e-10 at 1e6);
    the two-word mean here does not.  A sum-of-squares implementation would miss by order 1."""
    for name, (e_ref, e_new) in sc.cancellation_errors(lambda b: b).items():
        assert e_new <= 10 * e_ref + 1e-12, (name, e_ref, e_new)


# ---- torch.distributed -------------------------------------------------------------------------------------------------------
DDP_ENTRIES = (sc.entries_for(("forces",), kinds=["mean", "std", "var", "max", "min", "rms", "count"])
               + sc.entries_for(("total_energy", "per_atom:total_energy"), per_type=False, kinds=["std", "mean", "max", "min"])
               + sc.entries_for(("num_neighbors",), kinds=["mean", "std"]))


def _ddp_batches(rank):
    """Half of the batches each; ``O`` occurs on rank 1 only."""
    if rank == 0:
        return [sc.make_batch([3, 5], 10, type_choices=(0,)), sc.make_batch([4], 11, type_choices=(0,))]
    return [sc.make_batch([2, 6, 1], 12), sc.make_batch([7, 2], 13)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    m = DataStatisticsManager(sc.to_dicts(DDP_ENTRIES), type_names=TYPES)
    got = m.get_statistics(_ddp_batches(rank))
    torch.save(got, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_compute_merges_the_ranks_gloo(tmp_path):
    """Two ranks see half of the batches each; ``compute()`` on both equals a single process over all of them -- the standard
    deviations included, which a sum of the ranks' M2 would get wrong."""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    single = DataStatisticsManager(sc.to_dicts(DDP_ENTRIES), type_names=TYPES).get_statistics(_ddp_batches(0) + _ddp_batches(1))
    ref = sr.evaluate(DDP_ENTRIES, _ddp_batches(0) + _ddp_batches(1), TYPES)
    sc.assert_stats_close(single, ref)
    for rank in range(world):
        got = torch.load(os.path.join(str(tmp_path), f"rank{rank}.pt"))
        sc.assert_stats_close(got, single)
    assert not math.isnan(single["forces|std|pt|keep"]["O"])  # a type only one rank has seen


# ---- into the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per_type_neighbors", [False, True])
def test_statistics_feed_the_model_builder(per_type_neighbors):
    from nequip_amd.model import NequIPGNNModel

    names = ["H", "O"]
    batches = [sc.make_batch([6, 5], 20), sc.make_batch([9], 21)]
    stats = CommonDataStatisticsManager(type_names=names).get_statistics(batches)
    ann = stats["per_type_num_neighbors_mean"] if per_type_neighbors else stats["num_neighbors_mean"]
    assert set(stats["per_type_forces_rms"]) == set(stats["per_type_num_neighbors_mean"]) == set(names)
    model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=4.0, type_names=names, num_layers=2, l_max=1, parity=False,
                           num_features=8, radial_mlp_depth=1, radial_mlp_width=16, avg_num_neighbors=ann,
                           per_type_energy_shifts=stats["per_atom_energy_mean"],
                           per_type_energy_scales=stats["per_type_forces_rms"])
    assert sum(p.numel() for p in model.parameters()) > 0
    edges, atoms = sum(b["edge_index"].shape[1] for b in batches), sum(len(b["pos"]) for b in batches)
    assert stats["num_neighbors_mean"] == pytest.approx(edges / atoms, rel=1e-14)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_constants_structs_and_symbols_agree_with_the_header_and_the_library():
    import ctypes

    from nequip_amd import _lib

    header = open(os.path.join(ROOT, "include", "nequip_amd.h")).read()
    defined = {k: int(v) for k, v in re.findall(r"#define\s+(NQA_STATS_[A-Z_]+)\s+(\d+)", header)}
    assert set(defined) == {"NQA_STATS_MAX_STREAMS", "NQA_STATS_MAX_TERMS", "NQA_STATS_MAX_NODE_TYPES",
                            "NQA_STATS_MAX_EDGE_TYPES", "NQA_STATS_MAX_SLOTS", "NQA_STATS_GROUPS"}
    assert defined == {k: getattr(_lib, k) for k in defined}
    for enum in ("F32", "F64", "I32", "I64", "MOD_IDENTITY", "MOD_ABS", "MOD_SQUARE", "GROUP_NONE", "GROUP_NODE", "GROUP_EDGE"):
        (value,) = re.findall(rf"NQA_STATS_{enum} = (\d+)", header)
        assert int(value) == getattr(_lib, f"NQA_STATS_{enum}")
    declared = set(re.findall(r"\b(nqa_stats_[a-z_]+)\(", header))
    assert declared == {"nqa_stats_groups", "nqa_stats_workspace_bytes", "nqa_stats_update", "nqa_stats_neighbor_counts"}
    assert declared <= set(_lib.SIGNATURES)
    assert ctypes.sizeof(_lib.StatsStream) == 64 and ctypes.sizeof(_lib.StatsTerm) == 32
    lib = _lib.load()  # (every listed symbol is resolved here)
    assert _stats_ops.NUM_WORKGROUPS == _lib.NQA_STATS_GROUPS == lib.nqa_stats_groups()
    assert lib.nqa_stats_workspace_bytes(3) == _lib.NQA_STATS_GROUPS * 3 * 48
    assert lib.nqa_stats_workspace_bytes(_lib.NQA_STATS_MAX_SLOTS + 1) == -1


def test_invalid_arguments_are_refused_before_any_launch():
    """``NQA_ERR_INVALID`` with a message, without a GPU: the checks come before the first launch."""
    from nequip_amd import _lib

    lib = _lib.load()
    streams, terms = (_lib.StatsStream * 1)(), (_lib.StatsTerm * 1)()
    streams[0].rows, streams[0].cols, streams[0].dtype = 0, 1, _lib.NQA_STATS_F64
    terms[0].n_groups = 1
    assert lib.nqa_stats_update(streams, 0, terms, 1, None, 0, None, None) == -1
    assert b"streams" in lib.nqa_last_error()
    assert lib.nqa_stats_update(streams, 1, terms, _lib.NQA_STATS_MAX_TERMS + 1, None, 0, None, None) == -1
    terms[0].mod = 7
    assert lib.nqa_stats_update(streams, 1, terms, 1, None, 0, None, None) == -1
    assert b"modifier" in lib.nqa_last_error()
    terms[0].mod, terms[0].n_groups = 0, 3
    assert lib.nqa_stats_update(streams, 1, terms, 1, None, 0, None, None) == -1
    assert b"grouped stream" in lib.nqa_last_error()
    terms[0].n_groups, streams[0].dtype = 1, 9
    assert lib.nqa_stats_update(streams, 1, terms, 1, None, 0, None, None) == -1
    assert lib.nqa_stats_neighbor_counts(None, -1, 4, None, None) == -1
    assert lib.nqa_stats_neighbor_counts(None, 0, 0, None, None) == 0  # no atoms: nothing to launch


def test_statistics_kernels_do_not_spill():
    """No scratch, no spills (52, 52 and 7 VGPRs at the time of writing), read from the built code object (no GPU)."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    import kernel_resources as kr

    obj = os.path.join(kr.BUILD, "stats.o")
    if not os.path.exists(obj) or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("build objects / ROCm LLVM tools not present (run python -m nequip_amd.csrc.build)")
    ks = kr.kernels_of(obj)
    for needle in ("stats_partial_kernel", "stats_final_kernel", "neighbor_count_kernel"):
        (r,) = [v for n, v in ks.items() if needle in n]
        assert r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] <= 128, (needle, r)
