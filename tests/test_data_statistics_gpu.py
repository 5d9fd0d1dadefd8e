"""The statistics kernels (``csrc/stats.hip``: ``nqa_stats_update`` / ``nqa_stats_neighbor_counts``) on the GPU against
``tests/stats_restatement.py``, the plain-torch float64 restatement of the reference's semantics, evaluated on the same device.

The reference (nequip/data/stats.py, stats_manager.py) cannot be imported here -- it needs ``torchmetrics``, which is not
installed -- so there are no reference-generated fixtures for this feature.

Tolerance: rtol 1e-10, atol 0, NaN equal to NaN (float64 reductions of fewer than 1e5 well-conditioned terms in another order
differ by about n * 2^-53).  Element counts: 1, 63, 64, 65 (a wavefront), 255, 256, 257 (a sweep of a workgroup) and
``G * 256 + 1`` with ``G`` the workgroup count of the first launch (the grid stride wraps once).  T = 3 leaves every stream
with few slots, i.e. 16 owner threads per slot; ``test_owners_per_slot_boundaries`` builds the plans on which the first stage
takes 16, 8 and 1 owners.
"""
import math

import pytest
import torch

import stats_cases as sc
import stats_restatement as sr
from nequip_amd.data import (CommonDataStatisticsManager, DataStatisticsManager, EdgeLengths, Max, Mean, NumNeighbors,
                             StandardDeviation, _stats_ops)

pytestmark = pytest.mark.gpu

TYPES = sc.TYPES
G = _stats_ops.NUM_WORKGROUPS
COUNTS = [1, 63, 64, 65, 255, 256, 257, G * 256 + 1]
F32, F64 = torch.float32, torch.float64


def run(entries, batches, type_names=TYPES):
    """(manager, its statistics) after the batches (fresh dictionaries: the modifiers may add fields)."""
    m = DataStatisticsManager(sc.to_dicts(entries), type_names=type_names)
    return m, m.get_statistics([dict(b) for b in batches])


def frames_of(n, k):
    """``n`` atoms in at most ``k`` frames of unequal sizes."""
    k = min(k, n)
    sizes = [n // k] * k
    sizes[0] += n - sum(sizes)
    return sizes


@pytest.mark.parametrize("dtype", [F32, F64])
@pytest.mark.parametrize("n", COUNTS)
def test_node_streams_against_the_restatement(device, n, dtype):
    """A [N, 1] per-atom field with N the element count (every metric, plain and per type) and the [N, 3] forces next to it;
    T = 3 with ``Cs`` absent; three consecutive batches of n, (n + 1) / 2 and n atoms."""
    entries = sc.entries_for(("charges",)) + sc.entries_for(("forces",), kinds=["rms", "std", "max"])
    batches = [sc.make_batch(frames_of(k, 3), 100 + i, dtype, num_edges=8, device=device)
               for i, k in enumerate([n, (n + 1) // 2, n])]
    _, got = run(entries, batches)
    sc.assert_stats_close(got, sr.evaluate(entries, batches, TYPES))
    assert got["charges|count|all|keep"] == 2 * n + (n + 1) // 2 and got["charges|count|pt|keep"]["Cs"] == 0.0


@pytest.mark.parametrize("e", COUNTS)
def test_edge_streams_against_the_restatement(device, e):
    """E edge lengths (positions, cells and shifts of two frames through ``with_edge_vectors_``), every metric, plain and over
    the nine type pairs of T = 3; three consecutive batches."""
    entries = sc.entries_for(("edge_lengths",))
    batches = [sc.make_batch([20, 30], 200 + i, num_edges=k, type_choices=(0, 1, 2), device=device)
               for i, k in enumerate([e, (e + 1) // 2, e])]
    _, got = run(entries, batches)
    ref = sr.evaluate(entries, batches, TYPES)
    sc.assert_stats_close(got, ref)
    assert len(got["edge_lengths|mean|pt|keep"]) == 9 and got["edge_lengths|count|all|keep"] == 2 * e + (e + 1) // 2


@pytest.mark.parametrize("dtype", [F32, F64])
def test_per_atom_stream_over_four_frames(device, dtype):
    entries = sc.entries_for(("per_atom:total_energy", "total_energy"), per_type=False)
    batches = [sc.make_batch(sizes, 300 + i, dtype, device=device)
               for i, sizes in enumerate([[3, 5, 2, 7], [1, 9, 4, 4], [6, 2, 8, 3]])]
    _, got = run(entries, batches)
    sc.assert_stats_close(got, sr.evaluate(entries, batches, TYPES))


@pytest.mark.parametrize("dtype", [F32, F64])
def test_nan_elements_are_dropped_or_propagate(device, dtype):
    entries = sc.entries_for(("fnan",), kinds=["mean", "rms", "std", "max", "absmin", "count"], ignore_nan=(False, True))
    batches = sc.three_batches(dtype, device=device)
    _, got = run(entries, batches)
    sc.assert_stats_close(got, sr.evaluate(entries, batches, TYPES))
    for kind in ("mean", "rms", "std", "max", "absmin"):
        assert math.isnan(got[f"fnan|{kind}|all|keep"]) and math.isnan(got[f"fnan|{kind}|pt|keep"]["H"])
        assert math.isfinite(got[f"fnan|{kind}|all|drop"]) and math.isfinite(got[f"fnan|{kind}|pt|drop"]["H"])
    assert math.isnan(got["fnan|mean|pt|drop"]["Cs"]) and got["fnan|count|pt|keep"]["Cs"] == 0.0


def test_variance_does_not_cancel(device):
    """Measured on an MI355X: std e_ref = 3.6e-10, e_new = 0.0; mean e_ref = 1.2e-16, e_new = 0.0 (the restatement runs its
    batch reductions on the same device)."""
    errors = sc.cancellation_errors(lambda batches: [{k: v.to(device) for k, v in b.items()} for b in batches], str(device))
    for name, (e_ref, e_new) in errors.items():
        assert e_new <= 10 * e_ref + 1e-12, (name, e_ref, e_new)


def test_num_neighbors_on_an_unsorted_edge_list_with_an_isolated_atom(device):
    data = {"pos": torch.zeros(5, 3, dtype=F64), "atom_types": torch.tensor([0, 0, 1, 1, 1]),
            "edge_index": torch.tensor([[3, 0, 4, 3, 2, 0, 3], [0, 3, 3, 4, 3, 2, 2]])}
    data = {k: v.to(device) for k, v in data.items()}
    m = DataStatisticsManager([{"field": NumNeighbors(), "metric": Mean(), "name": "nn"},
                               {"field": NumNeighbors(), "metric": Mean(), "name": "nn_pt", "per_type": True},
                               {"field": NumNeighbors(), "metric": Max(), "name": "nn_max", "per_type": True}],
                              type_names=["H", "O"])
    got = m.get_statistics([data])
    assert m._plan.neighbor_counts(data["edge_index"], 5).tolist() == NumNeighbors()(data).tolist() == [2, 0, 1, 3, 1]
    assert got["nn"] == pytest.approx(7 / 5, rel=1e-14) and got["nn_pt"] == pytest.approx({"H": 1.0, "O": 5 / 3}, rel=1e-14)
    assert got["nn_max"] == {"H": 2.0, "O": 3.0}
    # ... and a few thousand random edges over three batches, every metric
    entries = sc.entries_for(("num_neighbors",))
    batches = [sc.make_batch(frames_of(n, 3), 400 + i, device=device) for i, n in enumerate([257, 1, 700])]
    _, got = run(entries, batches)
    sc.assert_stats_close(got, sr.evaluate(entries, batches, TYPES))
    assert got["num_neighbors|min|all|keep"] == 0.0  # (the isolated last atom)


def common_plus_edges():
    m = CommonDataStatisticsManager(type_names=TYPES)
    extra = [{"field": EdgeLengths(), "metric": StandardDeviation(), "name": "len_std", "per_type": True},
             {"field": "total_energy", "metric": StandardDeviation(), "name": "e_std"}]
    metrics = [{"name": n, "field": f, "metric": x, "per_type": p}
               for n, f, x, p in zip(m.names, m.fields, m.metrics, m.per_type)]
    return DataStatisticsManager(metrics + extra, type_names=TYPES)


def fixed_shape_batches(device):
    return [sc.make_batch([40, 24], 500 + i, F32, num_edges=900, type_choices=(0, 1, 2), device=device) for i in range(3)]


def test_two_managers_end_with_bit_identical_state(device):
    batches = fixed_shape_batches(device) + [sc.make_batch(frames_of(G * 256 + 1, 2), 510, num_edges=5000, device=device)]
    states = []
    for _ in range(2):
        m = common_plus_edges()
        for b in batches:
            m(dict(b))
        states.append(m._plan.buffers(device)["state"].clone())
    assert torch.equal(states[0], states[1]) and int(states[0][0]) == sum(len(b["pos"]) for b in batches)


def test_gpu_state_against_the_cpu_form(device):
    batches = sc.three_batches(F32)
    gpu, cpu = common_plus_edges(), common_plus_edges()
    for b in batches:
        cpu(dict(b))
        gpu({k: v.to(device) for k, v in b.items()})
    (n_g, hi_g, lo_g, *rest_g), (n_c, hi_c, lo_c, *rest_c) = gpu._plan.state(), cpu._plan.state()
    assert torch.equal(n_g, n_c)
    for a, b in zip([hi_g + lo_g] + rest_g, [hi_c + lo_c] + rest_c):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=0.0, equal_nan=True)
    sc.assert_stats_close(gpu.compute(), cpu.compute())


def test_forward_captures_into_a_graph(device):
    """``manager(data)`` captured once on static buffers (capture itself runs nothing); the buffers are filled with each of
    three batches and the graph replayed: state and ``compute()`` equal those of an eager manager exactly."""
    batches = fixed_shape_batches(device)
    eager, graphed = common_plus_edges(), common_plus_edges()
    for b in batches:
        eager(dict(b))
    static = {k: v.clone() for k, v in batches[0].items()}
    side = torch.cuda.Stream(device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):  # (warm-up: allocations of the plan)
        graphed(dict(static))
    torch.cuda.current_stream(device).wait_stream(side)
    graphed.reset()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        graphed(dict(static))
    for b in batches:
        for k, v in b.items():
            static[k].copy_(v)
        graph.replay()
    torch.cuda.synchronize(device)
    assert torch.equal(graphed._plan.buffers(device)["state"], eager._plan.buffers(device)["state"])
    got, ref = graphed.compute(), eager.compute()
    sc.assert_stats_close(got, ref, rtol=0.0)
    assert got["num_neighbors_mean"] == pytest.approx(900 / 64, rel=1e-14)


def test_cpu_tensors_after_gpu_tensors_keep_a_state_of_their_own(device):
    """As ``MetricsManager``: one running state per device; ``compute()`` merges them (Chan) in the order of first use."""
    batches = sc.three_batches(F64)
    mixed, single = common_plus_edges(), common_plus_edges()
    for i, b in enumerate(batches):
        single(dict(b))
        mixed({k: v.to(device) for k, v in b.items()} if i < 2 else dict(b))
    assert sorted(d.type for d in mixed._plan._dev) == ["cpu", "cuda"]
    sc.assert_stats_close(mixed.compute(), single.compute())


@pytest.mark.parametrize("rows", [1, 257, G * 256 + 1])
@pytest.mark.parametrize("num_types,plain,slots", [(16, False, 16), (16, True, 17), (128, True, 129)])
def test_owners_per_slot_boundaries(device, rows, num_types, plain, slots):
    """The first stage gives a slot 16 owner threads, halved until owners * slots <= 256: one per-type term at T = 16 is the
    last plan with 16 owners (16 slots), one plain term more the first with 8 (17 slots), and T = 128 plus a plain term
    (129 slots) has one owner, which folds the whole sweep of 256 elements.  One [rows, 1] node stream, two batches, against
    the CPU form of the same plan at this file's tolerance; two runs end with the same bits."""
    def plan():
        terms = [_stats_ops.TermSpec(0, _stats_ops.IDENTITY, per_type=True)]
        terms += [_stats_ops.TermSpec(0, _stats_ops.ABS)] if plain else []
        return _stats_ops.StatsPlan(terms, [_stats_ops.GROUP_NODE], num_types=num_types)

    g = torch.Generator().manual_seed(1000 * slots + rows)
    batches = [_stats_ops.StreamInput(0.5 + torch.randn(rows, 1, generator=g, dtype=F64), None,
                                      torch.randint(0, num_types, (rows,), generator=g)) for _ in range(2)]
    cpu, gpu, again = plan(), plan(), plan()
    assert cpu.n_slots == slots
    for b in batches:
        cpu.update([b])
        for p in (gpu, again):
            p.update([_stats_ops.StreamInput(b.data.to(device), None, b.atom_types.to(device))])
    assert torch.equal(gpu.buffers(device)["state"], again.buffers(device)["state"])
    (n_g, hi_g, lo_g, *rest_g), (n_c, hi_c, lo_c, *rest_c) = gpu.state(), cpu.state()
    assert torch.equal(n_g, n_c) and int(n_g[:num_types].sum()) == 2 * rows and (not plain or int(n_g[-1]) == 2 * rows)
    for name, a, b in zip(("mean", "M2", "min", "max"), [hi_g + lo_g] + rest_g, [hi_c + lo_c] + rest_c):
        torch.testing.assert_close(a, b, rtol=1e-10, atol=0.0, equal_nan=True, msg=lambda m, name=name: f"{name}: {m}")
