"""The host layer the STREAM / TERM / SLOT reductions share (``nequip_amd/utils/_slot_plan.py``) through its two users,
``train/_metrics_ops.py::FusedPlan`` and ``data/_stats_ops.py::StatsPlan``: a five-term table on three streams, given OUT of
stream order, against the table order, slots, value indices and ctypes bytes written out by hand."""
import pickle

import pytest
import torch

from nequip_amd import _lib
from nequip_amd.data import _stats_ops as so
from nequip_amd.train import _metrics_ops as mo
from nequip_amd.utils._slot_plan import SlotPlan, canonical_row_scale, canonical_rows, membership

# the terms as (stream, groups) in the caller's order; by stream (stable): terms 1, 4 | 2 | 0, 3
STREAMS = [2, 0, 1, 2, 0]
TABLE_ORDER = [1, 4, 2, 0, 3]


def fused_plan():
    terms = [mo.TermSpec(2, mo.MSE, n_groups=3, coeff=2.0), mo.TermSpec(0, mo.MAXABS, ignore_nan=True),
             mo.TermSpec(1, mo.STRATIFIED_HUBER, strata=[(0.0, 1.0), (2.0, 0.25)], reduce_sum=True),
             mo.TermSpec(2, mo.HUBER, delta=0.5), mo.TermSpec(0, mo.RMSE, n_groups=2, group_coeffs=[3.0, 1.0], coeff=0.5)]
    return mo.FusedPlan(terms, 3)


def stats_plan():
    # T = 3: a per-type term owns 3 slots on the node stream 2 and 9 on the edge stream 0
    terms = [so.TermSpec(2, so.SQUARE, per_type=True), so.TermSpec(0, so.ABS, ignore_nan=True), so.TermSpec(1, so.IDENTITY),
             so.TermSpec(2, so.IDENTITY), so.TermSpec(0, so.IDENTITY, per_type=True)]
    return so.StatsPlan(terms, [so.GROUP_EDGE, so.GROUP_NONE, so.GROUP_NODE], num_types=3)


def raw(table):
    return bytes(memoryview(table).cast("B"))


def test_fused_plan_layout_and_table_bytes():
    plan = fused_plan()
    assert isinstance(plan, SlotPlan) and [t.stream for t in plan.terms] == STREAMS
    assert plan.table_order == TABLE_ORDER
    assert [t.slot0 for t in plan.terms] == [4, 0, 3, 7, 1] and plan.n_slots == 8
    assert [t.out0 for t in plan.terms] == [0, 4, 5, 6, 7] and plan.n_term_values == 10  # (in the CALLER's order)
    assert plan.ws_index == 10 and plan.n_values == 11
    want = (_lib.MetricTerm * 5)()
    rows = [  # stream, kind, n_groups, ignore_nan, reduce_sum, n_strata, has_coeff, has_group_coeffs, slot0, out0, coeff, delta
        (0, mo.MAXABS, 1, 1, 0, 0, 0, 0, 0, 4, 0.0, 1.0), (0, mo.RMSE, 2, 0, 0, 0, 1, 1, 1, 7, 0.5, 1.0),
        (1, mo.STRATIFIED_HUBER, 1, 0, 1, 2, 0, 0, 3, 5, 0.0, 1.0), (2, mo.MSE, 3, 0, 0, 0, 1, 0, 4, 0, 2.0, 1.0),
        (2, mo.HUBER, 1, 0, 0, 0, 0, 0, 7, 6, 0.0, 0.5)]
    names = [f[0] for f in _lib.MetricTerm._fields_[:12]]
    for c, row in zip(want, rows):
        for name, v in zip(names, row):
            setattr(c, name, v)
    want[1].group_coeff[0], want[1].group_coeff[1] = 3.0, 1.0
    want[2].bound[0], want[2].bound[1], want[2].stratum_delta[0], want[2].stratum_delta[1] = 0.0, 2.0, 1.0, 0.25
    assert raw(plan.host_table()) == raw(want)
    assert plan.host_table() is plan.host_table()  # (cached)


def test_stats_plan_layout_and_table_bytes():
    plan = stats_plan()
    assert isinstance(plan, SlotPlan) and plan.n_streams == 3 and plan.table_order == TABLE_ORDER
    assert [t.n_groups for t in plan.terms] == [3, 1, 1, 1, 9]
    assert [t.slot0 for t in plan.terms] == [11, 0, 10, 14, 1] and plan.n_slots == 15
    want = (_lib.StatsTerm * 5)()
    rows = [(0, so.ABS, 1, 1, 0), (0, so.IDENTITY, 9, 0, 1), (1, so.IDENTITY, 1, 0, 10), (2, so.SQUARE, 3, 0, 11),
            (2, so.IDENTITY, 1, 0, 14)]  # stream, mod, n_groups, ignore_nan, slot0
    for c, row in zip(want, rows):
        c.stream, c.mod, c.n_groups, c.ignore_nan, c.slot0 = row
    assert raw(plan.host_table()) == raw(want)


def test_limits_raise_with_the_users_messages():
    with pytest.raises(ValueError, match="9 distinct prediction/target pairs: the fused metric kernels take at most 8"):
        mo.FusedPlan([mo.TermSpec(0, mo.MSE)], 9)
    with pytest.raises(ValueError, match="33 metric terms: the fused metric kernels take at most 32"):
        mo.FusedPlan([mo.TermSpec(0, mo.MSE) for _ in range(33)], 1)
    with pytest.raises(ValueError, match=r"9 distinct fields: the statistics kernels take at most 8 \(NQA_STATS_MAX_STREAMS\)"):
        so.StatsPlan([so.TermSpec(0, so.IDENTITY)], [so.GROUP_NONE] * 9)
    with pytest.raises(ValueError, match=r"1280 groups over all entries: the statistics kernels take at most 1024"):
        so.StatsPlan([so.TermSpec(0, so.IDENTITY, per_type=True) for _ in range(10)], [so.GROUP_NODE], num_types=128)


@pytest.mark.parametrize("make", [fused_plan, stats_plan])
def test_pickling_drops_the_device_buffers_and_keeps_the_tables(make):
    plan = make()
    bufs = plan.buffers("cpu")
    bufs["count"] += 3
    table = raw(plan.host_table())
    assert len(plan._dev) == 1 and plan._host_table is not None
    copy = pickle.loads(pickle.dumps(plan))
    assert copy._dev == {} and copy._host_table is None
    assert copy.table_order == plan.table_order and copy.n_slots == plan.n_slots and raw(copy.host_table()) == table
    assert [vars(t) for t in copy.terms] == [vars(t) for t in plan.terms]
    assert int(copy.buffers("cpu")["count"].sum()) == 0 and int(bufs["count"].sum()) == 3 * plan.n_slots  # (an empty state)


def test_state_planes_and_reset():
    inf = float("inf")
    for plan, init in ((fused_plan(), {"sum": 0.0, "count": 0, "max": -inf}),
                       (stats_plan(), {"count": 0, "mean": 0.0, "mean_lo": 0.0, "m2": 0.0, "min": inf, "max": -inf})):
        bufs = plan.buffers(torch.device("cpu"))
        S = plan.n_slots
        assert bufs["state"].dtype == torch.int64 and bufs["state"].numel() == len(init) * S
        for j, (name, v) in enumerate(init.items()):  # plane j of the state, viewed in its own dtype
            assert bufs[name].dtype == (torch.int64 if name == "count" else torch.float64)
            assert bufs[name].data_ptr() == bufs["state"].data_ptr() + 8 * j * S
            assert bufs[name].tolist() == [v] * S
            bufs[name].fill_(7)
        plan.reset()
        assert all(bufs[name].tolist() == [v] * S for name, v in init.items())
        assert plan.buffers("cpu") is bufs


@pytest.mark.parametrize("shape,want", [((), (1, 1)), ((5,), (5, 1)), ((0, 3), (0, 3)), ((4, 3, 3), (4, 9))])
def test_canonical_rows_shapes(shape, want):
    x = torch.arange(max(1, torch.Size(shape).numel()), dtype=torch.float64)[:torch.Size(shape).numel()].reshape(shape)
    y = canonical_rows(x)
    assert y.shape == want and y.dtype == torch.float64 and y.is_contiguous() and torch.equal(y.reshape(shape), x)
    # what the two drivers make of the same tensor
    p, t, _, _ = mo._canonical(x, x.clone(), None, None)
    s = so._canonical(so.StreamInput(x), so.GROUP_NONE, 0)
    assert p.shape == t.shape == s.data.shape == want and torch.equal(p, y) and torch.equal(s.data, y)


def test_canonical_rows_dtypes_and_views():
    x = torch.randn(6, 4, generator=torch.Generator().manual_seed(0))
    assert canonical_rows(x.bfloat16()).dtype == torch.float32 and canonical_rows(x.half()).dtype == torch.float32
    assert torch.equal(canonical_rows(x.bfloat16()), x.bfloat16().float())
    assert mo._canonical(x.bfloat16(), x.double(), None, None)[0].dtype == torch.float32
    assert so._canonical(so.StreamInput(x.bfloat16()), so.GROUP_NONE, 0).data.dtype == torch.float32
    view = x[:, ::2]  # non-contiguous
    assert canonical_rows(view).is_contiguous() and torch.equal(canonical_rows(view), view)
    ints = torch.arange(6, dtype=torch.int16)
    assert canonical_rows(ints).dtype == torch.float64  # the metrics promote; the statistics keep integers as int64
    assert so._canonical(so.StreamInput(ints), so.GROUP_NONE, 0).data.dtype == torch.int64
    assert so._canonical(so.StreamInput(ints.int()), so.GROUP_NONE, 0).data.dtype == torch.int32


def test_row_scale_and_membership():
    assert canonical_row_scale(None, 4, "cpu") is None
    s = canonical_row_scale(torch.tensor([[1, 2], [3, 4]]), 4, "cpu")
    assert s.dtype == torch.float64 and s.tolist() == [1.0, 2.0, 3.0, 4.0]
    with pytest.raises(AssertionError, match="one scale per row"):
        canonical_row_scale(torch.ones(3), 4, "cpu")
    contrib = torch.tensor([[True, False], [True, True], [False, True]])
    assert torch.equal(membership(None, 1, contrib), contrib[None])
    got = membership(torch.tensor([1, -1, 0]), 2, contrib)  # (a row of group -1 belongs to no group)
    assert got.tolist() == [[[False, False], [False, False], [False, True]], [[True, False], [False, False], [False, False]]]
