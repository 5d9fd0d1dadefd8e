"""The cases and the float64 restatement of ``tests/tp_generic_cases.py`` checked on the CPU: the restatement against
``oracle.tp.tp_scatter`` and its autograd, the bound against evaluations that must pass and must fail it, the native plans
(``nqa_plan_create`` / ``nqa_plan_query``: host code, no GPU) against what every case intends, and the agreement of the two
Wigner tables that the float64 bound relies on."""

import numpy as np
import pytest
import torch

import tp_generic_cases as tc
from oracle import tp as otp

F32, F64 = torch.float32, torch.float64


def _oracle(case, dtype):
    """(out, gx, gy, gw) of ``oracle.tp.tp_scatter`` and its autograd on the inputs as ``dtype`` holds them, in float64."""
    x, y, w, g = (t.clone().requires_grad_(True) for t in tc.inputs(case, dtype))
    f_in, e_at, mid = case.plan.strings()
    out = otp.tp_scatter(x, y, w, case.dst, case.src, f_in, e_at, mid, [tuple(i) for i in case.plan.instructions])
    gx, gy, gw = torch.autograd.grad(out, (x, y, w), g.detach(), allow_unused=True)
    return out.detach(), gx, gy, gw


@pytest.mark.parametrize("name", tc.MUL_IR_CASES)
def test_restatement_equals_oracle(name):
    case = tc.make_case(name)
    for dtype in tc.dtypes_of(name):
        ref = tc.reference(name, dtype)
        for key, got in zip(tc.NAMES, _oracle(case, dtype)):
            if got is None:  # (autograd: the operand does not reach the output -- no edges, no instructions)
                got = torch.zeros_like(ref[key].val)
            tc.check(got, ref[key], F64, f"{name} {key} (oracle)")


def _float32_evaluation(name, tables=tc.table):
    case = tc.make_case(name)
    x, y, w, g = (t.to(F32) for t in tc.inputs(case, F32))
    return dict(zip(tc.NAMES, tc.evaluate(case.plan, x, y, w, g, case.dst, case.src, tables)))


@pytest.mark.parametrize("name", [n for n in tc.MUL_IR_CASES if F32 in tc.dtypes_of(n)])
def test_float32_evaluation_passes_float32_bound_and_fails_float64_bound(name):
    ref, got = tc.reference(name, F32), _float32_evaluation(name)
    for key in tc.NAMES:
        tc.check(got[key], ref[key], F32, f"{name} {key} (float32 ATen)")
    if tc.make_case(name).num_edges:
        ratios = [tc.worst(got[key], ref[key], F64)[0] for key in tc.NAMES]
        assert min(ratios) > 1.0, f"{name}: a float32 result within the float64 bound: {ratios}"


def _one_coefficient_off(triple, rel=1e-5):
    """``tables`` with the largest coefficient of ``triple`` scaled by ``1 + rel``."""
    C = tc.table(*triple).clone()
    idx = tuple(int(i) for i in (C.abs() == C.abs().max()).nonzero()[0])
    C[idx] *= 1.0 + rel
    return lambda *l: C if l == triple else tc.table(*l)


@pytest.mark.parametrize("name", tc.TRIPLE_CASES)
def test_wrong_coefficient_fails_float32_bound(name):
    """A table with one coefficient wrong in the sixth digit, evaluated in float64, fails the float32 check of its triple.
    (Not in each of the four quantities: grad_w sums every non-zero coefficient of the triple into one element, up to 61
    terms, and one term's share of that bound can be below 1e-5; the forward and the other two adjoints split the same terms
    over 2l + 1 elements.  Measured over the 65 triples, the worst of the four ratios is at least 2.1.)"""
    case = tc.make_case(name)
    triple = tuple(p[0][1] for p in (case.plan.in1, case.plan.in2, case.plan.out))
    ref = tc.reference(name, F32)
    wrong = tc.restate(case.plan, *tc.inputs(case, F32), case.dst, case.src, _one_coefficient_off(triple))
    ratios = {key: tc.worst(wrong[key].val, ref[key], F32)[0] for key in tc.NAMES}
    assert max(ratios.values()) > 1.0, f"{name}: a wrong coefficient stays within the float32 bound: {ratios}"


def test_wigner_tables_agree():
    """The literals of the kernels (``nequip_amd.o3.wigner``) and the reference's table (``oracle.wigner``): the same zeros,
    and values within ``WIGNER_AGREEMENT`` of each other relative to the largest coefficient of the triple."""
    from nequip_amd.o3.wigner import wigner_3j as product_wigner_3j

    assert len(tc.TRIPLES) == 65
    worst = 0.0
    for triple in tc.TRIPLES:
        ours = torch.from_numpy(np.array(product_wigner_3j(*triple), dtype=np.float64))
        ref = tc.table(*triple)
        assert torch.equal(ours != 0, ref != 0), f"sparsity patterns differ at {triple}"
        worst = max(worst, float((ours - ref).abs().max() / ref.abs().max()))
    print(f"Wigner tables: largest disagreement {worst / 2.0 ** -53:.2f} x 2^-53 of max|C|")
    assert worst <= tc.WIGNER_AGREEMENT


def test_graphs_are_what_the_cases_intend():
    n, (dst, src) = tc.small_graph()
    assert n == 5 and dst.numel() == 12
    assert sorted(torch.bincount(dst, minlength=n).tolist()) == [0, 3, 3, 3, 3]
    assert sorted(torch.bincount(src, minlength=n).tolist()) == [1, 2, 3, 3, 3]
    n, (dst, src) = tc.degree_graph()
    deg = torch.bincount(dst, minlength=n).tolist()
    assert n == 7 and {0, 1, 37} <= set(deg) and 0 in torch.bincount(src, minlength=n).tolist()
    assert bool((dst == src).any())  # a self loop
    pairs = (dst * n + src).tolist()
    assert len(set(pairs)) < len(pairs)  # repeated edges
    assert dst.tolist() != sorted(dst.tolist()) and pairs != sorted(pairs)  # unsorted


def test_layout_permutation_round_trips():
    case = tc.make_case("shared-m5")
    for t, irreps in ((case.x, case.plan.in1), (case.g, case.plan.out)):
        p = tc.to_ir_mul(t, irreps)
        assert not torch.equal(p, t) and torch.equal(tc.to_mul_ir(p, irreps), t)
    # column off + u (2l + 1) + i goes to off + i mul + u
    mul, l = case.plan.in1[1][0], case.plan.in1[1][1]
    off = case.plan.in1[0][0]
    p = tc.to_ir_mul(case.x, case.plan.in1)
    assert torch.equal(p[:, off + 2 * mul + 3], case.x[:, off + 3 * (2 * l + 1) + 2])


# ---- the native plans ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", tc.ALL_CASES)
def test_native_plan_is_what_the_case_intends(name):
    from nequip_amd import _lib

    case = tc.make_case(name)
    plan = tc.native_plan(case)
    d1, d2, do = case.plan.dims
    assert plan.query(_lib.NQA_PLAN_DIM_IN1) == d1
    assert plan.query(_lib.NQA_PLAN_DIM_IN2) == d2
    assert plan.query(_lib.NQA_PLAN_DIM_OUT) == do
    f_in, e_at, _ = case.plan.strings()
    assert plan.query(_lib.NQA_PLAN_WEIGHT_NUMEL) == otp.weight_numel(f_in, e_at, case.plan.instructions)
    assert plan.query(_lib.NQA_PLAN_WEIGHT_NUMEL) == case.plan.weight_numel
    assert plan.query(_lib.NQA_PLAN_NUM_INSTR) == len(case.plan.instructions)
    assert plan.query(_lib.NQA_PLAN_YPART_WIDTH) == tc.expected_ypart_width(case.plan)
    shared = "shared" in name or name in tc.EMPTY_CASES
    assert plan.query(_lib.NQA_PLAN_OUT_NEEDS_ZERO) == (1 if shared else 0)
    if not case.plan.uniform:
        # float32 reaches the generic kernels in-process only through plans without a specialised kernel
        assert plan.query(_lib.NQA_PLAN_HAS_SPECIALIZED) == 0
        assert _lib.load().nqa_tp_bwd_fused_workspace_bytes(plan.handle, _lib.NQA_F32, 0) < 0
    assert _lib.load().nqa_tp_bwd_fused_workspace_bytes(plan.handle, _lib.NQA_F64, 0) < 0


def test_chunk_counts():
    """A second 64-channel chunk (and a partial last one) really exists where a case is named for it, and the forward's
    work items do not fill whole blocks of 4 wavefronts."""
    chunks = {m: tc.num_chunks(tc.chunks_plan(m)) for m in tc.CHUNK_MULS}
    n_instr = len(tc.chunks_plan(1).instructions)
    per_m = [sum(1 for i1, *_ in tc.chunks_plan(1).instructions if i1 < 2)]  # instructions on the two m-channel blocks
    assert chunks[1] == chunks[63] == chunks[64] == n_instr
    assert chunks[65] == n_instr + per_m[0] and chunks[130] == n_instr + 2 * per_m[0]
    assert tc.num_chunks(tc.shared_plan(65)) == 2 * len(tc.shared_plan(5).instructions)
    n = tc.degree_graph()[0]
    not_whole = [m for m in tc.CHUNK_MULS if (n * chunks[m]) % 4]
    assert 65 in not_whole and len(not_whole) >= 3, (chunks, not_whole)
