"""Parity of the fused edge-embedding HIP kernel (real spherical harmonics + Bessel x polynomial cutoff x factor)
and of its vector-Jacobian product against the oracle (oracle/nn.py, oracle/sh.py), which follows
nequip/nn/embedding/_edge.py:65-80,136-150,193-198 and cutoffs.py:17-27.  Tolerances: 1e-5 (float32 outputs)
/ 1e-9 (float64), as in the reference's tests/unit/nn/test_embed.py:23-49.

Below the first three tests: every entry point of csrc/edge_embed.hip to second order against the float64 oracle, per
edge (tests/edge_embed_cases.py: cases, floors, checker), and CPU tests that the checker rejects wrong oracles and that the
oracle itself is far inside the bounds."""
# Measured maxima of error / bound, bound = tol * scale_e (+ the float32 store roundings), tol = 1e-12 / 1e-11 / 1e-9 for
# forward / VJP / second order.  "kernel": the HIP kernels on an MI355X against the float64 oracle, as
# test_case_through_the_autograd_functions, the paired and the C ABI tests print them; the float32 forward and second-order
# entries are the one rounding to float32 (2^-24 |ref|, next to which tol * scale_e is nothing).  "oracle": the float64
# oracle's radial part alone against the numpy longdouble restatement, through the same checker
# (test_reference_error_is_below_a_tenth_of_the_bounds requires <= 0.1).  Second order: the bound of the clamped edge's
# g_vec2 is 10 x the oracle's measured error there where harmonics do not dominate (edge_embed_cases.reference_limits; the
# oracle is 9e6 .. 2e8 x tol * scale_e off, printed by that test); "emb only vs longdouble" holds the kernel to the plain
# bound on that row as well.  The float64 second-order entries of 1.0e-01 are that row: the kernel agrees with the
# longdouble value, so its distance from the oracle is the oracle's error, a tenth of the moved bound.
#
# case group                         kernel: fwd      vjp   second   oracle: fwd      vjp
# lmax 0-4, float32                   9.9e-01  1.8e-03  9.7e-01        2.7e-04  5.2e-03
# weight sets, float32                9.7e-01  7.7e-05  9.5e-01        3.1e-04  3.7e-03
# cutoff p, float32                   9.7e-01  1.4e-04  9.5e-01        2.2e-04  2.9e-03
# per-edge cutoffs, float32           9.7e-01  5.1e-03  9.7e-01        2.7e-04  5.1e-03
# emb only vs longdouble, float32     7.4e-01  4.9e-05  8.5e-01              -        -
# sh / emb only, float32              9.9e-01  2.4e-03  9.7e-01        3.1e-04  2.4e-03
# requires_grad subsets, float32      9.7e-01  1.8e-04  9.6e-01        2.7e-04  3.4e-03
# E = 0 .. 257, float32               9.7e-01  1.2e-04  9.8e-01        2.7e-04  2.9e-03
# factor 1, float32                   4.6e-01  2.3e-03  8.5e-01        3.3e-04  2.3e-03
# paired launches, float32                  -  4.9e-03        -              -        -
# C ABI, E = 257, float32             9.9e-01  1.2e-04  9.7e-01              -        -
# lmax 0-4, float64                   1.6e-03  2.2e-03  1.0e-01        2.7e-04  7.2e-03
# weight sets, float64                8.9e-04  6.1e-03  1.0e-01        3.1e-04  1.8e-02
# cutoff p, float64                   6.2e-04  5.5e-03  1.0e-01        2.7e-04  6.9e-03
# emb only vs longdouble, float64     8.9e-04  3.8e-04  5.1e-04              -        -
# per-edge cutoffs, float64           8.5e-04  4.1e-03  1.0e-01        2.7e-04  6.0e-03
# sh / emb only, float64              1.6e-03  5.8e-03  1.0e-01        3.1e-04  5.8e-03
# requires_grad subsets, float64      1.1e-03  1.1e-03  9.4e-05        2.7e-04  5.2e-03
# factor 1, float64                   5.6e-04  1.6e-04  1.0e-01        3.3e-04  1.4e-03
# paired launches, float64                  -  2.5e-03        -              -        -
# C ABI, E = 257, float64             7.1e-04  6.8e-03  1.0e-01              -        -
import ctypes
import dataclasses
import math
import types

import pytest
import torch

import edge_embed_cases as ec
from oracle import nn as onn


def _vectors(E, seed=0, r_lo=0.6, r_hi=5.2):
    g = torch.Generator().manual_seed(seed)
    v = torch.randn(E, 3, generator=g, dtype=torch.float64)
    v = v / v.norm(dim=1, keepdim=True)
    r = r_lo + (r_hi - r_lo) * torch.rand(E, 1, generator=g, dtype=torch.float64)
    return v * r


@pytest.mark.gpu
@pytest.mark.parametrize("lmax", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("trained", [False, True])
def test_sh_and_radial_forward_backward(device, lmax, dtype, trained):
    # trained = True: Bessel weights moved off the roots n + 1 (the kernel's angle-addition path only applies to the
    # untrained roots; any other weights take one sin/cos per basis function)
    from nequip_amd.nn.embedding._edge import _EdgeEmbedFn

    tol = 1e-5 if dtype == torch.float32 else 1e-9
    E, r_max, nb, p = 257, 4.5, 8, 6.0
    vec = _vectors(E, seed=lmax)
    vec[0] = torch.tensor([0.0, 4.5 * 1.2, 0.0])  # beyond the cutoff, on the polar axis
    bw = torch.linspace(1.0, nb, nb, dtype=torch.float64)
    if trained:
        bw = bw + 0.07 * torch.randn(nb, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    factor = 2 * math.pi / (r_max * r_max)

    v_ref = vec.clone().requires_grad_(True)
    sh_ref = onn.sh_edge_attrs(v_ref, lmax, dtype)
    emb_ref, _ = onn.bessel_embedding(v_ref, r_max, nb, p, dtype, bessel_weights=bw.unsqueeze(0))

    v_dev = vec.to(device).requires_grad_(True)
    cfg = dict(dtype=dtype, lmax=lmax, want_sh=True, want_emb=True, nb=nb, rmax_recip=1.0 / r_max, p=p, factor=factor)
    sh, emb = _EdgeEmbedFn.apply(v_dev, bw.to(device), cfg)
    torch.testing.assert_close(sh_ref, sh.cpu(), atol=tol, rtol=tol)
    torch.testing.assert_close(emb_ref, emb.cpu(), atol=tol, rtol=tol)
    assert (emb[0] == 0).all(), "embedding must vanish exactly beyond the cutoff"

    g = torch.Generator().manual_seed(5)
    g_sh = torch.randn(sh_ref.shape, generator=g, dtype=dtype)
    g_emb = torch.randn(emb_ref.shape, generator=g, dtype=dtype)
    sh_ref_d = sh_ref if sh_ref.requires_grad else sh_ref + 0.0 * v_ref.sum()  # lmax = 0: Y_0 = 1 is constant
    (gv_ref,) = torch.autograd.grad([sh_ref_d, emb_ref], [v_ref], [g_sh, g_emb])
    (gv,) = torch.autograd.grad([sh, emb], [v_dev], [g_sh.to(device), g_emb.to(device)])
    gtol = 2e-5 if dtype == torch.float32 else 1e-9
    torch.testing.assert_close(gv_ref, gv.cpu(), atol=gtol * float(gv_ref.abs().max()), rtol=gtol)


@pytest.mark.gpu
def test_sh_properties(device):
    """|Y_l|^2 = 2l+1, Y_1 = sqrt(3) r_hat, closed forms for l = 2."""
    from nequip_amd.nn.embedding._edge import _EdgeEmbedFn

    vec = _vectors(100, seed=11).to(device)
    cfg = dict(dtype=torch.float64, lmax=4, want_sh=True, want_emb=False, nb=0, rmax_recip=1.0, p=6.0, factor=1.0)
    Y = _EdgeEmbedFn.apply(vec, torch.ones(1, dtype=torch.float64, device=device), cfg).cpu()
    for l in range(5):
        n2 = (Y[:, l * l : (l + 1) ** 2] ** 2).sum(1)
        torch.testing.assert_close(n2, torch.full_like(n2, 2 * l + 1.0), atol=1e-12, rtol=1e-12)
    u = torch.nn.functional.normalize(vec.cpu(), dim=1)
    x, y, z = u.T
    torch.testing.assert_close(Y[:, 1:4], math.sqrt(3) * u, atol=1e-13, rtol=0)
    torch.testing.assert_close(Y[:, 4], math.sqrt(15) * x * z, atol=1e-13, rtol=0)
    torch.testing.assert_close(Y[:, 6], math.sqrt(5) * (y * y - 0.5 * (x * x + z * z)), atol=1e-13, rtol=0)
    torch.testing.assert_close(Y[:, 8], math.sqrt(15) / 2 * (z * z - x * x), atol=1e-13, rtol=0)


@pytest.mark.gpu
def test_sh_kernel_equals_standard_real_spherical_harmonics(device):
    """The HIP kernel's real spherical harmonics against sympy's Ynm directly (no oracle in between): sqrt(4 pi) x the
    textbook real harmonics with y as the polar axis, plus sign for every (l, m), l <= 4 (see tests/test_oracle.py)."""
    import numpy as np

    from nequip_amd.nn.embedding._edge import _EdgeEmbedFn
    from tests.test_oracle import _standard_real_sh

    vec = _vectors(80, seed=21)
    cfg = dict(dtype=torch.float64, lmax=4, want_sh=True, want_emb=False, nb=0, rmax_recip=1.0, p=6.0, factor=1.0)
    Y = _EdgeEmbedFn.apply(vec.to(device), torch.ones(1, dtype=torch.float64, device=device), cfg).cpu().numpy()
    u = torch.nn.functional.normalize(vec, dim=1).numpy()
    theta, phi = np.arccos(u[:, 1]), np.arctan2(u[:, 0], u[:, 2])
    for l in range(5):
        for m in range(-l, l + 1):
            ref = math.sqrt(4 * math.pi) * np.broadcast_to(_standard_real_sh(l, m)(theta, phi), theta.shape)
            np.testing.assert_allclose(Y[:, l * l + l + m], ref, atol=1e-12, err_msg=f"l={l} m={m}")


# ---- the checker itself (CPU) ------------------------------------------------------------------------------------------------
NAMES_OF_ORDER = {"fwd": ("sh", "emb", "cutoff"), "vjp": ("g_vec",), "second": ("g_vec2", "gg_sh", "gg_emb")}


def _report(case, ratios, tag="RATIO"):
    print(tag, case.name, " ".join(f"{k}={v:.3e}" for k, v in sorted(ratios.items())))


def test_restated_oracle_is_the_oracle():
    """The mutated oracles restate ``bessel_embedding``: with nothing mutated the restatement gives the oracle's bits."""
    for name in set(ec.MUTATION_CASE.values()) | {"p2.5-float64", "factor-one-float64"}:
        case = ec.BY_NAME[name]
        inp, ref = ec.reference(case)
        again = ec.oracle_outputs(case, inp, mutation="restated")
        assert set(again) == set(ref)
        for k in ref:
            assert torch.equal(ref[k], again[k]), (name, k)
        fails, ratios = ec.check(case, inp, ref, again)
        assert not fails and all(v == 0.0 for v in ratios.values())


@pytest.mark.parametrize("mutation", sorted(ec.MUTATIONS))
def test_checker_rejects_a_mutated_oracle(mutation):
    case = ec.BY_NAME[ec.MUTATION_CASE[mutation]]
    inp, ref = ec.reference(case)
    wrong = ec.oracle_outputs(case, inp, mutation=mutation)
    for order in ec.MUTATIONS[mutation]:
        names = [n for n in NAMES_OF_ORDER[order] if n in ref]
        fails, ratios = ec.check(case, inp, ref, wrong, names=names)
        print(f"MUTATION {mutation} {order}: {ratios[order]:.3e} x the bound")
        assert fails, f"the checker accepts the oracle with mutation {mutation!r} at order {order!r}"


@pytest.mark.parametrize("case", [c for c in ec.CASES if c.want_emb and c.E > 0], ids=lambda c: c.name)
def test_reference_error_is_below_a_tenth_of_the_bounds(case):
    """The float64 oracle's radial values, cutoff and dE/dr against the numpy longdouble restatement, through the same
    checker: its own error has to stay below 1/10 of every bound (a condition on the cases and the floors).  At second
    order the same holds on every row but the clamped edge's ``g_vec2``, where the oracle is the limit (see
    ``edge_embed_cases``): that row, and no other, gets 10 x the oracle's measured error as its bound."""
    inp = ec.make_inputs(case)
    radial = dataclasses.replace(case, want_sh=False, dtype="float64")
    inp_r = dict(inp, g_sh=None, g_emb=inp["g_emb"].double())
    got = ec.oracle_outputs(radial, inp_r)
    ld = ec.longdouble_radial(radial, inp_r)
    fails, ratios = ec.check(radial, inp_r, ld, got, names=("emb", "cutoff", "g_vec"), ref_is_oracle=False)
    _report(case, ratios, "REFERENCE")
    assert not fails, "\n".join(fails)
    assert max(ratios.values()) <= 0.1, ratios
    ref = ec.reference(case)[1]
    limits = ec.reference_limits(case, inp, ref)
    fl = ec.floors(case, inp)
    assert not bool(limits["gg_emb"].any())
    rows = limits["g_vec2"].nonzero().flatten().tolist()
    assert rows == ([ec.ROW_CLAMPED] if case.E > ec.ROW_CLAMPED and case.lmax < 2 or not case.want_sh and case.E > ec.ROW_CLAMPED
                    else []), rows
    for e in rows:
        bound = ec.TOL["second"] * max(float(ref["g_vec2"][e].abs().max()), float(fl["g_vec2"][e]))
        print(f"REFERENCE-LIMIT {case.name} g_vec2[{e}]: oracle error {float(limits['g_vec2'][e]):.3e} = "
              f"{float(limits['g_vec2'][e]) / bound:.3e} x tol * scale_e")


def test_named_edges_are_where_the_cases_say():
    vec = ec.edge_set()
    r = vec.norm(dim=1)
    assert vec.shape == (ec.E_FULL, 3) and float(r[ec.NAMED_ROWS[6:7]]) == pytest.approx(1e-3)
    assert float(r[ec.ROW_CLAMPED]) < 1e-12 and float(vec[ec.ROW_AT_CUT].square().sum().sqrt()) == ec.R_MAX
    case = ec.BY_NAME["lmax2-float64"]
    out = ec.outside(case, ec.make_inputs(case))
    assert bool(out[ec.ROW_BEYOND]) and not bool(out[ec.ROW_BELOW_CUT]) and not bool(out[ec.ROW_NEAR_CUT])
    assert bool(out[ec.ROW_AT_CUT]) == (ec.R_MAX * (1.0 / ec.R_MAX) >= 1.0)
    bulk = torch.ones(ec.E_FULL, dtype=torch.bool)
    bulk[list(ec.NAMED_ROWS)] = False
    assert float(r[bulk].min()) >= 0.05 and float(r[bulk].max()) <= 1.15 * ec.R_MAX and int(out[bulk].sum()) > 20
    # every item of the case list, at least once (all cases run all three orders)
    cs = ec.CASES
    assert {(c.lmax, c.dtype) for c in cs} >= {(l, d) for l in range(5) for d in ("float32", "float64")}
    assert {c.weights for c in cs} >= {"one", "roots8", "roots32", "trained8", "trained32", "ulp8", "ulp32"}
    assert {c.p for c in cs} >= {2.0, 2.5, 6.0, 48.0, 64.0} and {c.per_edge for c in cs} == {False, True}
    assert {(c.want_sh, c.want_emb) for c in cs} == {(True, True), (True, False), (False, True)}
    assert {c.grads for c in cs} == {"all", "vec", "cot"} and {c.E for c in cs} >= {0, 1, 255, 256, 257, 513}
    assert {c.factor for c in cs} == {"model", "one"}


# ---- operand checks of the host layer -------------------------------------------------------------------------------------------
def _host_args(device="cpu", E=5, nb=8, lmax=1, dtype=torch.float32):
    vec = torch.randn(E, 3, dtype=torch.float64, device=device)
    bw = torch.linspace(1.0, nb, nb, dtype=torch.float64, device=device)
    cfg = dict(dtype=dtype, lmax=lmax, want_sh=True, want_emb=True, nb=nb, rmax_recip=1 / 4.5, p=6.0, factor=1.0)
    g_sh = torch.randn(E, (lmax + 1) ** 2, dtype=dtype, device=device)
    g_emb = torch.randn(E, nb, dtype=dtype, device=device)
    return vec, bw, cfg, g_sh, g_emb


BAD_WEIGHTS = {
    "float32": lambda bw: bw.float(),
    "too short": lambda bw: bw[:-1].contiguous(),
    "strided": lambda bw: torch.stack([bw, bw], dim=1)[:, 0],
    "not a tensor": lambda bw: bw.tolist(),
}
BAD_RMAX_EDGE = {
    "float32": lambda re: re.float(),
    "wrong length": lambda re: re[:-1].contiguous(),
    "two-dimensional": lambda re: re.view(-1, 1),
    "strided": lambda re: torch.stack([re, re], dim=1)[:, 0],
}


def _launchers(vec, bw, cfg, g_sh, g_emb):
    from nequip_amd.nn.embedding import _edge as M

    pairing = types.SimpleNamespace(rows=torch.zeros(vec.shape[0], dtype=torch.int32, device=vec.device), num_pairs=1)
    c = torch.randn(vec.shape[0], 3, dtype=torch.float64, device=vec.device)
    return {
        "fwd": lambda: M._EdgeEmbedFn.apply(vec, bw, cfg),
        "bwd": lambda: M._EdgeEmbedBwdFn.apply(vec, bw, g_sh, g_emb, cfg),
        "bwd_bwd": lambda: M._edge_embed_second_order(vec, bw, g_sh, g_emb, c, cfg, True, True, True),
        "fwd_paired": lambda: M._EdgeEmbedPairedFn.apply(vec, bw, cfg, pairing),
    }


@pytest.mark.parametrize("entry", ["fwd", "bwd", "bwd_bwd", "fwd_paired"])
def test_bad_operands_are_refused_before_any_launch(entry):
    """On the CPU: the operand checks come before the refusal to run without a GPU, which comes before the library loads."""
    from nequip_amd.nn.embedding._edge import EdgeEmbedOperandError

    vec, bw, cfg, g_sh, g_emb = _host_args()
    with pytest.raises(RuntimeError, match="GPU only"):
        _launchers(vec, bw, cfg, g_sh, g_emb)[entry]()
    for why, spoil in BAD_WEIGHTS.items():
        with pytest.raises(EdgeEmbedOperandError, match="bessel_weights"):
            _launchers(vec, spoil(bw), cfg, g_sh, g_emb)[entry]()
    if entry != "fwd_paired":  # (the paired launches take no per-edge cutoffs)
        re = torch.full((vec.shape[0],), 0.25, dtype=torch.float64)
        with pytest.raises(RuntimeError, match="GPU only"):
            _launchers(vec, bw, dict(cfg, rmax_edge=re), g_sh, g_emb)[entry]()
        for why, spoil in BAD_RMAX_EDGE.items():
            with pytest.raises(EdgeEmbedOperandError, match="rmax_edge"):
                _launchers(vec, bw, dict(cfg, rmax_edge=spoil(re)), g_sh, g_emb)[entry]()


@pytest.mark.parametrize("entry", ["bwd", "bwd_bwd"])
def test_bad_cotangents_are_refused_before_any_launch(entry):
    from nequip_amd.nn.embedding import _edge as M

    vec, bw, cfg, g_sh, g_emb = _host_args()
    for name, a, b in (("g_sh", g_sh.double(), g_emb), ("g_sh", g_sh[:, :-1], g_emb), ("g_sh", g_sh[:-1], g_emb),
                       ("g_emb", g_sh, g_emb.double()), ("g_emb", g_sh, g_emb[:, :-1])):
        with pytest.raises(M.EdgeEmbedOperandError, match=f"cotangent {name}"):
            _launchers(vec, bw, cfg, a, b)[entry]()
    for c in (torch.randn(5, 3), torch.randn(5, 2, dtype=torch.float64), torch.randn(4, 3, dtype=torch.float64)):
        with pytest.raises(M.EdgeEmbedOperandError, match="cotangent c"):
            M._edge_embed_second_order(vec, bw, g_sh, g_emb, c, cfg, True, True, True)


@pytest.mark.gpu
def test_operands_on_another_device_and_paired_cotangents_are_refused(device):
    from nequip_amd.nn.embedding import _edge as M

    vec, bw, cfg, g_sh, g_emb = _host_args(device)
    for entry in ("fwd", "bwd", "bwd_bwd", "fwd_paired"):
        with pytest.raises(M.EdgeEmbedOperandError, match="bessel_weights"):
            _launchers(vec, bw.cpu(), cfg, g_sh, g_emb)[entry]()
    with pytest.raises(M.EdgeEmbedOperandError, match="rmax_edge"):
        M._EdgeEmbedFn.apply(vec, bw, dict(cfg, rmax_edge=torch.full((5,), 0.25, dtype=torch.float64)))
    with pytest.raises(M.EdgeEmbedOperandError, match="cotangent g_emb"):
        M._EdgeEmbedBwdFn.apply(vec, bw, g_sh, g_emb.cpu(), cfg)
    pairing = types.SimpleNamespace(rows=torch.tensor([0, 2, 1, 3, 4], dtype=torch.int32, device=device), num_pairs=2)
    v = vec.clone().requires_grad_(True)
    sh, emb, pairs = M._EdgeEmbedPairedFn.apply(v, bw, cfg, pairing)
    assert pairs.shape == (2, 8)
    # backward() is called directly, with a stand-in for ctx: driven through autograd.grad, autograd's own check of a
    # cotangent's shape against the output fires first and this check of the host layer would never be reached
    with pytest.raises(M.EdgeEmbedOperandError, match="cotangent g_pairs"):
        M._EdgeEmbedPairedFn.backward(types.SimpleNamespace(saved_tensors=(vec, bw), cfg=cfg, pairing=pairing), g_sh, g_emb,
                                      torch.zeros(3, 8, dtype=torch.float32, device=device))


# ---- the case list on the GPU ----------------------------------------------------------------------------------------------------
def _function_backend(case, inp, device):
    from nequip_amd.nn.embedding._edge import _EdgeEmbedBwdFn, _EdgeEmbedFn

    cfg, bw = ec.cfg_of(case, inp, device), inp["bw"].to(device)

    def embed(v):
        out = _EdgeEmbedFn.apply(v, bw, cfg)
        out = list(out) if isinstance(out, tuple) else [out]
        return (out.pop(0) if case.want_sh else None), (out.pop(0) if case.want_emb else None)

    return embed, (lambda v, a, b: _EdgeEmbedBwdFn.apply(v, bw, a, b, cfg))


def _ops_backend(case, inp, device):
    from nequip_amd.nn.embedding import _edge_ops

    cfg, bw = ec.cfg_of(case, inp, device), inp["bw"].to(device)
    flat = (int(cfg["lmax"]), cfg["want_sh"], cfg["want_emb"], int(cfg["nb"]), float(cfg["rmax_recip"]), float(cfg["p"]),
            float(cfg["factor"]), cfg["dtype"] == torch.float32)
    empty = torch.empty(0, dtype=cfg["dtype"], device=device)

    def embed(v):
        out = _edge_ops.edge_embed(v, bw, cfg)
        out = list(out) if isinstance(out, tuple) else [out]
        return (out.pop(0) if case.want_sh else None), (out.pop(0) if case.want_emb else None)

    def vjp(v, a, b):
        return torch.ops.nequip_amd.edge_embed_bwd(v, bw, a if a is not None else empty, b if b is not None else empty, *flat)

    return embed, vjp


def _assert_bitwise(first, second, what):
    assert set(first) == set(second), what
    for k in first:
        assert first[k].dtype == second[k].dtype and first[k].shape == second[k].shape, (what, k)
        assert torch.equal(first[k].view(torch.uint8), second[k].view(torch.uint8)), f"{what}: {k} differs bitwise"


def _expected_outputs(case):
    names = ["g_vec"] + (["sh"] if case.want_sh else []) + (["emb"] if case.want_emb else [])
    if case.grads in ("all", "vec"):
        names.append("g_vec2")
    if case.grads in ("all", "cot"):
        names += (["gg_sh"] if case.want_sh else []) + (["gg_emb"] if case.want_emb else [])
    return set(names)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.name)
def test_case_through_the_autograd_functions(device, case):
    """_EdgeEmbedFn -> _EdgeEmbedBwdFn -> _edge_embed_second_order against the float64 oracle, per edge; twice, bitwise."""
    inp, ref = ec.reference(case)
    embed, vjp = _function_backend(case, inp, device)
    got = ec.run_chain(case, inp, embed, vjp, device)
    assert set(got) == _expected_outputs(case)
    for name in ("sh", "emb", "gg_sh", "gg_emb"):
        assert name not in got or got[name].dtype == case.torch_dtype
    fails, ratios = ec.check(case, inp, ref, got)
    _report(case, ratios)
    if not case.want_sh and case.E > 0:  # radial terms only: the longdouble restatement is a reference too, the clamped
        f2, r2 = ec.check(case, inp, ec.longdouble_radial(case, inp), got, ref_is_oracle=False)  # edge at the plain bound
        _report(case, r2, "RATIO-LONGDOUBLE")
        fails += f2
    _assert_bitwise(got, ec.run_chain(case, inp, embed, vjp, device), case.name)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_one_ulp_off_the_roots_takes_the_direct_path(device):
    """Roots 1..32 with the last one moved by one ulp: every column must come from the one-sin/cos-per-function path
    (bitwise what a launch with the last root at 32.5 gives in its first 31 columns), not from the angle addition (which
    differs in the last bits), and the two paths agree within the bound."""
    base = ec.BY_NAME["embonly-float64"]
    inp, _ = ec.reference(base)
    got = {}
    for kind in ("roots32", "ulp32", "direct32"):
        case = dataclasses.replace(base, name=f"path-{kind}", weights=kind)
        inp_k = dict(inp, bw=ec.bessel_weights(case))
        got[kind] = ec.run_chain(case, inp_k, *_function_backend(case, inp_k, device), device)
        fails, ratios = ec.check(case, inp_k, ec.oracle_outputs(case, inp_k), got[kind])
        _report(case, ratios)
        assert not fails, "\n".join(fails)
    head = slice(0, 31)
    for name in ("emb", "gg_emb"):
        assert torch.equal(got["ulp32"][name][:, head], got["direct32"][name][:, head]), name
        assert not torch.equal(got["ulp32"][name][:, head], got["roots32"][name][:, head]), name
    both = {k: got["ulp32"][k][:, head] for k in ("emb", "gg_emb")}
    rec = {k: got["roots32"][k][:, head] for k in ("emb", "gg_emb")}
    case = dataclasses.replace(base, name="path-head", weights="roots32")
    fl = ec.floors(case, inp)
    for name, order in (("emb", "fwd"), ("gg_emb", "second")):
        scale = torch.maximum(rec[name].abs().amax(dim=1), fl[name])
        assert bool(((both[name] - rec[name]).abs().amax(dim=1) <= 2 * ec.TOL[order] * scale).all()), name


OPS_CASES = ("lmax2-float32", "lmax4-float64", "embonly-float32", "shonly-float64", "grads-vec-float32", "grads-cot-float64",
             "grads-cot-embonly-float64", "grads-cot-shonly-float64", "p2.5-float64", "E1-float32")


@pytest.mark.gpu
@pytest.mark.parametrize("name", OPS_CASES)
def test_dispatcher_ops_equal_the_functions_bitwise(device, name):
    case = ec.BY_NAME[name]
    inp, ref = ec.reference(case)
    fn = ec.run_chain(case, inp, *_function_backend(case, inp, device), device)
    ops = ec.run_chain(case, inp, *_ops_backend(case, inp, device), device)
    assert set(ops) == _expected_outputs(case)
    _assert_bitwise(fn, ops, name)


# ---- paired launches ---------------------------------------------------------------------------------------------------------------
def _hand_pairing(E, device):
    """Representatives and reverses interleaved (rows 2k -> pair k, 2k + 1 -> its reverse, P + k); with an odd E the last edge
    has no partner and carries a row >= P like a reverse edge, so it neither writes nor reads a per-pair row."""
    P = E // 2
    rows = torch.empty(E, dtype=torch.int32)
    rows[0:2 * P:2] = torch.arange(P, dtype=torch.int32)
    rows[1:2 * P:2] = P + torch.arange(P, dtype=torch.int32)
    if E % 2:
        rows[-1] = 2 * P
    return types.SimpleNamespace(rows=rows.to(device), num_pairs=P), torch.arange(0, 2 * P, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,lmax,weights", [("float32", 0, "roots8"), ("float64", 4, "roots32"), ("float32", 4, "trained32"),
                                                ("float64", 0, "trained8")])
def test_paired_launches_with_a_hand_built_pairing(device, dtype, lmax, weights):
    from nequip_amd.nn.embedding._edge import _EdgeEmbedPairedFn

    case = ec.Case(f"paired-{dtype}-l{lmax}-{weights}", dtype=dtype, lmax=lmax, weights=weights)
    inp = ec.make_inputs(case)
    pairing, rep = _hand_pairing(case.E, device)
    assert pairing.num_pairs == 256 and case.E == 513
    cfg, bw = ec.cfg_of(case, inp, device), inp["bw"].to(device)
    plain = ec.run_chain(case, inp, *_function_backend(case, inp, device), device)
    g_pairs = torch.randn(pairing.num_pairs, case.nb, generator=torch.Generator().manual_seed(9), dtype=case.torch_dtype)

    def launch(cots):
        v = inp["vec"].to(device).requires_grad_(True)
        outs = _EdgeEmbedPairedFn.apply(v, bw, cfg, pairing)
        picked = [(o, c.to(device)) for o, c in zip(outs, cots) if c is not None]
        (gv,) = torch.autograd.grad([o for o, _ in picked], [v], [c for _, c in picked])
        return [o.detach().cpu() for o in outs], gv.cpu()

    for cots in ((None, None, g_pairs), (inp["g_sh"], inp["g_emb"], g_pairs)):
        (sh, emb, emb_pairs), gv = launch(cots)
        assert torch.equal(sh, plain["sh"]) and torch.equal(emb, plain["emb"])
        assert torch.equal(emb_pairs, emb[rep])
        (_, _, _), gv_again = launch(cots)
        assert torch.equal(gv, gv_again)
        expanded = torch.zeros(case.E, case.nb, dtype=torch.float64)
        expanded[rep] = g_pairs.double()
        inp_x = dict(inp, g_sh=(cots[0].double() if cots[0] is not None else torch.zeros_like(inp["g_sh"], dtype=torch.float64)),
                     g_emb=expanded + (cots[1].double() if cots[1] is not None else 0.0))
        fails, ratios = ec.check(case, inp_x, ec.oracle_outputs(case, inp_x), dict(g_vec=gv))
        _report(case, ratios, "RATIO-PAIRED" + ("-all" if cots[0] is not None else "-pairs"))
        assert not fails, "\n".join(fails)


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------------
RAW_CASES = {
    "E257-float32": ec.BY_NAME["E257-float32"],
    "E257-peredge-float64": dataclasses.replace(ec.BY_NAME["peredge-float64"], name="E257-peredge-float64", E=257),
    "E257-lmax4-roots32-float32": ec.Case("E257-lmax4-roots32-float32", dtype="float32", lmax=4, weights="roots32", E=257),
    "E257-embonly-p2-float64": dataclasses.replace(ec.BY_NAME["p2-embonly-float64"], name="E257-embonly-p2-float64", E=257),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(RAW_CASES))
def test_raw_abi_cutoff_output_and_the_row_after_the_last_edge(device, name):
    """nqa_edge_embed_fwd / _bwd / _bwd_bwd through ctypes, E = 257 (a second workgroup with one edge): every output buffer
    is one row longer than E and sentinel-filled, and that row has to survive all three launches; the ``cutoff`` output
    (which no Python caller asks for) against the oracle's second return value, alone and next to the other outputs."""
    from nequip_amd import _lib

    lib = _lib.load()
    case = RAW_CASES[name]
    inp, ref = ec.reference(case)
    stream = _lib.stream_ptr(device)
    got, fails = ec.run_raw(case, inp, lib, device, stream)
    assert "cutoff" in got and got["cutoff"].dtype == case.torch_dtype
    f2, ratios = ec.check(case, inp, ref, got)
    _report(case, ratios, "RATIO-RAW")
    assert not (fails + f2), "\n".join(fails + f2)
    again, fails = ec.run_raw(case, inp, lib, device, stream)
    assert not fails, "\n".join(fails)
    _assert_bitwise(got, again, name)
    # only the cutoff pointer set
    head, keep = ec.raw_common(case, inp, device)
    only = ec.padded(case.E, 1, case.torch_dtype, device)
    rc = lib.nqa_edge_embed_fwd(*head, ctypes.c_void_p(), ctypes.c_void_p(), ec._p(only), stream)
    _lib.check(rc, "nqa_edge_embed_fwd")
    torch.cuda.synchronize(device)
    only = only.cpu()
    assert float(only[case.E]) == ec.SENTINEL
    assert torch.equal(only[:case.E], got["cutoff"])


@pytest.mark.gpu
def test_refusals_launch_nothing(device):
    from nequip_amd import _lib

    lib = _lib.load()
    case = ec.BY_NAME["E257-float32"]
    inp = ec.make_inputs(case)
    stream = _lib.stream_ptr(device)
    (dt, lmax, vec, E, rr, re, nb, bw, p, factor), keep = ec.raw_common(case, inp, device)
    null = ctypes.c_void_p()
    g_sh, g_emb, c = inp["g_sh"].to(device), inp["g_emb"].to(device), inp["c"].to(device)
    refusals = {
        "nb=33": (dict(nb=33), "bessel"),
        "p=1.5": (dict(p=1.5), "p >= 2"),
        "lmax=5": (dict(lmax=5), "lmax"),
        "dtype": (dict(dt=7), "dtype"),
        "negative E": (dict(E=-1), "edge vectors"),
        "null vectors": (dict(vec=null), "edge vectors"),
    }
    for why, (change, word) in refusals.items():
        a = dict(dt=dt, lmax=lmax, vec=vec, E=E, rr=rr, re=re, nb=nb, bw=bw, p=p, factor=factor)
        a.update(change)
        head = tuple(a[k] for k in ("dt", "lmax", "vec", "E", "rr", "re", "nb", "bw", "p", "factor"))
        # lmax = 5 needs room for 36 harmonics should the launch happen after all
        bufs = [ec.padded(257, 36, case.torch_dtype, device), ec.padded(257, 40, case.torch_dtype, device),
                ec.padded(257, 1, case.torch_dtype, device), ec.padded(257, 3, torch.float64, device),
                ec.padded(257, 3, torch.float64, device), ec.padded(257, 36, case.torch_dtype, device),
                ec.padded(257, 40, case.torch_dtype, device)]
        sh, emb, cut, g_vec, g_vec2, gg_sh, gg_emb = bufs
        calls = {
            "fwd": lambda: lib.nqa_edge_embed_fwd(*head, ec._p(sh), ec._p(emb), ec._p(cut), stream),
            "bwd": lambda: lib.nqa_edge_embed_bwd(*head, ec._p(g_sh), ec._p(g_emb), ec._p(g_vec), stream),
            "bwd_bwd": lambda: lib.nqa_edge_embed_bwd_bwd(*head, ec._p(g_sh), ec._p(g_emb), ec._p(c), ec._p(gg_sh),
                                                          ec._p(gg_emb), ec._p(g_vec2), stream),
        }
        for fn, call in calls.items():
            rc = call()
            msg = lib.nqa_last_error().decode()
            assert rc != 0, f"nqa_edge_embed_{fn} accepted {why}"
            assert word in msg and f"nqa_edge_embed_{fn}" in msg, (why, fn, msg)
        torch.cuda.synchronize(device)
        for buf in bufs:
            assert bool((buf == ec.SENTINEL).all()), f"{why}: an output buffer was written"
    del keep
