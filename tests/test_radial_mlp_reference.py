"""The reference and the checker of tests/radial_mlp_cases.py, checked themselves (no GPU):

* every float64 restatement equals float64 autograd of the oracle's ScalarMLPFunction restatement (oracle/nn.py::scalar_mlp),
  first order and second order (the gradient of <c, g_emb>), to 1e-12;
* the checker accepts the float32 CPU evaluation of every case on the lists (the reference alone stays within the bound,
  the floors stay below 1e-6) and rejects it with one known defect at a time."""


import pytest
import torch

import radial_mlp_cases as rc
from oracle import nn as onn
from test_f16_split_numerics import scale_up_exponent, split

TOL = 1e-12


def _close(got, want, what):
    torch.testing.assert_close(got, want, rtol=TOL, atol=TOL * max(1e-300, float(want.abs().max())), msg=lambda m: f"{what}: {m}")


# ---- restatements against autograd ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 5, 8])
@pytest.mark.parametrize("data", rc.REAL_FORMS)
def test_restatements_equal_float64_autograd_of_the_oracle(nb, data):
    H, W, E = 64, 36, 150  # two 128-row tiles, the second ragged
    p = rc.make_inputs(rc.Case("fwd", nb, H, W, E, data))
    a0, a1 = rc.alphas(nb, H)
    emb = p["emb"].double().requires_grad_(True)
    w0 = p["w0"].double().requires_grad_(True)
    w1 = p["w1"].double().requires_grad_(True)
    c = p["c"].double()
    val = lambda op, g="g": {k: v.v for k, v in rc.restate(rc.Case(op, nb, H, W, E, data)).items()}

    out = onn.scalar_mlp(emb, [w0, w1], "silu")
    _close(val("fwd")["out"], out.detach(), "fwd out")
    for op, g in (("bwd", p["g"].double()), ("paired", p["g_a"].double() + p["g_b"].double())):
        (ge,) = torch.autograd.grad(out, emb, g, retain_graph=True)
        _close(val(op)["g_emb"], ge, f"{op} g_emb")

    # first-order training form: g_emb, and the pieces of dL/dw1 = alpha1 hidden^T g, dL/dw0 = alpha0 sum_tiles parts
    g = p["g"].double().requires_grad_(True)
    ge, gw0, gw1 = torch.autograd.grad(out, [emb, w0, w1], g, create_graph=True)
    t1 = val("train1")
    assert t1["parts"].shape == (rc.tiles(E), nb, H) and rc.tiles(E) == 2
    _close(t1["g_emb"], ge.detach(), "train1 g_emb")
    _close(a1 * t1["hidden"].t() @ g.detach(), gw1.detach(), "train1 hidden -> dw1")
    _close(a0 * t1["parts"].sum(0), gw0.detach(), "train1 parts -> dw0")
    # each tile's partial is that tile's rows alone: the restatement on the tile's rows as a problem of its own
    for t in range(2):
        lo, hi = t * rc.TILE_ROWS, min(E, (t + 1) * rc.TILE_ROWS)
        sub = {k: (v[lo:hi] if v.shape[0] == E else v) for k, v in p.items()}
        alone = rc.restate(rc.Case("train1", nb, H, W, hi - lo, data), inputs=sub)["parts"].v
        _close(t1["parts"][t], alone[0], f"train1 parts of tile {t}")

    # second order: the gradient of <c, g_emb> w.r.t. emb, w0, w1 and g
    d_emb, d_w0, d_w1, d_g = torch.autograd.grad((c * ge).sum(), [emb, w0, w1, g])
    t2 = val("train2")
    _close(t2["g_emb"], d_emb, "train2 g_emb")
    _close(a1 * t2["hidden"].t() @ g.detach(), d_w1, "train2 hidden -> d<c,g_emb>/dw1")
    _close(a0 * t2["parts"].sum(0), d_w0, "train2 parts -> d<c,g_emb>/dw0")
    _close(val("tangent")["out"], d_g, "tangent out")


@pytest.mark.parametrize("nb", [1, 5, 8])
@pytest.mark.parametrize("data", rc.REAL_FORMS + rc.PRE_FORMS)
def test_last_layer_restatements_equal_float64_autograd_of_the_oracle(nb, data):
    """A depth-2 MLP nb -> H -> H -> W: ``last_fwd`` on the pre-activations the first two weights give is the oracle's
    output; ``last_bwd`` followed by the two-layer ``bwd`` is the oracle's gradient w.r.t. the embedding."""
    H, W, E = 64, 36, 150
    first = rc.make_inputs(rc.Case("fwd", nb, H, H, E, "randn"))
    last = rc.make_inputs(rc.Case("last_fwd", 0, H, W, E, data))
    emb = first["emb"].double().requires_grad_(True)
    ws = [first["w0"].double(), first["w1"].double(), last["w1"].double()]
    out = onn.scalar_mlp(emb, ws, "silu")
    pre = onn.scalar_mlp(emb, ws[:2], "silu").detach()
    for op in ("last_bwd", "last_bwd2"):
        inputs = dict(last, pre=pre)
        got = rc.restate(rc.Case("last_fwd", 0, H, W, E, data), inputs=inputs)["out"].v
        _close(got, out.detach(), "last_fwd out")
        g = (last["g_a"].double() + last["g_b"].double()) if op == "last_bwd2" else last["g"].double()
        (ge,) = torch.autograd.grad(out, emb, g, retain_graph=True)
        grad_pre = rc.restate(rc.Case(op, 0, H, W, E, data), inputs=inputs)["grad_pre"].v
        chain = dict(first, g=grad_pre, g_a=grad_pre, g_b=torch.zeros_like(grad_pre))
        _close(rc.restate(rc.Case("bwd", nb, H, H, E, "randn"), inputs=chain)["g_emb"].v, ge, f"{op} grad_pre -> g_emb")
    # the last layer's own data form: silu and silu' at the case's pre-activations against autograd of torch's silu
    x = last["pre"].double().requires_grad_(True)
    a = rc.alphas(0, H)[1]
    y = torch.nn.functional.silu(x) @ (last["w1"].double() * a)
    (gx,) = torch.autograd.grad(y, x, last["g"].double())
    _close(rc.restate(rc.Case("last_fwd", 0, H, W, E, data))["out"].v, y.detach(), "last_fwd out (own data)")
    _close(rc.restate(rc.Case("last_bwd", 0, H, W, E, data))["grad_pre"].v, gx, "last_bwd grad_pre (own data)")


def test_magnitude_sums_bound_the_values_and_zero_rows_are_as_stated():
    for case in (rc.Case("train2", 5, 64, 36, 150, "rows"), rc.Case("tangent", 5, 64, 36, 150, "cols"),
                 rc.Case("last_bwd2", 0, 64, 36, 150, "neg30")):
        r = rc.reference(case)
        z = rc.zero_row(case.E)
        for out in r.ref:
            assert bool((r.mag[out] >= r.ref[out].abs() * (1 - 1e-12)).all()), (case.name, out)
            rule = rc.ZERO_ROW.get((case.op, out))
            if rule == "0":
                assert not torch.count_nonzero(r.ref[out][z]) and not torch.count_nonzero(r.mag[out][z])
            if rule == "formula":
                assert torch.count_nonzero(r.ref[out][z]) == r.ref[out][z].numel()
    p = rc.make_inputs(rc.Case("train2", 5, 64, 36, 150, "rows"))
    hidden = rc.reference(rc.Case("train2", 5, 64, 36, 150, "rows")).ref["hidden"]
    q = p["c"][75].double() @ (p["w0"].double() * rc.alphas(5, 64)[0])
    torch.testing.assert_close(hidden[75], q / 2, rtol=1e-14, atol=0)


# ---- the checker accepts the reference ... -----------------------------------------------------------------------------------------
GROUPS = sorted({(c.op, c.H) for c in rc.ALL_CASES})


@pytest.mark.parametrize("op,H", GROUPS)
def test_checker_accepts_the_float32_cpu_evaluation_of_every_case(op, H):
    cases = [c for c in rc.ALL_CASES if (c.op, c.H) == (op, H)]
    assert cases
    fails = []
    for case in cases:
        r = rc.reference(case)
        for out in rc.OPS[op][0]:
            f, rk = rc.check(case, out, r.f32[out], tag="[fp32 CPU]")
            assert rk == r.rho32[out]
            fails += f
    assert not fails, "\n".join(fails)


def test_floors_come_from_every_kind_and_stay_below_the_absolute_level():
    floors = rc.floors()
    kinds = {rc.kind(c, out) for c in rc.ALL_CASES for out in rc.OPS[c.op][0]}
    assert set(floors) == kinds
    print("\n".join(f"floor {k}: {v:.3e}" for k, v in sorted(floors.items())))
    for k, v in floors.items():
        assert 0.0 < v <= rc.FLOOR_LIMIT, (k, v)
    # no case is left out by its magnitude: every element is live, or belongs to the all-zero row
    for case in rc.ALL_CASES[::37]:
        r = rc.reference(case)
        z = rc.zero_row(case.E)
        for out, mag in r.mag.items():
            dead = (mag == 0)
            if out != "parts" and z is not None:
                dead[z] = False
            assert not bool(dead.any()), (case.name, out)


def test_case_lists_hold_what_the_launch_tests_promise():
    names = {c.name for c in rc.ALL_CASES}
    assert len(names) == len(rc.ALL_CASES)
    for nb in rc.SWEEP_NB:
        for H, W in rc.SWEEP_HW:
            rows = [E for E, _ in rc.sweep_rows(nb, H, W)]
            assert rows[:2] == [1, 129] and rows[2] in rc.ROW_EDGES and len(set(rows)) == 3
    assert {E for nb in rc.SWEEP_NB for H, W in rc.SWEEP_HW for E, _ in rc.sweep_rows(nb, H, W)} == set(rc.ROW_EDGES)
    assert {d for nb in rc.SWEEP_NB for H, W in rc.SWEEP_HW for _, d in rc.sweep_rows(nb, H, W)} == set(rc.REAL_FORMS)


# ---- ... and rejects it with one defect --------------------------------------------------------------------------------------------
MUTATION_CASES = [rc.Case(op, nb, H, W, E, data)
                  for op in ("fwd", "bwd", "paired", "train1", "train2", "tangent")
                  for nb, H, W, E, data in ((5, 64, 36, 129, "rows"), (8, 128, 100, 257, "randn"), (3, 128, 192, 1000, "cols"))]
MUTATION_CASES += [rc.Case(op, 0, H, W, E, data) for op in rc.LAST_OPS
                   for H, W, E, data in ((64, 36, 129, "rows"), (128, 160, 257, "neg30"), (128, 256, 1000, "cols"))]


def _rejected(case, out, x):
    fails, _ = rc.check(case, out, x, tag="[mutated]")
    return bool(fails)


def _f32(case):
    r = rc.reference(case)
    for out in r.f32:  # the unmodified evaluation is accepted: a rejection below is the defect's doing
        assert not _rejected(case, out, r.f32[out]), (case.name, out)
    return {k: v.clone() for k, v in r.f32.items()}


@pytest.mark.parametrize("case", MUTATION_CASES, ids=lambda c: c.name)
def test_checker_rejects_a_wrong_last_row(case):
    for out, x in _f32(case).items():
        if out == "parts":
            continue
        zeroed = x.clone()
        zeroed[case.E - 1] = 0.0
        assert _rejected(case, out, zeroed), (out, "row E - 1 zeroed")
        copied = x.clone()
        copied[case.E - 1] = x[case.E - 2]
        assert _rejected(case, out, copied), (out, "row E - 1 replaced by row E - 2")


@pytest.mark.parametrize("case", [c for c in MUTATION_CASES if c.op in ("train1", "train2")], ids=lambda c: c.name)
def test_checker_rejects_a_partial_stored_at_the_next_tile(case):
    x = _f32(case)["parts"]
    assert x.shape[0] >= 2
    for t in range(x.shape[0] - 1):
        moved = x.clone()
        moved[t + 1] = x[t]
        moved[t] = x[t + 1]
        assert _rejected(case, "parts", moved), t
    # the sum over the tiles, which is all the module-level tests see, does not notice
    torch.testing.assert_close(moved.sum(0), x.sum(0), rtol=1e-5, atol=1e-5 * float(x.abs().max()))


@pytest.mark.parametrize("case", [c for c in MUTATION_CASES if "g_emb" in rc.OPS[c.op][0]], ids=lambda c: c.name)
def test_checker_rejects_a_stride_8_write_into_stride_nb_rows(case):
    x = _f32(case)["g_emb"]
    nb = case.nb
    shifted = x.clone()
    shifted[1:, nb - 1] = x[:-1, nb - 1]  # the last column holds the previous row's value
    assert _rejected(case, "g_emb", shifted)
    if nb < 8:  # rows written at stride 8 into the [E, nb] buffer, as far as it reaches
        flat = torch.zeros(case.E * 8)
        flat.view(case.E, 8)[:, :nb] = x
        assert _rejected(case, "g_emb", flat[:case.E * nb].view(case.E, nb).clone())


@pytest.mark.parametrize("case", [c for c in MUTATION_CASES if c.data != "cols"], ids=lambda c: c.name)
def test_checker_rejects_a_dropped_column_of_the_last_ragged_chunk(case):
    """Forward-type outputs: column W - 1 not written.  Backward-type: column W - 1 of the gradient left out of the sum
    (not on the ``cols`` form, where that column's group may weigh 2^-60 of the sum and its loss is no error)."""
    W = case.W
    base = _f32(case)
    if "out" in base:
        x = base["out"]
        x[:, W - 1] = 0.0
        assert _rejected(case, "out", x)
        return
    inputs = {k: v.clone() for k, v in rc.make_inputs(case).items()}
    for k in ("g", "g_a", "g_b"):
        inputs[k][:, W - 1] = 0.0
    mutated = rc.restate(case, torch.float32, inputs)
    for out in base:
        if case.op in ("train1", "train2") and out == "hidden":
            continue  # silu(P) and Q silu'(P) do not read the gradient
        assert _rejected(case, out, mutated[out].v), out


def _split_products(x, w, drop=None):
    """x @ w on two fp16 planes per operand, rows of x and 32-column tiles of w scaled by their own power of two: the
    three products hi.hi + hi.lo + lo.hi (tests/test_f16_split_numerics.py), one of them left out with ``drop``."""
    E, Wd = x.shape[0], w.shape[1]
    kx = torch.tensor([scale_up_exponent(float(r.abs().max())) for r in x])
    xh, xl = split(torch.ldexp(x, kx[:, None]), flush=False)
    out = torch.zeros(E, Wd, dtype=torch.float64)
    for t in range(-(-Wd // 32)):
        cols = slice(32 * t, min(Wd, 32 * t + 32))
        kw = scale_up_exponent(float(w[:, cols].abs().max()))
        wh, wl = split(torch.ldexp(w[:, cols], torch.tensor(kw)), flush=False)
        terms = {"hi.hi": xh @ wh, "hi.lo": xh @ wl, "lo.hi": xl @ wh}
        acc = sum(v for k, v in terms.items() if k != drop)
        out[:, cols] = acc * torch.exp2(-(kx[:, None] + kw).double())
    return out.float()


@pytest.mark.parametrize("H,W,E,data", [(64, 36, 129, "randn"), (128, 160, 257, "rows"), (128, 256, 129, "cols")])
def test_checker_rejects_a_split_without_one_2_to_the_minus_11_product(H, W, E, data):
    case = rc.Case("last_fwd", 0, H, W, E, data)
    p = rc.make_inputs(case)
    pre = p["pre"]
    hidden = pre * torch.sigmoid(pre)
    w = p["w1"] * torch.tensor(rc.alphas(0, H)[1], dtype=torch.float32)
    assert not _rejected(case, "out", _split_products(hidden, w)), "the complete three-product split is fp32-accurate"
    for drop in ("hi.lo", "lo.hi"):
        assert _rejected(case, "out", _split_products(hidden, w, drop)), drop
