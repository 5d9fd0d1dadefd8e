"""Every launch of the fused radial MLP (nqa_radial_mlp_* of nequip_amd/csrc/radial_mlp.hip and radial_mlp_pipe.h), called
directly through ctypes and compared output by output, element by element, with the float64 restatements of
tests/radial_mlp_cases.py: num_basis 1..8, the row edges of the 32-row wavefront block and the 128-row tile, ragged and
whole column tiles, every mode an entry point accepts, the training launches' three outputs (the dW0 partials per tile),
the last-layer entry points with and without the second gradient stream, the opt-in kernel variants.  Every output sits
between sentinel guards: a launch has to write all of its output and nothing else."""
# Measured on an MI355X, every figure the largest over the cases of its row (rho = max |X - ref64| / magnitude sum over all
# elements; bound: rho(kernel) <= 3 max(rho(fp32 CPU), rho(exact-fp32 kernel)) + floor; `ratio` = rho(kernel) / rho(fp32 CPU)
# of the same case -- above 3 only where the CPU's own error is small by luck (E = 1, nb = 1), which is what the floor is
# for; `rho/bound` is the margin that is asserted).  train* and tangent rows: sweep (nb 1..8) and per-output cases together.
#
# entry.output                           mode    rho(kernel)  rho(fp32 CPU)  ratio  rho/bound  cases   (each the largest seen)
# bwd.g_emb                              bf16x6  2.813e-08    4.073e-08      10.56   0.26      75
# bwd.g_emb                              f16x3   2.626e-08    4.073e-08       4.32   0.26      75
# bwd.g_emb                              fp32    2.419e-08    4.073e-08       3.88   0.29      75
# fwd.out                                bf16x6  1.190e-07    2.926e-07       1.70   0.15      75
# fwd.out                                f16x3   9.912e-08    2.926e-07       0.89   0.12      75
# fwd.out                                fp32    2.493e-07    2.926e-07       1.56   0.26      75
# last_bwd.grad_pre                      f16x3   4.582e-07    5.548e-07       2.84   0.42      432
# last_bwd2.grad_pre                     f16x3   4.835e-07    5.596e-07       2.77   0.43      432
# last_fwd.out                           f16x3   1.674e-07    3.859e-07       2.94   0.15      432
# paired.g_emb                           bf16x6  2.743e-08    4.093e-08       7.94   0.31      75
# paired.g_emb                           f16x3   2.660e-08    4.093e-08       5.71   0.27      75
# tangent.out                            bf16x6  1.362e-07    2.092e-07       1.26   0.19      183
# train1.g_emb                           bf16x6  4.736e-08    4.073e-08      10.56   0.35      183
# train1.g_emb                           f16x3   6.492e-08    4.073e-08       4.32   0.48      183
# train1.hidden                          bf16x6  3.406e-07    3.348e-07       2.06   0.34      183
# train1.hidden                          f16x3   3.406e-07    3.348e-07       2.06   0.34      183
# train1.parts                           bf16x6  2.511e-07    2.305e-07       2.69   0.46      183
# train1.parts                           f16x3   1.587e-07    2.305e-07       2.04   0.29      183
# train2.g_emb                           bf16x6  3.758e-08    3.377e-08       5.90   0.36      183
# train2.g_emb                           f16x3   3.289e-08    3.377e-08       4.61   0.31      183
# train2.hidden                          bf16x6  3.213e-07    3.235e-07       1.65   0.31      183
# train2.hidden                          f16x3   3.213e-07    3.235e-07       1.65   0.31      183
# train2.parts                           bf16x6  1.856e-07    2.267e-07       3.87   0.40      183
# train2.parts                           f16x3   1.734e-07    2.267e-07       3.20   0.32      183
#
# opt-in variants (nb = 5 and 8) and the many-units cases (nb = 5), both split modes together; a variant of one direction
# runs the other direction's default kernel.  Same columns without the mode:
# bwd:bwd_balanced_prefetch4.g_emb               2.127e-08    1.621e-08       1.31   0.24      12
# bwd:bwd_balanced_ranges.g_emb                  2.127e-08    1.621e-08       1.31   0.24      12
# bwd:bwd_coalesced_rows.g_emb                   1.471e-08    1.227e-08       1.24   0.19      8
# bwd:bwd_half_chip.g_emb                        1.471e-08    1.227e-08       1.24   0.19      8
# bwd:bwd_small_lds_resident.g_emb               1.401e-08    1.227e-08       1.18   0.18      8
# bwd:bwd_small_when_idle.g_emb                  1.401e-08    1.227e-08       1.18   0.18      8
# bwd:fwd_direct_epilogue.g_emb                  1.471e-08    1.227e-08       1.24   0.19      8
# bwd:fwd_one_workgroup_per_block.g_emb          2.127e-08    1.621e-08       1.31   0.24      12
# bwd:general_fwd_bwd.g_emb                      2.127e-08    1.621e-08       1.31   0.24      12
# bwd:many_units.g_emb                           2.547e-08    2.273e-08       1.35   0.24      24
# fwd:bwd_balanced_prefetch4.out                 1.353e-07    2.423e-07       0.69   0.13      12
# fwd:bwd_balanced_ranges.out                    1.353e-07    2.423e-07       0.69   0.13      12
# fwd:bwd_coalesced_rows.out                     8.188e-08    1.271e-07       0.69   0.12      8
# fwd:bwd_half_chip.out                          8.188e-08    1.271e-07       0.69   0.12      8
# fwd:bwd_small_lds_resident.out                 8.188e-08    1.271e-07       0.69   0.12      8
# fwd:bwd_small_when_idle.out                    8.188e-08    1.271e-07       0.69   0.12      8
# fwd:fwd_direct_epilogue.out                    8.188e-08    1.271e-07       0.69   0.12      8
# fwd:fwd_one_workgroup_per_block.out            1.353e-07    2.423e-07       0.69   0.13      12
# fwd:general_fwd_bwd.out                        1.353e-07    2.423e-07       0.69   0.13      12
# fwd:many_units.out                             1.311e-07    2.172e-07       0.65   0.15      14
#
# floors used in that run (largest rho(fp32 CPU) over all cases of the kind, computed on the host of the run):
#   bwd.g_emb 4.093e-08, fwd.out 2.926e-07, last_bwd.grad_pre 5.596e-07, last_fwd.out 3.859e-07
#   tangent.out 2.092e-07, train1.g_emb 4.073e-08, train1.hidden 3.348e-07, train1.parts 2.305e-07
#   train2.g_emb 3.377e-08, train2.hidden 3.235e-07, train2.parts 2.267e-07
#
# Before the compensated exponential of the last-layer kernels (radial_mlp.hip: exp_neg_given_f) the rows of -30 gave
# last_bwd.grad_pre rho = 1.85e-06 (ratio 14.0; W = 4 and 36 failed the bound) and last_fwd.out 6.22e-07 (ratio 5.8).
import math

import pytest
import torch

import radial_mlp_cases as rc
from oracle import nn as onn
from test_radial_mlp import MLP_VARIANTS

TABLE = {}  # (entry.output, mode) -> largest rho(kernel), rho(float32 CPU), ratio: printed when the module is done


@pytest.fixture(scope="module", autouse=True)
def _measured_table():
    yield
    if TABLE:
        print("\n" + rc.format_table(TABLE))


def _run_modes(case, device, modes=None, **kw):
    """All modes of the case's entry point, the exact-fp32 mode (where there is one) first: its rho enters the bound of the
    split modes.  -> failure strings."""
    modes = rc.OPS[case.op][1] if modes is None else modes
    fails, exact = [], None
    for mode in sorted(modes):  # FP32 = 0 first
        f, rhos = rc.run_and_check(case, mode, device, rho_exact=exact, table=TABLE, **kw)
        fails += f
        if mode == rc.FP32 and not f:
            exact = rhos
    return fails


def _refused(case, mode, device, code, **kw):
    _, fails, _ = rc.launch(case, mode, device, expect=code, **kw)
    return fails


@pytest.mark.gpu
def test_train_tiles_are_128_row_tiles(device):
    from nequip_amd import _lib

    lib = _lib.load()
    for E in rc.ROW_EDGES + (0, 256, 2 ** 31 + 1):
        assert lib.nqa_radial_mlp_train_tiles(E) == -(-E // 128) == rc.tiles(E), E


# ---- num_basis sweep ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("op", rc.SWEEP_OPS)
@pytest.mark.parametrize("H,W", rc.SWEEP_HW)
@pytest.mark.parametrize("nb", rc.SWEEP_NB)
def test_num_basis_sweep(device, nb, H, W, op):
    from nequip_amd import _lib

    assert _lib.load().nqa_radial_mlp_supported(_lib.NQA_F32, nb, H, W) == 1
    fails = []
    for case in rc.sweep_cases(op, nb, H, W):
        fails += _run_modes(case, device)
    assert not fails, "\n".join(fails)


# ---- the training launch, output by output ---------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("mode", [rc.BF16X6, rc.F16X3], ids=["bf16x6", "f16x3"])
@pytest.mark.parametrize("op", rc.TRAIN_OPS)
@pytest.mark.parametrize("data", rc.REAL_FORMS)
@pytest.mark.parametrize("H,W", rc.TRAIN_HW)
def test_training_launch_per_output(device, H, W, data, op, mode):
    """g_emb, hidden_out and w0_partials[tile] of nqa_radial_mlp_bwd_train (first order: cotangent null; second order),
    each against its own restatement -- the partials tile by tile, not their sum."""
    fails = []
    for case in rc.train_cases(op, H, W, data):
        got, f, _ = rc.launch(case, mode, device)
        fails += f
        if f:
            continue
        assert got["parts"].shape == (math.ceil(case.E / 128), 8, H)
        for out in ("g_emb", "hidden", "parts"):
            f, rk = rc.check(case, out, got[out], tag=f"[{rc.MODE_NAMES[mode]}]")
            fails += f
            rc.record(TABLE, case, out, mode, rk)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("op", ["train1", "train2", "paired"])
@pytest.mark.parametrize("nb,H,W,E", [(8, 64, 64, 129), (5, 128, 100, 33)])
def test_exact_fp32_refuses_training_forms_and_the_second_stream(device, op, nb, H, W, E):
    fails = _refused(rc.Case(op, nb, H, W, E), rc.FP32, device, rc.NQA_ERR_UNSUPPORTED)
    assert not fails, "\n".join(fails)


# ---- nqa_radial_mlp_fwd_tangent ----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("data", rc.REAL_FORMS)
@pytest.mark.parametrize("H,W", rc.TRAIN_HW)
def test_fwd_tangent(device, H, W, data):
    fails = []
    for case in rc.train_cases("tangent", H, W, data):
        fails += _run_modes(case, device, modes=(rc.BF16X6,))
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("nb,H,W,E", [(8, 64, 64, 129), (5, 128, 100, 33)])
def test_fwd_tangent_refusals_leave_the_output_alone(device, nb, H, W, E):
    case = rc.Case("tangent", nb, H, W, E)
    fails = _refused(case, rc.F16X3, device, rc.NQA_ERR_UNSUPPORTED)
    fails += _refused(case, rc.FP32, device, rc.NQA_ERR_UNSUPPORTED)
    fails += _refused(case, rc.BF16X6, device, rc.NQA_ERR_INVALID, null_cotangent=True)
    assert not fails, "\n".join(fails)


# ---- the last layers of a deeper MLP ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("data", rc.REAL_FORMS + rc.PRE_FORMS)
@pytest.mark.parametrize("W", rc.LAST_W)
@pytest.mark.parametrize("H", rc.LAST_H)
def test_last_layers(device, H, W, data):
    """nqa_radial_mlp_last_fwd, and nqa_radial_mlp_last_bwd with grad_out2 null and with grad_out = 0.25 g,
    grad_out2 = g - 0.25 g, at every row edge."""
    fails = []
    for op in rc.LAST_OPS:
        for case in rc.last_cases(op, H, W, data):
            fails += _run_modes(case, device)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("op", rc.LAST_OPS)
def test_last_layers_refuse_other_modes_and_widths(device, op):
    case = rc.Case(op, 0, 64, 36, 129)
    fails = []
    for mode in (rc.FP32, rc.BF16X6):
        fails += _refused(case, mode, device, rc.NQA_ERR_UNSUPPORTED)
    fails += _refused(case, rc.F16X3, device, rc.NQA_ERR_UNSUPPORTED, H_arg=32)
    assert not fails, "\n".join(fails)


REUSE = [rc.Case(op, 0, 128, 160, 257, "cols") for op in rc.LAST_OPS] + \
        [rc.Case(op, 5, 128, 100, 257, "cols") for op in rc.SWEEP_OPS]


@pytest.mark.gpu
@pytest.mark.parametrize("case", REUSE, ids=lambda c: c.name)
def test_workspace_reuse_is_bit_identical_and_a_short_workspace_is_refused(device, case):
    for mode in rc.OPS[case.op][1]:
        first, fails, ws = rc.launch(case, mode, device, ready=0)
        again, f, _ = rc.launch(case, mode, device, workspace=ws, ready=1)
        fails += f
        assert not fails, "\n".join(fails)
        for out in first:
            assert torch.equal(first[out].view(torch.int32), again[out].view(torch.int32)), (mode, out)
        if ws.needed > 0:
            fails = _refused(case, mode, device, rc.NQA_ERR_WORKSPACE, short_by=1)
            assert not fails, "\n".join(fails)


# ---- the opt-in kernel variants against the reference -----------------------------------------------------------------------------
IDLE = 0x100  # NQA_MLP_HINT_DEVICE_IS_IDLE
VARIANTS = {name: (env, 0) for name, env in MLP_VARIANTS.items()}
VARIANTS["bwd_small_when_idle"] = ({"NQA_MLP_BWD_SMALL": "1"}, IDLE)
# kernels of the variants that are instantiated for H = 64 (the others keep the default kernel there)
H64_VARIANTS = ("general_fwd_bwd", "fwd_one_workgroup_per_block", "bwd_balanced_ranges", "bwd_balanced_prefetch4")


@pytest.mark.gpu
@pytest.mark.parametrize("variant,E,H,W", [(v, E, H, W) for E, H, W in rc.VARIANT_SHAPES for v in VARIANTS
                                            if H == 128 or v in H64_VARIANTS])
def test_opt_in_kernels_against_float64(device, monkeypatch, variant, E, H, W):
    """num_basis 5 and 8, forward and backward, on both split modes (the one-workgroup-per-block forward is a form of the
    bf16 split, the others of the fp16 split)."""
    env, hint = VARIANTS[variant]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fails = []
    for op in ("fwd", "bwd"):
        for case in rc.variant_cases(op, E, H, W):
            for mode in (rc.BF16X6, rc.F16X3):
                got, f, _ = rc.launch(case, mode | (hint if op == "bwd" else 0), device)
                fails += f
                for out, x in ({} if f else got).items():
                    f2, rk = rc.check(case, out, x, tag=f"[{variant} {rc.MODE_NAMES[mode]}]")
                    fails += f2
                    rc.record(TABLE, case, out, mode, rk, label=f"{op}:{variant}")
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", [None] + list(VARIANTS))
def test_more_work_units_than_workgroups(device, monkeypatch, variant):
    """The balanced / persistent kernels with num_basis = 5 where a workgroup takes a range of units, not one."""
    env, hint = VARIANTS[variant] if variant else ({}, 0)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    fails = []
    for case in rc.MANY_UNITS_FWD + rc.MANY_UNITS_BWD:
        if variant and ((case.H == 64 and variant not in H64_VARIANTS) or not variant.startswith(case.op)
                        and variant != "general_fwd_bwd"):
            continue
        for mode in (rc.BF16X6, rc.F16X3):
            got, f, _ = rc.launch(case, mode | (hint if case.op == "bwd" else 0), device)
            fails += f
            for out, x in ({} if f else got).items():
                f2, rk = rc.check(case, out, x, tag=f"[{variant} {rc.MODE_NAMES[mode]}]")
                fails += f2
                rc.record(TABLE, case, out, mode, rk, label=f"{case.op}:many_units")
    assert not fails, "\n".join(fails)


# ---- module level -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("E,H,W", [(129, 64, 36), (1000, 128, 192), (257, 128, 100)])
def test_module_with_five_basis_functions_eval(device, E, H, W):
    from nequip_amd.nn.mlp import ScalarMLPFunction

    torch.manual_seed(E + H + W)
    mlp = ScalarMLPFunction(input_dim=5, output_dim=W, hidden_layers_depth=1, hidden_layers_width=H).eval()
    emb = torch.randn(E, 5) * 0.7
    g = torch.randn(E, W)
    ws = [mlp.mlp[0].weight.detach().double(), mlp.mlp[2].weight.detach().double()]
    e_ref = emb.double().requires_grad_(True)
    ref = onn.scalar_mlp(e_ref, ws, "silu")
    (ge_ref,) = torch.autograd.grad(ref, e_ref, g.double())
    mlp = mlp.to(device)
    e_dev = emb.to(device).requires_grad_(True)
    assert mlp._fused_ok(e_dev), "the fused kernels must take num_basis = 5"
    out = mlp(e_dev)
    (ge,) = torch.autograd.grad(out, e_dev, g.to(device))
    assert ge.shape == (E, 5)
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), atol=1e-5 * float(ref.detach().abs().max()), rtol=1e-5)
    torch.testing.assert_close(ge.cpu().double(), ge_ref, atol=2e-5 * float(ge_ref.abs().max()), rtol=2e-5)


def _force_matching_loss(mlp_fn, emb, v, f_t):
    out = mlp_fn(emb)
    (force,) = torch.autograd.grad((out * v).sum(), emb, create_graph=True)
    return (force - f_t).square().sum() + out.square().sum() / max(1, out.numel())


@pytest.mark.gpu
@pytest.mark.parametrize("E,H,W", [(129, 64, 36), (257, 128, 100)])
def test_module_with_five_basis_functions_train(device, E, H, W):
    from nequip_amd.nn.mlp import ScalarMLPFunction, _RadialMLPTrainFn

    torch.manual_seed(E + W)
    mlp = ScalarMLPFunction(input_dim=5, output_dim=W, hidden_layers_depth=1, hidden_layers_width=H).train()
    emb = torch.randn(E, 5) * 0.7
    v, f_t = torch.randn(E, W), torch.randn(E, 5)
    w_ref = [mlp.mlp[0].weight.detach().double().requires_grad_(True),
             mlp.mlp[2].weight.detach().double().requires_grad_(True)]
    e_ref = emb.double().requires_grad_(True)
    loss_ref = _force_matching_loss(lambda e: onn.scalar_mlp(e, w_ref, "silu"), e_ref, v.double(), f_t.double())
    g_ref = torch.autograd.grad(loss_ref, [e_ref] + w_ref)

    mlp = mlp.to(device)
    e_dev = emb.to(device).requires_grad_(True)
    assert mlp._fused_ok(e_dev)
    seen = []
    orig = _RadialMLPTrainFn.forward
    try:
        _RadialMLPTrainFn.forward = staticmethod(lambda *a, **k: (seen.append(1), orig(*a, **k))[1])
        loss = _force_matching_loss(mlp, e_dev, v.to(device), f_t.to(device))
    finally:
        _RadialMLPTrainFn.forward = staticmethod(orig)
    assert seen, "training mode must run the fused Function pair for num_basis = 5"
    loss.backward()
    got = [e_dev.grad, mlp.mlp[0].weight.grad, mlp.mlp[2].weight.grad]
    torch.testing.assert_close(loss.detach().cpu().double(), loss_ref.detach(), atol=1e-4 * max(1.0, float(loss_ref.detach())), rtol=1e-4)
    for r, g in zip(g_ref, got):
        assert g is not None and g.shape == r.shape
        torch.testing.assert_close(g.cpu().double(), r, atol=2e-4 * float(r.abs().max()), rtol=1e-3)


@pytest.mark.gpu
def test_depth_two_module_width_128_with_five_basis_functions(device):
    from nequip_amd.nn.mlp import ScalarMLPFunction

    torch.manual_seed(13)
    E, H, W = 257, 128, 100
    mlp = ScalarMLPFunction(input_dim=5, output_dim=W, hidden_layers_depth=2, hidden_layers_width=H).eval()
    ws = [m.weight.detach().double() for m in mlp.mlp if hasattr(m, "weight")]
    emb = torch.randn(E, 5) * 0.7
    g = torch.randn(E, W)
    e_ref = emb.double().requires_grad_(True)
    ref = onn.scalar_mlp(e_ref, ws, "silu")
    (ge_ref,) = torch.autograd.grad(ref, e_ref, g.double())
    mlp = mlp.to(device)
    e_dev = emb.to(device).requires_grad_(True)
    assert mlp._deep_ok(e_dev), "the depth-2 MLP must run on the fused kernels and nqa_radial_mlp_last_*"
    out = mlp(e_dev)
    (ge,) = torch.autograd.grad(out, e_dev, g.to(device))
    torch.testing.assert_close(out.detach().cpu().double(), ref.detach(), atol=1e-5 * float(ref.detach().abs().max()), rtol=1e-5)
    torch.testing.assert_close(ge.cpu().double(), ge_ref, atol=2e-5 * float(ge_ref.abs().max()), rtol=2e-5)
