"""nqa_wgrad (nequip_amd/csrc/wgrad.hip): split-K parameter gradients dW = A^T B against float64 einsum -- the weight-side
backward of ScalarLinearLayer (nequip/nn/mlp.py:262-268), e3nn o3.Linear (interaction_block.py:82-87,129-138) and the
per-type pre-contracted self-connection (:142-146), as restated in oracle/ (the oracle's autograd produces exactly these
einsums)."""
# Measured on an MI355X (rho = max |X - ref64| / (|A|^T |B|); bound: rho(kernel) <= 3 rho(fp32 CPU); the two settings are
# NQA_WGRAD_EXACT_FP32 = 0 and 1, each entry rho(kernel) and its ratio to rho(fp32 CPU)).  The largest ratio is 0.92; the
# CPU emulation without one 2^-16 product gives >= 4.6 (tests/test_wgrad_host.py).
#
# case                   fp32 CPU   0 (default)       1
# dense128-Z67-randn     2.200e-07  1.029e-07 0.47    1.692e-07 0.77
# dense128-Z67-rows      2.089e-07  1.069e-07 0.51    1.308e-07 0.63
# dense128-Z67-cols      2.084e-07  1.062e-07 0.51    1.426e-07 0.68
# dense128-Z1000-randn   7.343e-08  2.792e-08 0.38    3.107e-08 0.42
# dense128-Z1000-rows    7.225e-08  3.253e-08 0.45    3.362e-08 0.47
# dense128-Z1000-cols    6.172e-08  2.686e-08 0.44    3.287e-08 0.53
# dense128-Z4099-randn   2.977e-08  1.579e-08 0.53    1.547e-08 0.52
# dense128-Z4099-rows    2.969e-08  1.343e-08 0.45    1.641e-08 0.55
# dense128-Z4099-cols    2.901e-08  1.605e-08 0.55    1.514e-08 0.52
# typed128-Z67-randn     3.592e-07  2.833e-07 0.79    2.242e-07 0.62
# typed128-Z67-rows      2.185e-07  2.008e-07 0.92    1.811e-07 0.83
# typed128-Z67-cols      2.941e-07  2.564e-07 0.87    2.263e-07 0.77
# typed128-Z1000-randn   1.097e-07  6.546e-08 0.60    4.421e-08 0.40
# typed128-Z1000-rows    1.455e-07  5.666e-08 0.39    4.390e-08 0.30
# typed128-Z1000-cols    1.436e-07  7.038e-08 0.49    6.567e-08 0.46
# typed128-Z4099-randn   4.208e-08  2.793e-08 0.66    2.016e-08 0.48
# typed128-Z4099-rows    3.858e-08  2.966e-08 0.77    1.964e-08 0.51
# typed128-Z4099-cols    6.223e-08  4.334e-08 0.70    3.177e-08 0.51
# dense64-Z67-randn      2.054e-07  1.326e-07 0.65    1.326e-07 0.65
# dense64-Z67-rows       1.983e-07  1.052e-07 0.53    1.052e-07 0.53
# dense64-Z67-cols       2.646e-07  1.043e-07 0.39    1.043e-07 0.39
# dense64-Z1000-randn    7.202e-08  3.512e-08 0.49    3.512e-08 0.49
# dense64-Z1000-rows     5.894e-08  3.605e-08 0.61    3.605e-08 0.61
# dense64-Z1000-cols     5.874e-08  3.622e-08 0.62    3.622e-08 0.62
# dense64-Z4099-randn    2.837e-08  1.440e-08 0.51    1.440e-08 0.51
# dense64-Z4099-rows     2.338e-08  1.940e-08 0.83    1.940e-08 0.83
# dense64-Z4099-cols     2.630e-08  1.678e-08 0.64    1.678e-08 0.64
import subprocess

import pytest
import torch

import wgrad_cases as wc


@pytest.mark.gpu
@pytest.mark.parametrize("E,M,N", [(1000, 128, 704), (4133, 128, 192), (777, 8, 128), (63, 40, 72), (5, 64, 64),
                                   (100000, 128, 96)])
def test_wgrad_dense(device, E, M, N):
    from nequip_amd.utils import wgrad as wg

    torch.manual_seed(E + M + N)
    a, b = torch.randn(E, M), torch.randn(E, N)
    ref = a.double().t() @ b.double()
    got = wg.wgrad(a.to(device), b.to(device), wg.WgradTable([(0, 0, M, N, 1, 0)], M * N)).view(M, N)
    torch.testing.assert_close(got.cpu().double(), ref, atol=2e-6 * float(ref.abs().max()) * max(1.0, (E / 1000) ** 0.5),
                               rtol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5])
@pytest.mark.parametrize("Z", [1, 300, 8192])
def test_wgrad_irreps_blocks(device, T, Z):
    """Several (input block -> output block) matrices with d = 2l+1 components, per atom type."""
    from nequip_amd.utils import wgrad as wg

    torch.manual_seed(Z + T)
    blocks_in = [(64, 1), (64, 3), (32, 5), (16, 7)]   # (mul, d)
    blocks_out = [(96, 1), (64, 3), (64, 5), (8, 7)]
    din = sum(m * d for m, d in blocks_in)
    dout = sum(m * d for m, d in blocks_out)
    x, g = torch.randn(Z, din), torch.randn(Z, dout)
    types = torch.randint(0, T, (Z,))
    recs, ref_parts = [], []
    io = oo = wo = 0
    onehot = torch.nn.functional.one_hot(types, T).double()
    for (mi, d), (mo, _) in zip(blocks_in, blocks_out):
        recs.append((io, oo, mi, mo, d, wo))
        xb = x[:, io:io + mi * d].double().view(Z, mi, d)
        gb = g[:, oo:oo + mo * d].double().view(Z, mo, d)
        ref_parts.append(torch.einsum("zt,zum,zwm->tuw", onehot, xb, gb).reshape(T, mi * mo))
        io, oo, wo = io + mi * d, oo + mo * d, wo + mi * mo
    ref = torch.cat(ref_parts, dim=1)
    got = wg.wgrad(x.to(device), g.to(device), wg.WgradTable(recs, wo), types.to(device) if T > 1 else None, T)
    assert got.shape == (T, wo)
    torch.testing.assert_close(got.cpu().double(), ref, atol=3e-6 * max(1.0, float(ref.abs().max())), rtol=1e-4)


@pytest.mark.gpu
def test_wgrad_partial_coverage_and_empty(device):
    from nequip_amd.utils import wgrad as wg

    a, b = torch.randn(50, 16, device=device), torch.randn(50, 24, device=device)
    tab = wg.WgradTable([(0, 0, 16, 24, 1, 10)], 16 * 24 + 30)  # gap before and after the matrix stays zero
    got = wg.wgrad(a, b, tab)[0]
    assert torch.count_nonzero(got[:10]) == 0 and torch.count_nonzero(got[10 + 16 * 24:]) == 0
    torch.testing.assert_close(got[10:10 + 16 * 24].view(16, 24), a.t() @ b, atol=1e-4, rtol=1e-4)
    empty = wg.wgrad(a[:0], b[:0], wg.WgradTable([(0, 0, 16, 24, 1, 0)], 16 * 24))
    assert empty.shape == (1, 16 * 24) and torch.count_nonzero(empty) == 0
    with pytest.raises(RuntimeError):
        wg.wgrad(a.cpu(), b.cpu(), tab)


# ---- every kernel variant against float64, at tile and row edges (cases and checkers: tests/wgrad_cases.py) ---------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in wc.EXACT_CASES])
def test_wgrad_exact(device, name):
    """Integer data: bit-for-bit equal to the float64 reference, output gaps zero, partial elements outside every record
    untouched (forced-S cases).  Default switch: wgrad_kernel<1 | 2, TYPED, false> and wgrad_kernel<2, TYPED, true>."""
    fails = wc.check_exact(wc.EXACT_BY_NAME[name], device)
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_wgrad_refuses_65_records(device):
    from nequip_amd.utils import wgrad as wg

    recs, lda, ldb, stride = wc.packed(((4, 4, 1),) * (wc.MAX_RECORDS + 1))
    a, b = torch.ones(10, lda, device=device), torch.ones(10, ldb, device=device)
    with pytest.raises(RuntimeError):
        wg.wgrad(a, b, wg.WgradTable(recs, stride))
    got = wg.wgrad(a, b, wg.WgradTable(recs[:-1], stride))[0]
    assert torch.equal(got[:-16], torch.full_like(got[:-16], 10.0)) and torch.count_nonzero(got[-16:]) == 0


@pytest.mark.gpu
def test_wgrad_unwritten_part_of_an_equal_sum_table_is_zero(device):
    """sum(M*N) == out_stride without a tiling (two records at one place): the second half is written by nobody and has to
    come back zero, whatever the allocator hands out."""
    from nequip_amd.utils import wgrad as wg

    Z, M, N = 50, 40, 24
    tab = wg.WgradTable([(0, 0, M, N, 1, 0), (0, 0, M, N, 1, 0)], 2 * M * N)
    a = torch.randint(-8, 9, (Z, M)).float()
    b = torch.randint(-8, 9, (Z, N)).float()
    S = wc.library_splits(tab.records, 1, Z)
    for _ in range(2):  # what the partial tiles are most likely to be carved from
        junk = torch.full((S, 1, tab.out_stride), float("nan"), device=device)
        del junk
    got = wg.wgrad(a.to(device), b.to(device), tab)[0].cpu()
    assert torch.equal(got[:M * N].double().view(M, N), a.double().t() @ b.double())
    assert torch.equal(got[M * N:], torch.zeros(M * N))


@pytest.mark.gpu
def test_wgrad_types_are_converted_or_refused(device):
    """int32 types and a strided view give the gradient of the int64 contiguous tensor; a wrong length raises."""
    from nequip_amd.utils import wgrad as wg

    case = wc.EXACT_BY_NAME["mixed-T5-alternating"]
    a, b, types = wc.make_inputs(case)
    ref = wc.atb(case, a, b, types)
    tab = wg.WgradTable(case.records, case.out_stride)
    ad, bd = a.to(device), b.to(device)
    interleaved = torch.stack([types, (types + 1) % case.T], dim=1).flatten().to(device)  # [::2] is `types`
    assert not interleaved[::2].is_contiguous()
    for t in (types.to(device), types.to(device, torch.int32), interleaved[::2], types):  # (the last one: on the CPU)
        assert torch.equal(wg.wgrad(ad, bd, tab, t, case.T).cpu().double(), ref), (t.dtype, t.device, t.stride())
    for bad in (types[:-1].to(device), torch.cat([types, types]).to(device), types.view(-1, 1).to(device),
                types.float().to(device)):
        with pytest.raises(ValueError):
            wg.wgrad(ad, bd, tab, bad, case.T)
    with pytest.raises(ValueError):
        wg.wgrad(ad, bd, tab, None, case.T)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in wc.ACCURACY_CASES])
def test_wgrad_accuracy_and_determinism(device, name):
    """Real data: rho(kernel) <= 3 rho(float32 CPU product) (the table at the top), and two launches are bitwise equal
    (the kernel's header: "deterministic: no atomics")."""
    case = {c.name: c for c in wc.ACCURACY_CASES}[name]
    fails, rk, r32 = wc.check_accuracy(case, device)
    print(f"{name}: rho(kernel) {rk:.3e} rho(fp32 CPU) {r32:.3e} ratio {rk / r32:.2f}")
    a, b, types = wc.real_reference(case)[:3]
    first, _ = wc.launch(case, a, b, types, device)
    second, _ = wc.launch(case, a, b, types, device)
    assert torch.equal(first, second), "two launches on the same data differ"
    assert not fails, "\n".join(fails)


@pytest.mark.gpu
def test_wgrad_switch_settings_in_child_processes(device):
    """NQA_WGRAD_EXACT_FP32 = 0 and 1 (a function-local static: a fresh process each), one child after another: each
    proves from nqa_wgrad_splits that its setting took effect, then runs the exact-data list and the accuracy cases.
    1: wgrad_kernel<4, *, false> instead of wgrad_kernel<2, *, true>.  The first child that fails, is killed by a signal or
    runs out of time ends the test: no further child is started."""
    for exact_fp32 in wc.SWITCH_SETTINGS:
        done = subprocess.run(wc.child_command("child_gpu_main"), timeout=300, env=wc.child_env(exact_fp32),
                              capture_output=True, text=True)
        print(done.stdout)
        assert done.returncode == 0, (exact_fp32, done.returncode, done.stdout[-4000:], done.stderr[-4000:])
