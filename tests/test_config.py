"""``nequip_amd.train.ConFIGGradients`` without a GPU: the restatement against the reference's own method (the fixture
``tests/golden/ref_config.npz``), the Gram form of the kernels against the restatement, the class on CPU tensors, two ranks on
gloo, and the resources of the compiled kernels.

Relative difference means ``max |a - b| / max |b|`` over a whole flat gradient (``config_restatement.rel_diff``).

C2's records (``GRAM_TOL``): the largest relative difference between ``sum_l w_l g_l`` of the Gram form and the restatement's
new gradient, over K = 2, 3, 8, both solver branches and P = 5146 (the parameter list of the GPU test), per case class.  The
``pinv`` branch is reproducible (regular 1.2e-14, dependent 9.6e-15, zero 1.5e-15, tiny 1.2e-12).  The ``lstsq`` branch (LAPACK's
``gelsy``) is threaded and its result moves from run to run: the records are the largest of 20 runs with 32 threads (regular
9.8e-14, dependent 1.7e-14, zero 4.1e-15, tiny 3.7e-11), rounded up to one digit; with one thread, as this test runs, the
figures are 2.5e-14, 9.6e-15, 3.0e-15, 3.1e-11.  Ten times the records are the GPU tolerances (``tests/test_config_gpu.py``).

    regular 1e-13     dependent 2e-14     zero 5e-15     tiny 5e-11

The ``tiny`` class is the one whose normalised Gram matrix is ill-conditioned by construction (a row of norm 1e-12 is divided by
``eps = 1e-8``: an eigenvalue of 1e-8); its figure is the conditioning of the problem, seen by ``lstsq`` and the Gram form alike
(the two branches of the restatement are 3e-11 apart themselves: 1.1e-12 against ``pinv``, 3.2e-11 against ``lstsq``).
"""
import glob
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.abspath(os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", "scripts"))
import config_restatement as cr  # noqa: E402

GRAM_TOL = {"regular": 1e-13, "dependent": 2e-14, "zero": 5e-15, "tiny": 5e-11}
P_GPU = 5146  # 1 + 15 + 1023 + 1024 + 1025 + 2051 + 0 + 7: the parameter list of tests/test_config_gpu.py with a chunk of 1024
F32_ULP = 2.0 ** -23


def assert_grads(got, want64, tol, what):
    """Every ``.grad`` in ``got`` (a list) against the slices of the flat float64 ``want64``: the value before its rounding to
    the parameter's dtype within ``tol`` (relative to the largest element), plus one ulp of that dtype."""
    scale, start = float(want64.abs().max()), 0
    for i, g in enumerate(got):
        w = want64[start:start + g.numel()].view(g.shape).to(g.device)
        start += g.numel()
        ulp = F32_ULP if g.dtype == torch.float32 else 2.0 ** -52
        bound = tol * scale + ulp * w.abs()
        err = (g.double() - w).abs()
        assert bool((err <= bound).all()), f"{what} tensor {i}: error {float(err.max()):.3e}, bound {float(bound.max()):.3e}"
    assert start == want64.numel()


# ---- C1 -------------------------------------------------------------------------------------------------------------------------
def test_restatement_reproduces_the_reference_method():
    """The reference computes in the promoted dtype of the gradients: float64 for the mixed model (its float32 parameters get
    the float64 result rounded once: half a float32 ulp on top of the relative 1e-10), float32 for the all-float32 one.
    Measured distance of the float32 fixture from the float64 restatement: 2.26e-6 (K = 2, lstsq), 1.1e-7 (K = 2, pinv),
    3.1e-7 / 6.5e-7 (K = 3); compared at twice the largest, 4.6e-6."""
    golden = cr.load_golden()
    worst = 0.0
    for kind in cr.GOLDEN_MODELS:
        params = list(cr.GoldenMLP(kind).parameters())
        for k in (2, 3):
            rows = torch.from_numpy(golden[f"rows_{kind}_{k}"])
            assert rows.shape == (k, sum(p.numel() for p in params))
            for tag, lsqr in (("lstsq", True), ("pinv", False)):
                ref = torch.from_numpy(golden[f"grad_{kind}_{k}_{tag}"])
                mine = cr.new_gradient(rows, cr.GOLDEN_COEFFS[k], cr.EPS, lsqr)
                if kind == "mixed":
                    got, start = [], 0
                    for p in params:
                        got.append(ref[start:start + p.numel()].to(p.dtype))
                        start += p.numel()
                    assert_grads(got, mine, 1e-10, f"{kind} K={k} {tag}")
                else:
                    d = cr.rel_diff(mine, ref)
                    worst = max(worst, d)
                    print(f"{kind} K={k} {tag}: distance {d:.3e}")
                    assert d <= 4.6e-6
    assert worst > 1e-8, "the float32 fixture cannot be this close to a float64 computation"


# ---- C2 -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", cr.KS)
def test_gram_form_is_the_restatement(k):
    """``gram_weights`` (ATen) and ``nqa_config_solve_host`` (the function the solve kernel runs, on the host) against both
    solver branches.  Which eigenvalues are dropped must never hang on TAU: with every row at its true length (zero rows left
    out) the spectrum is either well separated (ratio >= 1e-4) or has an exact dependence, i.e. eigenvalues at rounding level
    (<= 1e-14 of the largest).  The issue words this for one spectrum; the row of norm 1e-12, which it names as a case, has its
    small eigenvalue only in the eps-normalised matrix (1e-8), so both spectra are checked: see ``_gram_form_cases``."""
    from nequip_amd.train.config import TAU, gram_weights, solve_host

    assert TAU == cr.TAU == 1e-12
    threads = torch.get_num_threads()
    torch.set_num_threads(1)  # (gelsy's result depends on how its threads split the work: see the module docstring)
    try:
        _gram_form_cases(k, gram_weights, solve_host)
    finally:
        torch.set_num_threads(threads)


def _gram_form_cases(k, gram_weights, solve_host):
    from nequip_amd.train.config import TAU, _jacobi_eigh

    b = torch.tensor(cr.coefficients(k), dtype=torch.float64)
    seen = {}
    for name, cls, rows in cr.cases(k, P_GPU):
        lam = cr.unit_row_spectrum(rows)
        if len(lam):
            ratio = lam / lam.max()
            exact = cls == "dependent"
            assert bool(((ratio >= 1e-4) | ((ratio.abs() <= 1e-14) & exact)).all()), (name, ratio)
            assert exact == bool((ratio.abs() <= 1e-14).any()), (name, ratio)
        gram = rows @ rows.t()
        # ... and on the matrix TAU acts on, Gh = G / (n n') with n = max(|g|, eps): the row of norm 1e-12 is divided by eps and
        # leaves an eigenvalue of 1e-8 (four decades above TAU); nothing kept lies within three decades of TAU * lambda_max, and
        # what is dropped is rounding (a zero row: exactly 0)
        n = gram.diagonal().sqrt().clamp_min(cr.EPS)
        lam_h, _ = _jacobi_eigh((gram / (n[:, None] * n[None, :])).tolist())
        lam_h = torch.tensor(lam_h, dtype=torch.float64)
        if float(lam_h.max()) > 0:
            ratio_h = lam_h / lam_h.max()
            assert bool(((ratio_h >= 1e3 * TAU) | (ratio_h.abs() <= 1e-14)).all()), (name, ratio_h)
            if cls == "tiny":
                assert 1e-9 < float(ratio_h.min()) < 1e-7, (name, ratio_h)
        w, norm = gram_weights(gram, b, cr.EPS)
        host = solve_host(gram, b, cr.EPS)
        assert float(host[9]) == 1.0 and bool((host[k:8] == 0).all())
        for lsqr in (True, False):
            ref = cr.new_gradient(rows, b, cr.EPS, lsqr)
            assert not bool(torch.isnan(ref).any())
            for form, weights, n in (("aten", w, norm), ("host", host[:k], host[8])):
                got = weights @ rows
                assert not bool(torch.isnan(got).any() or torch.isnan(n))
                d = cr.rel_diff(got, ref)
                seen[cls] = max(seen.get(cls, 0.0), d)
                assert d <= GRAM_TOL[cls], (name, form, lsqr, d)
                assert abs(float(n) - float(ref.norm())) <= GRAM_TOL[cls] * max(float(ref.norm()), 1e-300), (name, form)
            if name == "all_zero":
                assert bool((ref == 0).all()) and bool((w @ rows == 0).all()) and bool((host[:k] @ rows == 0).all())
    print({c: f"{v:.2e}" for c, v in seen.items()})


def test_host_solve_folds_the_norm_clip_into_the_weights():
    from nequip_amd.train.config import solve_host

    k = 3
    _, _, rows = cr.cases(k, 64)[0]
    gram, b = rows @ rows.t(), torch.tensor(cr.coefficients(k), dtype=torch.float64)
    plain = solve_host(gram, b, cr.EPS)
    for clip in (0.5 * float(plain[8]), 2.0 * float(plain[8])):
        got = solve_host(gram, b, cr.EPS, "norm", clip)
        factor = min(1.0, clip / (float(plain[8]) + 1e-6))
        assert float(got[8]) == float(plain[8]) and float(got[9]) == factor
        torch.testing.assert_close(got[:k], plain[:k] * factor, rtol=1e-15, atol=0.0)
    assert torch.equal(solve_host(gram, b, cr.EPS, "value", 0.1), plain)  # (the clamp is the apply kernel's)


# ---- C3 -------------------------------------------------------------------------------------------------------------------------
def _golden_step(kind, k, **kw):
    from nequip_amd.train import ConFIGGradients

    model = cr.GoldenMLP(kind)
    loss = cr.make_loss(cr.GOLDEN_NAMES[:k], cr.GOLDEN_COEFFS[k])
    x, target = cr.golden_inputs()
    cf = ConFIGGradients(model, loss, **kw)
    loss_dict = loss(cr.golden_terms(model(x), target, k), {}, prefix="train/")
    return model, loss, cf, loss_dict


def _flat(grads):
    return torch.cat([g.double().flatten() for g in grads])


@pytest.mark.parametrize("kind", cr.GOLDEN_MODELS)
@pytest.mark.parametrize("k", [2, 3])
@pytest.mark.parametrize("lsqr", [True, False])
def test_class_on_cpu_gives_the_restatement(kind, k, lsqr):
    golden = cr.load_golden()
    model, loss, cf, loss_dict = _golden_step(kind, k, lsqr=lsqr)
    assert "train/weighted_sum" in loss_dict
    cf.backward(loss_dict, prefix="train/")
    params = list(model.parameters())
    rows = cf.component_gradients()
    assert rows.dtype == (torch.float64 if kind == "mixed" else torch.float32)  # torch.cat's promotion
    torch.testing.assert_close(rows.double(), torch.from_numpy(golden[f"rows_{kind}_{k}"]), rtol=1e-6, atol=1e-9)
    want = cr.new_gradient(rows, cr.GOLDEN_COEFFS[k], cr.EPS, lsqr)
    for p in params:
        assert p.grad.dtype == p.dtype and p.grad.shape == p.shape
    assert_grads([p.grad for p in params], want, 1e-12, f"{kind} K={k}")
    # ... and the reference's own result: exactly at the fixture's distance from float64 arithmetic
    ref = torch.from_numpy(golden[f"grad_{kind}_{k}_{'lstsq' if lsqr else 'pinv'}"])
    assert cr.rel_diff(_flat(p.grad for p in params), ref) <= (1.3e-7 if kind == "mixed" else 4.6e-6)
    torch.testing.assert_close(cf.weights @ rows.double(), want, rtol=0.0, atol=10 * GRAM_TOL["regular"] * float(want.abs().max()))
    torch.testing.assert_close(cf.grad_norm, want.norm(), rtol=1e-12, atol=0.0)


def test_short_circuits_and_errors():
    from nequip_amd.train import ConFIGGradients

    model, loss, cf, loss_dict = _golden_step("mixed", 3)
    loss.set_coeffs({})
    with pytest.raises(RuntimeError, match="At least one active loss component is required for training"):
        cf.backward(loss_dict, prefix="train/")
    assert all(p.grad is None for p in model.parameters())

    loss.set_coeffs({"mae": 2.0})  # one active term: the plain backward of the weighted sum
    x, target = cr.golden_inputs()
    loss_dict = loss(cr.golden_terms(model(x), target, 3), {}, prefix="train/")
    want = torch.autograd.grad(loss_dict["train/weighted_sum"], list(model.parameters()), retain_graph=True)
    cf.backward(loss_dict, prefix="train/")
    for p, w in zip(model.parameters(), want):
        assert torch.equal(p.grad, w)
    assert cf.weights is None

    names = [f"t{i}" for i in range(9)]
    nine = cr.make_loss(names, [1.0] * 9)
    p = torch.nn.Parameter(torch.ones(4))
    holder = torch.nn.Module()
    holder.p = p
    loss_dict = nine({n: (p * float(i + 1)).sum() for i, n in enumerate(names)}, {})
    with pytest.raises(ValueError, match="at most 8"):
        ConFIGGradients(holder, nine).backward(loss_dict)
    with pytest.raises(ValueError, match="'norm' or 'value'"):
        ConFIGGradients(holder, nine, gradient_clip_val=1.0, gradient_clip_algorithm="both")
    assert ConFIGGradients(holder, nine, gradient_clip_val=1.0).gradient_clip_algorithm == "norm"
    assert ConFIGGradients(holder, nine, gradient_clip_algorithm="value").gradient_clip_algorithm is None


def test_frozen_parameters_are_left_alone_and_unused_ones_get_zeros():
    from nequip_amd.train import ConFIGGradients

    model = cr.GoldenMLP("mixed")
    model.unused = torch.nn.Parameter(torch.ones(3, 2))
    model.b1.requires_grad_(False)
    sentinel = torch.full_like(model.b1, 7.0)
    model.b1.grad = sentinel
    loss = cr.make_loss(cr.GOLDEN_NAMES[:2], cr.GOLDEN_COEFFS[2])
    x, target = cr.golden_inputs()
    loss_dict = loss(cr.golden_terms(model(x), target, 2), {})
    cf = ConFIGGradients(model, loss)
    cf.backward(loss_dict)
    assert model.b1.grad is sentinel and bool((sentinel == 7.0).all())
    assert model.unused.grad is not None and bool((model.unused.grad == 0).all()) and model.unused.grad.shape == (3, 2)
    taking_part = [p for p in model.parameters() if p.requires_grad]
    rows = cf.component_gradients()
    assert rows.shape == (2, sum(p.numel() for p in taking_part))
    assert_grads([p.grad for p in taking_part], cr.new_gradient(rows, cr.GOLDEN_COEFFS[2]), 1e-12, "frozen b1")
    assert float(model.w1.grad.abs().max()) > 0


@pytest.mark.parametrize("algorithm", ["norm", "value"])
@pytest.mark.parametrize("kind", cr.GOLDEN_MODELS)
def test_clipping_is_torchs_applied_to_the_restatements_result(algorithm, kind):
    """``clip_grad_norm_`` / ``clip_grad_value_`` on parameters that carry the restatement's gradient in their own dtypes."""
    _, _, plain, loss_dict = _golden_step(kind, 3)
    plain.backward(loss_dict, prefix="train/")
    unclipped = plain.grad_norm
    clip = {"norm": 0.5 * float(unclipped), "value": 0.05}[algorithm]
    model, _, cf, loss_dict = _golden_step(kind, 3, gradient_clip_val=clip, gradient_clip_algorithm=algorithm)
    cf.backward(loss_dict, prefix="train/")
    twin = cr.GoldenMLP(kind)
    want, start = cr.new_gradient(cf.component_gradients(), cr.GOLDEN_COEFFS[3]), 0
    for p in twin.parameters():
        p.grad = want[start:start + p.numel()].view(p.shape).to(p.dtype)
        start += p.numel()
    if algorithm == "norm":
        torch.nn.utils.clip_grad_norm_(twin.parameters(), clip)
    else:
        torch.nn.utils.clip_grad_value_(twin.parameters(), clip)
        assert sum(int((p.grad.abs() == p.grad.new_tensor(clip)).sum()) for p in twin.parameters()) > 3, "nothing was clamped"
    for p, q in zip(model.parameters(), twin.parameters()):  # (torch scales in the gradient's dtype: a few float32 ulps)
        torch.testing.assert_close(p.grad, q.grad, rtol=4 * F32_ULP, atol=0.0)
    torch.testing.assert_close(cf.grad_norm, unclipped, rtol=1e-12, atol=0.0)
    if algorithm == "norm":
        torch.testing.assert_close(_flat(p.grad for p in model.parameters()).norm(), torch.tensor(clip, dtype=torch.float64),
                                   rtol=1e-5, atol=0.0)


def test_changed_coefficients_are_seen_at_the_next_call():
    model, loss, cf, loss_dict = _golden_step("f32", 3)
    cf.backward(loss_dict, prefix="train/")
    first = _flat(p.grad for p in model.parameters())
    new = {"mse": 0.2, "mae": 0.1, "sumsq": 3.0}
    loss.set_coeffs(new)
    x, target = cr.golden_inputs()
    loss_dict = loss(cr.golden_terms(model(x), target, 3), {}, prefix="train/")
    cf.backward(loss_dict, prefix="train/")
    want = cr.new_gradient(cf.component_gradients(), [new[n] for n in cr.GOLDEN_NAMES])
    assert_grads([p.grad for p in model.parameters()], want, 1e-12, "new coefficients")
    assert cr.rel_diff(first, want) > 1e-2
    with pytest.raises(RuntimeError, match="no backward has run on the kernels"):
        cf.sync_coefficients()  # (CPU tensors: there is no device vector)


# ---- C4 -------------------------------------------------------------------------------------------------------------------------
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
    from nequip_amd.train import ConFIGGradients

    model = cr.GoldenMLP("mixed")
    loss = cr.make_loss(cr.GOLDEN_NAMES, cr.GOLDEN_COEFFS[3])
    x, target = cr.golden_inputs()
    half = slice(0, 4) if rank == 0 else slice(4, 7)
    loss_dict = loss(cr.golden_terms(model(x[half]), target[half], 3), {})
    # pinv: LAPACK's gelsy (lstsq) does not return the same bits for the same matrix in two processes (its result depends on
    # threads and on the alignment of its workspace), and this test asks the ranks for IDENTICAL gradients
    cf = ConFIGGradients(model, loss, lsqr=False)
    cf.backward(loss_dict)
    torch.save({"grads": [p.grad for p in model.parameters()], "rows": cf.component_gradients()},
               os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_on_gloo_share_one_gradient(tmp_path):
    """Each rank backpropagates ``term * world_size`` of its half of the batch and the rows are averaged in one all-reduce: the
    rows are the sums over the ranks of the per-rank gradients (``world_size`` times their mean), on which a single process
    must find the same new gradient."""
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    model = cr.GoldenMLP("mixed")
    params = list(model.parameters())
    x, target = cr.golden_inputs()
    rows = torch.zeros(3, sum(p.numel() for p in params), dtype=torch.float64)
    for half in (slice(0, 4), slice(4, 7)):
        terms = cr.golden_terms(model(x[half]), target[half], 3)
        for i, name in enumerate(cr.GOLDEN_NAMES):
            gs = torch.autograd.grad(terms[name], params, retain_graph=True)
            rows[i] += torch.cat([g.double().flatten() for g in gs])
    want = cr.new_gradient(rows, cr.GOLDEN_COEFFS[3], lsqr=False)
    got = [torch.load(os.path.join(str(tmp_path), f"rank{r}.pt")) for r in range(world)]
    for a, b in zip(got[0]["grads"], got[1]["grads"]):
        assert torch.equal(a, b)
    assert torch.equal(got[0]["rows"], got[1]["rows"])
    torch.testing.assert_close(got[0]["rows"], rows, rtol=1e-12, atol=1e-15)
    assert_grads(got[0]["grads"], want, 1e-12, "two ranks")


# ---- C5 -------------------------------------------------------------------------------------------------------------------------
def test_config_kernels_compile_without_spills():
    import kernel_resources as kr

    objs = glob.glob(os.path.join(kr.BUILD, "config.o"))
    if not objs or not os.path.exists(os.path.join(kr.LLVM, "llvm-readelf")):
        pytest.skip("build objects / ROCm LLVM tools not present (run python -m nequip_amd.csrc.build)")
    ks = {n: r for n, r in kr.kernels_of(objs[0]).items() if "config_" in n}
    assert len(ks) == 5, list(ks)  # collect, gram<float>, gram<double>, solve, apply
    for name, r in ks.items():  # 18 / 92 / 94 / 54 / 24 VGPRs
        assert r["vgpr_spill"] == 0 and r["sgpr_spill"] == 0 and r["scratch"] == 0, (name, r)
        assert kr.waves_per_simd(r["vgpr"]) >= 4, (name, r)
