"""The second-order backward of the tensor-product scatter (force-matching training differentiates the forces once more)
against autograd-through-autograd of the float64 CPU oracle (``oracle/tp.py``).

* Every float32 structure-specialised entry point of that pass -- ``fwd_jvp`` (each non-empty subset of the three
  cotangents), ``bwd_x_dual`` and ``edge_grads_dual`` (with and without ``w_cot``) -- and the first-order entry points,
  at both launch shapes (``NQA_SPEC_WPN`` = 1 / 4, read at every call), at the channel counts of every preset segment
  (derived from ``channel_segments`` as ``test_presets.py`` does: XL's 224 is one full chunk short of four) and at
  32 / 64 / 96 / 128 / 320, on unpaired, paired, high-degree, isolated-node and edge-free graphs.
* The branch matrix of ``_TPScatterBwdFn`` (first and second pass) through ``TensorProductScatter.forward``: every
  subset of operands that require grad, crossed with every subset of cotangents, on a structure with a dual pair kernel,
  one with only a split pair kernel, float64 with pairing and an unpaired graph, under each switch that steers the
  selection; call counters on ``_Kernels`` prove which branch ran.
* The dispatcher-op form on a structure-specialised plan, and a force-matching training step of an XL-shaped model.

The oracle terms come from one double backward per cotangent; the op is linear in each cotangent, so the term of any
subset is the sum of its members' terms.  Tolerances: atol = rtol = 1e-5 scaled by max(1, max|ref|) in float32, 1e-10
in float64.
"""

import collections
import contextlib
import os
import sys

import pytest
import torch

from oracle import tp as otp

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_presets import PRESETS  # noqa: E402
from test_tp_spec_kernels import STRUCTS, _close, _graph, _module, gen_spec  # noqa: E402


BY_NAME = {s[0]: s for s in STRUCTS}
TOL64 = 1e-10


def _near(ref, got, what, tol=None):
    """float64 reference vs kernel result: ``_close`` (float32 tolerance) or ``tol`` (float64); shapes only if empty."""
    got = got.detach().cpu().double()
    assert got.shape == ref.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref.shape)}"
    if ref.numel() == 0:
        return
    if tol is None:
        _close(ref, got, what)
    else:
        torch.testing.assert_close(got, ref, atol=tol * max(1.0, float(ref.abs().max())), rtol=tol,
                                   msg=lambda m: f"{what}: {m}")


@pytest.fixture(autouse=True)
def _oracle_threads():
    """The oracle's CPU threads: OMP_NUM_THREADS, or 16 when unset (never the host's core count)."""
    before = torch.get_num_threads()
    try:
        n = int(os.environ.get("OMP_NUM_THREADS", "") or 16)
    except ValueError:
        n = 16
    torch.set_num_threads(max(1, n))
    yield
    torch.set_num_threads(before)


# ---- cases -----------------------------------------------------------------------------------------------------------
def _preset_segments():
    """{(structure name, mul): preset} of every channel segment of the preset convolutions (middle and last layer)."""
    from nequip_amd.nn._segmented import channel_segments
    from nequip_amd.nn.interaction_block import uvu_paths
    from nequip_amd.o3.irreps import Irreps

    by_key = {gen_spec.nequip_structure(f_in, lmax, f_out, name).key(): name for name, f_in, lmax, f_out in STRUCTS}
    out = {}
    for preset, p in PRESETS.items():
        L = p["l_max"]
        hidden = Irreps([(p["num_features"][l], (l, 1 if l % 2 == 0 else -1)) for l in range(L + 1)])
        sh = Irreps.spherical_harmonics(L)
        for f_out in (hidden, Irreps([(p["num_features"][0], (0, 1))])):
            mid, ins = uvu_paths(hidden, sh, f_out)
            for s in channel_segments(hidden, sh, mid, ins, lambda a, b, c, d: (a, b, c, d)):
                a, b, c, d = s.tp
                st = gen_spec.Structure([m.ir.l for m in a], [m.ir.l for m in b], [m.ir.l for m in c],
                                        [(i, j, k) for i, j, k, *_ in d])
                out.setdefault((by_key[st.key()], s.c1 - s.c0), preset)
    return out


def _kernel_cases():
    cases = _preset_segments()
    assert ("l4n_first", 224) in cases  # XL: 320 - 96 channels of l = 0 only -> three full chunks and a half-full one
    for name in ("l2n_mid", "l3n_mid"):  # pair-centric dual kernel / split pair kernel
        for mul in (32, 64, 96, 128, 320):
            cases.setdefault((name, mul), "mul")
    for mul in (96, 320):
        cases.setdefault(("l4n_first", mul), "mul")
    return [pytest.param(name, mul, id=f"{name}-mul{mul}-{tag}") for (name, mul), tag in sorted(cases.items())]


def _hub_graph(seed, hub_degree=72, n_nodes=90):
    """Pairable: node 1 linked both ways to ``hub_degree`` others (more edges than lanes in a wavefront), a sparse
    ragged rest, node 0 isolated; shuffled."""
    g = torch.Generator().manual_seed(seed)
    pairs = {(1, j) for j in range(2, 2 + hub_degree)}
    for _ in range(30):
        a, b = (int(v) for v in torch.randint(2, n_nodes, (2,), generator=g))
        if a != b:
            pairs.add((min(a, b), max(a, b)))
    pairs = sorted(pairs)
    dst = torch.tensor([a for a, b in pairs] + [b for a, b in pairs])
    src = torch.tensor([b for a, b in pairs] + [a for a, b in pairs])
    perm = torch.randperm(dst.numel(), generator=g)
    return n_nodes, dst[perm].contiguous(), src[perm].contiguous()


def _graphs(seed):
    """(tag, N, dst, src, pairable): repeated directed edges; a pairable ragged list; a hub of degree 72; no edges."""
    out = []
    d, s = _graph(19, seed, symmetric=False)
    out.append(("plain", 19, d, s, False))
    d, s = _graph(19, seed + 1, symmetric=True)
    out.append(("paired", 19, d, s, True))
    n, d, s = _hub_graph(seed + 2)
    out.append(("hub", n, d, s, True))
    e0 = torch.zeros(0, dtype=torch.long)
    out.append(("empty", 6, e0, e0, False))
    return out


# ---- oracle ----------------------------------------------------------------------------------------------------------
def _oracle(spec, x, y, w, go, cots, dst, src):
    """float64 oracle of one graph with per-edge weights ``w``: (out, [gx, gy, gw], T) where ``T[c][t]`` is the
    derivative of <grad_c, cot_c> w.r.t. t in (grad_out, x, y, w), c in (x, y, w): the second-order terms of that
    cotangent."""
    f_in, e_at, mid_s, instructions = spec
    leaves = [t.detach().double().clone().requires_grad_(True) for t in (go, x, y, w)]
    gr, xr, yr, wr = leaves
    out = otp.tp_scatter(xr, yr, wr, dst, src, f_in, e_at, mid_s, instructions)
    grads = torch.autograd.grad(out, (xr, yr, wr), gr, create_graph=True)
    T = []
    for gi, c in zip(grads, cots):
        if gi.requires_grad:
            d = torch.autograd.grad(gi, leaves, c.double(), retain_graph=True, allow_unused=True)
        else:  # (no edges: nothing depends on anything)
            d = (None,) * 4
        T.append([torch.zeros_like(l) if t is None else t.detach() for t, l in zip(d, leaves)])
    return out.detach(), [t.detach() for t in grads], T


def _fold(t, wrow, P):
    """Per-edge weight gradient -> per pair row (the oracle's gather of a pair's row by both its edges)."""
    return torch.zeros((P,) + tuple(t.shape[1:]), dtype=t.dtype).index_add_(0, wrow, t)


def _sum_terms(T, which, target):
    idx = {"x": 0, "y": 1, "w": 2}
    tgt = {"g": 0, "x": 1, "y": 2, "w": 3}[target]
    return sum(T[idx[c]][tgt] for c in which)


# ---- 1. the entry points, at every launch shape and multiplicity -----------------------------------------------------
_ORACLE_CACHE = {}


def _kernel_case_data(name, mul):
    """Inputs of every graph of one (structure, mul), shared by both launch shapes (the test adds the oracle terms on
    first use)."""
    key = (name, mul)
    if key in _ORACLE_CACHE:
        return _ORACLE_CACHE[key]
    _, f_in_1x, lmax, f_out_1x = BY_NAME[name]
    from nequip_amd.o3 import Irreps

    f_in = f_in_1x.replace("1x", f"{mul}x")
    f_out = f_out_1x.replace("1x", f"{mul}x")
    e_at = str(Irreps.spherical_harmonics(lmax))
    mid, instructions = otp.build_instructions(f_in, e_at, f_out)
    mid_s = "+".join(f"{m}x{l}{'e' if p == 1 else 'o'}" for m, l, p in mid)
    spec = (f_in, e_at, mid_s, instructions)
    din, dy, dout = Irreps(f_in).dim, Irreps(e_at).dim, Irreps(mid_s).dim
    wn = otp.weight_numel(f_in, e_at, instructions)
    data = []
    for tag, N, dst, src, pairable in _graphs(seed=7 * mul + lmax):
        E = dst.numel()
        g = torch.Generator().manual_seed(1000 + mul + E)
        x, go, cx = (torch.randn(N, d_, generator=g) for d_ in (din, dout, din))
        y, cy = (torch.randn(E, dy, generator=g) for _ in range(2))
        w, cw = (torch.randn(E, wn, generator=g) for _ in range(2))  # per edge; made pair-symmetric below when paired
        data.append(dict(tag=tag, N=N, dst=dst, src=src, pairable=pairable, x=x, y=y, w=w, go=go, cx=cx, cy=cy, cw=cw))
    _ORACLE_CACHE.clear()  # (one structure at a time: the two launch shapes of a case run next to each other)
    _ORACLE_CACHE[key] = (spec, data)
    return spec, data


def _poison(n, device):
    """Leave NaNs in the caching allocator's next block of this size, so that a row a kernel never writes shows up."""
    t = torch.full((n,), float("nan"), dtype=torch.float32, device=device)
    del t


@pytest.mark.gpu
@pytest.mark.parametrize("wpn", [1, 4])
@pytest.mark.parametrize("name,mul", _kernel_cases())
def test_second_order_kernels_vs_oracle(device, name, mul, wpn, monkeypatch):
    """Each entry point against the matching terms of the oracle's first and double backward; the rows of nodes without
    edges (isolated nodes, the edge-free graph) must come back as exact zeros from outputs allocated uninitialised."""
    from nequip_amd.nn._topology import EdgeTopology

    if os.environ.get("NQA_FORCE_GENERIC", "") not in ("", "0"):
        pytest.skip("specialised kernels switched off")
    monkeypatch.setenv("NQA_SPEC_WPN", str(wpn))
    _, f_in_1x, lmax, f_out_1x = BY_NAME[name]
    tps = _module(f_in_1x, lmax, f_out_1x, mul, device)[0]
    k = tps._get_kernels()
    assert k.has_spec(torch.float32) and k.has_fwd_jvp(torch.float32)
    spec, data = _kernel_case_data(name, mul)
    d = lambda t: t.to(device)  # noqa: E731
    for gd in data:
        N, dst, src = gd["N"], gd["dst"], gd["src"]
        E = dst.numel()
        topo = EdgeTopology(d(dst), d(src), N)
        pr = topo.pairing(None) if gd["pairable"] else None
        assert (pr is not None) == gd["pairable"]
        x, y, go, cx, cy = gd["x"], gd["y"], gd["go"], gd["cx"], gd["cy"]
        if pr is not None:  # one weight row per pair: both edges of a pair see the same row in the oracle's gather
            P = pr.num_pairs
            wrow = pr.rows.long().cpu() % P
            w_rows, cw_rows = gd["w"][:P], gd["cw"][:P]
            w, cw = w_rows[wrow], cw_rows[wrow]
        else:
            w, cw = gd["w"], gd["cw"]
        if "ref" not in gd:  # (per-edge weights: the unpaired run of a pairable graph shares it)
            gd["ref"] = _oracle(spec, x, y, w, go, (cx, cy, cw), dst, src)
        out, (rgx, rgy, rgw), T = gd["ref"]
        # incoming / outgoing edges per node: rows of nodes without any must come back as exact zeros
        no_in = torch.bincount(dst, minlength=N) == 0
        no_out = torch.bincount(src, minlength=N) == 0
        assert bool(no_in[0]) and bool(no_out[0])

        for paired in ((False, True) if pr is not None else (False,)):
            p_ = pr if paired else None
            tag = f"{name} mul={mul} wpn={wpn} {gd['tag']}{' paired' if paired else ''} N={N} E={E}"
            wd = d(w_rows if paired else w)
            cwd = d(cw_rows if paired else cw)
            xd, yd, god, cxd, cyd = d(x), d(y), d(go), d(cx), d(cy)
            gw_ref = _fold(rgw, wrow, P) if paired else rgw

            def node_out(got, ref, what, empty_rows):
                _near(ref, got, f"{what} {tag}")
                assert bool((got.cpu()[empty_rows] == 0).all()), f"{what} {tag}: rows without edges are not zero"

            # first order
            _poison(N * k.dim_out, device)
            node_out(k.fwd(xd, yd, wd, topo, p_), out, "fwd", no_in)
            _poison(N * k.dim_in1, device)
            node_out(k.bwd_x(yd, wd, god, topo, p_), rgx, "bwd_x", no_out)
            gw, gy = k.bwd_edge(xd, yd, wd, god, topo, True, True, pairing=p_)
            _near(gw_ref, _fold_halves(gw, p_), f"bwd_edge gw {tag}")
            _near(rgy, gy, f"bwd_edge gy {tag}")
            _poison(N * k.dim_in1, device)
            fx, fw, fy = k.bwd_fused(xd, yd, wd, god, topo, pairing=p_)
            node_out(fx, rgx, "bwd_fused gx", no_out)
            _near(gw_ref, _fold_halves(fw, p_), f"bwd_fused gw {tag}")
            _near(rgy, fy, f"bwd_fused gy {tag}")
            if paired and k.has_pairs_kernel(torch.float32):
                px, pw, py = k.bwd_pairs(xd, yd, wd, god, topo, p_)
                _near(rgx, px, f"bwd_pairs gx {tag}")
                _near(gw_ref, pw, f"bwd_pairs gw {tag}")
                _near(rgy, py, f"bwd_pairs gy {tag}")

            # second order: forward JVP, every non-empty subset of the cotangents
            for sub in ("x", "y", "w", "xy", "xw", "yw", "xyw"):
                _poison(N * k.dim_out, device)
                got = k.fwd_jvp(xd, yd, wd, cxd if "x" in sub else None, cyd if "y" in sub else None,
                                cwd if "w" in sub else None, topo, p_)
                node_out(got, _sum_terms(T, sub, "g"), f"fwd_jvp[{sub}]", no_in)
            _poison(N * k.dim_in1, device)
            node_out(k.bwd_x_dual(yd, wd, cyd, cwd, god, topo, p_), _sum_terms(T, "yw", "x"), "bwd_x_dual", no_out)
            if paired and k.has_dual_pairs_kernel(torch.float32):
                dw, dy = k.edge_grads_dual(xd, cxd, yd, cyd, wd, god, topo, p_)
                _near(_fold(_sum_terms(T, "xy", "w"), wrow, P), dw, f"edge_grads_dual gw {tag}")
                _near(_sum_terms(T, "x", "y"), dy, f"edge_grads_dual gy {tag}")
                dw3, dy3 = k.edge_grads_dual(xd, cxd, yd, cyd, wd, god, topo, p_, w_cot=cwd)
                _near(_fold(_sum_terms(T, "xy", "w"), wrow, P), dw3, f"edge_grads_dual(w_cot) gw {tag}")
                _near(_sum_terms(T, "xw", "y"), dy3, f"edge_grads_dual(w_cot) gy {tag}")


def _fold_halves(gw, pairing):
    """``bwd_edge`` / ``bwd_fused`` with pairing write the two directed edges of pair p into rows p and p + P."""
    if pairing is None:
        return gw
    P = pairing.num_pairs
    return gw[:P] + gw[P:]


# ---- 2. the branch matrix of _TPScatterBwdFn -------------------------------------------------------------------------
SWITCHES = ("default", "NQA_NO_FWD_JVP", "NQA_NO_DUAL_PAIR_BWD", "NQA_NO_PAIR_BWD", "NQA_NO_FUSED_BWD")
# (structure, mul, dtype, paired graph) -> the first-pass form (all three gradients needed) and the category of the
# second-order edge gradients each case reaches with the default switches
BRANCH_CASES = {
    "dual_pair_kernel": ("l2n_mid", 64, torch.float32, True),
    "split_pair_kernel": ("l3n_mid", 64, torch.float32, True),
    "no_pair_kernel": ("l4n_mid", 32, torch.float32, True),  # (XL's 32-channel l_max = 4 segment)
    "unpaired": ("l2n_mid", 64, torch.float32, False),
    "f64_unpaired": ("l2n_mid", 8, torch.float64, False),  # (float64 has no paired forward: generic kernels only)
}
BRANCH_EXPECT = {"dual_pair_kernel": ("fused_pairs", "dual"), "split_pair_kernel": ("fused_pairs", "pairs"),
                 "no_pair_kernel": ("separate", "buf"), "unpaired": ("fused_rows", "unpaired"),
                 "f64_unpaired": ("separate", "unpaired")}
SUBSETS = ("x", "y", "w", "xy", "xw", "yw", "xyw")
COUNTED = ("fwd", "bwd_x", "bwd_edge", "bwd_fused", "bwd_pairs", "fwd_jvp", "bwd_x_dual", "edge_grads_dual",
           "edge_grads_folded")


def _count_calls(monkeypatch):
    from nequip_amd.nn._tp_scatter_base import _Kernels

    calls = collections.Counter()
    for meth in COUNTED:
        orig = getattr(_Kernels, meth)

        def wrapped(self, *a, _orig=orig, _meth=meth, **kw):
            key = _meth
            if _meth == "bwd_edge" and kw.get("gw_out") is not None:
                key = "bwd_edge[buf]"
            if _meth == "bwd_pairs":
                key = "bwd_pairs[gx]" if kw.get("need_gx", True) else "bwd_pairs[edge]"
            calls[key] += 1
            return _orig(self, *a, **kw)

        monkeypatch.setattr(_Kernels, meth, wrapped)
    return calls


def _first_pass_branch(calls):
    if calls["bwd_pairs[gx]"]:
        return "fused_pairs"
    if calls["bwd_fused"] and not calls["bwd_x"]:  # (bwd_fused returns None without a specialised kernel)
        return "fused_rows"
    return "separate"


def _second_pass_branch(calls):
    if calls["edge_grads_dual"]:
        return "dual"
    if calls["bwd_pairs[edge]"]:
        return "pairs"
    if calls["bwd_edge[buf]"]:
        return "buf"
    return "unpaired"


def _branch_inputs(k, N, E, P, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    rows = P if P is not None else E
    r = lambda *s: torch.randn(*s, generator=g, dtype=dtype)  # noqa: E731
    return dict(x=r(N, k.dim_in1), y=r(E, k.dim_in2), w=r(rows, k.weight_numel), go=r(N, k.dim_out),
                cx=r(N, k.dim_in1), cy=r(E, k.dim_in2), cw=r(rows, k.weight_numel))


def _run_matrix(tps, inp, ref, dst, src, topo, pr, tol, tag, calls=None, check=None, grad_out_cases=(True, False)):
    """Every (operands requiring grad) x (cotangents) x (grad_out requiring grad) case through the module, first and
    second derivatives against the oracle terms; ``check(R, C, need_g, first_calls, second_calls)`` sees each case's
    kernel calls."""
    out_ref, grads_ref, T = ref
    device = topo.by_dst[0].device
    d = lambda t: t.to(device)  # noqa: E731
    dd, sd = d(dst), d(src)
    scale_close = lambda r, got, what: _near(r, got, what, tol)  # noqa: E731
    for R in SUBSETS:
        for g_rg in grad_out_cases:
            leaves = {n: d(inp[n]).requires_grad_(n in R) for n in "xyw"}
            gor = d(inp["go"]).requires_grad_(g_rg)
            for C in (c for c in SUBSETS if set(c) <= set(R)):
                what = f"{tag} R={R} C={C} grad_out{'(rg)' if g_rg else ''}"
                if calls is not None:
                    calls.clear()
                out = tps(leaves["x"], leaves["y"], leaves["w"], dd, sd, topology=topo, pairing=pr)
                grads = torch.autograd.grad(out, [leaves[n] for n in R], gor, create_graph=True)
                first = collections.Counter(calls) if calls is not None else None
                if calls is not None:
                    calls.clear()
                scale_close(out_ref, out.detach(), f"out {what}")
                for n, gr in zip(R, grads):
                    scale_close(grads_ref["xyw".index(n)], gr.detach(), f"first-order d{n} {what}")
                scalar = sum((grads[R.index(n)] * d(inp["c" + n])).sum() for n in C)
                targets = (["g"] if g_rg else []) + [n for n in "xyw" if n in R]
                tens = [gor if t == "g" else leaves[t] for t in targets]
                # (R = C = "x" without grad_out: grad_x = Bx(y, w, g) depends on nothing that requires grad)
                sec = (torch.autograd.grad(scalar, tens, allow_unused=True) if scalar.requires_grad
                       else (None,) * len(tens))
                for t, s, ten in zip(targets, sec, tens):
                    want = _sum_terms(T, C, t)
                    got = torch.zeros_like(ten) if s is None else s
                    scale_close(want, got.detach(), f"second-order d{t} {what}")
                if check is not None:
                    check(R, C, g_rg, first, collections.Counter(calls))


def _branch_case(case, device):
    name, mul, dtype, paired = BRANCH_CASES[case]
    from nequip_amd.model.nequip_models import torch_default_dtype
    from nequip_amd.nn._topology import EdgeTopology

    _, f_in_1x, lmax, f_out_1x = BY_NAME[name]
    with torch_default_dtype(dtype):
        tps, f_in, e_at, mid_s, instructions = _module(f_in_1x, lmax, f_out_1x, mul, device)
    k = tps._get_kernels()
    dst, src = _graph(19, seed=31 + mul, symmetric=paired)
    N, E = 19, dst.numel()
    topo = EdgeTopology(dst.to(device), src.to(device), N)
    pr = topo.pairing(None) if paired else None
    assert (pr is not None) == paired
    P = pr.num_pairs if paired else None
    inp = _branch_inputs(k, N, E, P, dtype, seed=5 + mul)
    if paired:
        wrow = pr.rows.long().cpu() % P
        w_e, cw_e = inp["w"][wrow], inp["cw"][wrow]
    else:
        w_e, cw_e = inp["w"], inp["cw"]
    out, grads, T = _oracle((f_in, e_at, mid_s, instructions), inp["x"], inp["y"], w_e, inp["go"],
                            (inp["cx"], inp["cy"], cw_e), dst, src)
    if paired:  # to the pair rows: d/dw of the gathered weights sums both edges of a pair
        grads[2] = _fold(grads[2], wrow, P)
        for t in T:
            t[3] = _fold(t[3], wrow, P)
    return tps, k, dst, src, topo, pr, inp, (out, grads, T)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", SWITCHES)
@pytest.mark.parametrize("case", list(BRANCH_CASES))
def test_second_order_branch_matrix_vs_oracle(device, case, switch, monkeypatch):
    name, mul, dtype, paired = BRANCH_CASES[case]
    for s in SWITCHES[1:]:
        monkeypatch.setenv(s, "1" if s == switch else "0")
    tps, k, dst, src, topo, pr, inp, ref = _branch_case(case, device)
    f32 = dtype == torch.float32
    # what each case must be able to reach: the test fails (never skips) if a category becomes unreachable
    if case == "dual_pair_kernel":
        assert k.has_dual_pairs_kernel(torch.float32), f"{name} lost its dual pair kernel"
    elif case == "split_pair_kernel":
        assert k.has_pairs_kernel(torch.float32) and not k.has_dual_pairs_kernel(torch.float32), \
            f"{name} is no longer a split-pair-kernel structure"
    elif case == "no_pair_kernel":
        assert not k.has_pairs_kernel(torch.float32), f"{name} has a pair kernel now: pick a structure without one"
    elif case == "f64_unpaired":
        assert not k.has_spec(torch.float64)
    if f32:
        assert k.has_spec(torch.float32) and k.has_fwd_jvp(torch.float32) and k.prefer_fused_bwd
    use_pairs = paired and k.has_pairs_kernel(dtype) and switch != "NQA_NO_PAIR_BWD"
    seen_first, seen_second = set(), set()

    def check(R, C, g_rg, first, second):
        where = f"{case} {switch} R={R} C={C} grad_out rg={g_rg}: first {dict(first)} second {dict(second)}"
        # first pass
        fb = _first_pass_branch(first)
        fused = R == "xyw" and k.prefer_fused_bwd and switch != "NQA_NO_FUSED_BWD"
        want = ("fused_pairs" if fused and use_pairs else
                "fused_rows" if fused and f32 and k.fused_rows_ok else "separate")
        assert fb == want, where
        seen_first.add(fb)
        # second pass.  autograd hands the Function a zero cotangent for each gradient it produced that the scalar does
        # not use, so the branches see a cotangent for every operand in R; C only decides which of them are zero.
        jvp = f32 and switch != "NQA_NO_FWD_JVP"
        assert second["fwd_jvp"] == int(jvp and g_rg and len(R) > 1), where
        assert second["bwd_x_dual"] == int(jvp and R == "xyw"), where
        if R == "xyw":  # the edge gradients
            sb = _second_pass_branch(second)
            if pr is None:
                want = "unpaired"
            elif use_pairs:
                want = "dual" if (k.has_dual_pairs_kernel(dtype) and switch != "NQA_NO_DUAL_PAIR_BWD") else "pairs"
            else:
                want = "buf"
            assert sb == want, where
            seen_second.add(sb)
        else:
            assert not second["edge_grads_dual"] and not second["bwd_edge[buf]"], where

    calls = _count_calls(monkeypatch)
    tol = None if f32 else TOL64
    _run_matrix(tps, inp, ref, dst, src, topo, pr, tol, f"{case} {switch}", calls=calls, check=check)
    expect_first, expect_second = BRANCH_EXPECT[case]
    if switch == "NQA_NO_FUSED_BWD":
        expect_first = "separate"
    elif switch == "NQA_NO_PAIR_BWD" and expect_first == "fused_pairs":
        expect_first = "fused_rows"
    if switch == "NQA_NO_PAIR_BWD" and paired:
        expect_second = "buf"
    elif switch == "NQA_NO_DUAL_PAIR_BWD" and expect_second == "dual":
        expect_second = "pairs"
    assert seen_first == {expect_first, "separate"}, (seen_first, expect_first)
    assert seen_second == {expect_second}, (seen_second, expect_second)


# ---- 3. the dispatcher-op form on a structure-specialised plan -------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wpn", [1, 4])
@pytest.mark.parametrize("mul", [64, 128])
def test_dispatcher_form_second_order_vs_oracle(device, mul, wpn, monkeypatch):
    from nequip_amd.nn import TensorProductScatter
    from nequip_amd.nn._topology import EdgeTopology
    from nequip_amd.o3 import Irreps

    monkeypatch.setenv("NQA_SPEC_WPN", str(wpn))
    name = "l2n_mid"
    _, f_in_1x, lmax, f_out_1x = BY_NAME[name]
    tps0, f_in, e_at, mid_s, instructions = _module(f_in_1x, lmax, f_out_1x, mul, device)
    assert tps0._get_kernels().has_spec(torch.float32)
    tps = TensorProductScatter(Irreps(f_in), Irreps(e_at), Irreps(mid_s), instructions,
                               use_dispatcher_ops=True).to(device)
    dst, src = _graph(19, seed=53 + mul, symmetric=False)
    N, E = 19, dst.numel()
    topo = EdgeTopology(dst.to(device), src.to(device), N)
    inp = _branch_inputs(tps0._get_kernels(), N, E, None, torch.float32, seed=9 + mul)
    ref = _oracle((f_in, e_at, mid_s, instructions), inp["x"], inp["y"], inp["w"], inp["go"],
                  (inp["cx"], inp["cy"], inp["cw"]), dst, src)
    from nequip_amd.nn import _tp_scatter_base

    with _no_function_form(monkeypatch, _tp_scatter_base):
        _run_matrix(tps, inp, ref, dst, src, topo, None, None, f"dispatcher {name} mul={mul} wpn={wpn}",
                    grad_out_cases=(True,))


@contextlib.contextmanager
def _no_function_form(monkeypatch, base):
    """The autograd Functions of the eager form must not run: the dispatcher-op form is what is under test."""
    def refuse(*a, **kw):
        raise AssertionError("the function form ran instead of the dispatcher ops")

    with monkeypatch.context() as m:
        m.setattr(base._TPScatterFn, "apply", refuse)
        m.setattr(base._TPScatterBwdFn, "apply", refuse)
        yield


# ---- 4. a force-matching training step of an XL-shaped model ---------------------------------------------------------
@pytest.mark.gpu
def test_xl_shaped_training_step_parameter_gradients(device, monkeypatch):
    """Preset XL's channel counts (320 / 96 / 64 / 32 / 32, l_max = 4: segments of 224 and 32 channels) with three
    layers on a small frame: force-matching parameter gradients against autograd-through-autograd of the oracle, at
    both launch shapes of the structure-specialised kernels."""
    from nequip_amd.data import AtomicDataDict
    from nequip_amd.model import NequIPGNNModel
    from nequip_amd.utils import synthetic as syn
    from oracle import model as omodel

    pos, types, cell, names = syn.water_box(n_side=2, seed=7)
    data = syn.make_data(pos, types, 4.0, cell)
    n, e = len(pos), data["edge_index"].shape[1]
    cfg = dict(r_max=4.0, num_layers=3, l_max=PRESETS["XL"]["l_max"], parity=False,
               num_features=list(PRESETS["XL"]["num_features"]), type_embed_num_features=32, radial_mlp_depth=1,
               radial_mlp_width=64, num_bessels=8, polynomial_cutoff_p=6, avg_num_neighbors=e / n,
               model_dtype="float32")
    model = NequIPGNNModel(seed=5, model_dtype="float32", type_names=names,
                           **{k: v for k, v in cfg.items() if k != "model_dtype"})
    gen = torch.Generator().manual_seed(0)
    f_t = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    e_t = torch.randn(1, 1, generator=gen, dtype=torch.float64)
    pn = {k for k, _ in model.named_parameters()}
    weights = {k.replace("model.func.", ""): v.detach().clone().requires_grad_(k in pn)
               for k, v in model.state_dict().items()}
    out = omodel.energy_forces(data, cfg, weights, create_graph=True)
    loss_ref = (out["forces"] - f_t).square().mean() + (out["total_energy"] - e_t).square().mean() / n
    names_w = [k for k, v in weights.items() if v.requires_grad]
    grads_ref = dict(zip(names_w, torch.autograd.grad(loss_ref, [weights[k] for k in names_w])))
    model = model.to(device).train()
    for wpn in (4, 1):
        monkeypatch.setenv("NQA_SPEC_WPN", str(wpn))
        model.zero_grad(set_to_none=True)
        out = model(AtomicDataDict.to_device(data, device))
        loss = (out["forces"] - f_t.to(device)).square().mean() + \
            (out["total_energy"] - e_t.to(device)).square().mean() / n
        loss.backward()
        torch.testing.assert_close(loss_ref.detach(), loss.detach().cpu(), atol=2e-4, rtol=2e-4)
        for k, p in model.named_parameters():
            r = grads_ref[k.replace("model.func.", "")]
            assert p.grad is not None, k
            torch.testing.assert_close(r, p.grad.cpu(), atol=2e-4 * max(1e-3, float(r.abs().max())), rtol=2e-3,
                                       msg=lambda m: f"wpn={wpn} {k}: {m}")
