"""The any-irreps tensor-product kernels (``nequip_amd/csrc/tp_generic.hip``), entry point by entry point, against the
float64 restatement of ``tests/tp_generic_cases.py`` on its named cases: every ``CGT<l1, l2, l3>`` with l <= 4, one to three
64-channel chunks with full and partial last chunks, output slots shared by 2 and 3 instructions with path weights, blocks
and attribute columns that no instruction touches, the ``ir_mul`` layout on either side, and empty graphs.

Every element is held to ``(terms + 6) u M`` (derivation: the docstring of ``tp_generic_cases``); elements without terms
must be exactly zero.  float32 reaches the generic kernels through plans that have no structure-specialised kernel
(asserted per case), float64 always does.  Every check prints its largest ``error / bound`` (``pytest -s``).

Largest ``error / bound`` measured on an MI355X, float32 / float64: ``fwd`` 0.43 / 0.30, ``bwd_x`` 0.45 / 0.30, ``bwd_edge``
grad_w 0.43 / 0.26, ``bwd_edge`` grad_y 0.27 / 0.24 (the same with one or both gradients asked for), through
``TensorProductScatter`` in either form 0.43 / 0.24.  The file's 866 tests take 5 s together; the slowest, the first
``test_autograd`` (it loads the module and the dispatcher ops), 1 s.
"""

import functools

import pytest
import torch

import tp_generic_cases as tc
from oracle import tp as otp

pytestmark = pytest.mark.gpu

PARAMS = [pytest.param(n, dt, id=f"{n}-{str(dt).split('.')[-1]}") for n, dt in tc.case_dtype_params()]
REPEAT = [p for p in PARAMS if p.values[0] in tc.CHUNK_CASES + tc.CHUNK_UNIFORM_CASES + tc.SHARED_CASES]
ZEROS = [p for p in PARAMS if "shared" in p.values[0]]
AUTOGRAD_CASES = ("shared-m5", "shared-m65", "chunks-m65")


@functools.lru_cache(maxsize=None)
def _setup(name, dtype, device):
    """(kernels, topology, (x, y, w, g) on the device in the layouts of the case's plan, the case)."""
    from nequip_amd.nn._tp_scatter_base import _Kernels
    from nequip_amd.nn._topology import EdgeTopology

    case = tc.make_case(name)
    plan = tc.native_plan(case)
    k = _Kernels(plan, plan.image.to(device))
    if dtype == torch.float32:
        assert not k.has_spec(torch.float32), f"{name}: float32 would not run the generic kernels"
    assert not k.has_spec(torch.float64)
    topo = EdgeTopology(case.dst.to(device), case.src.to(device), case.num_nodes)
    x, y, w, g = tc.inputs(case, dtype)
    x, g = tc.in_layout(x, case.plan.in1, case.layout_in1), tc.in_layout(g, case.plan.out, case.layout_out)
    return k, topo, tuple(t.to(dtype).to(device).contiguous() for t in (x, y, w, g)), case


def _rows(t, irreps, layout):
    """Node rows that a kernel wrote, in mul_ir columns."""
    t = t.detach().cpu()
    return tc.to_mul_ir(t, irreps) if layout == tc.IR_MUL else t


def _check(entry, got, name, dtype, key):
    r = tc.check(got, tc.reference(name, dtype)[key], dtype, f"{name} {entry} {key}")
    print(f"ratio {entry}:{key} {str(dtype).split('.')[-1]} {name} {r:.4f}")
    return r


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_fwd(device, name, dtype):
    k, topo, (x, y, w, g), case = _setup(name, dtype, device)
    out = k.fwd(x, y, w, topo)
    _check("fwd", _rows(out, case.plan.out, case.layout_out), name, dtype, "out")


@pytest.mark.parametrize("name,dtype", PARAMS)
def test_bwd_x(device, name, dtype):
    k, topo, (x, y, w, g), case = _setup(name, dtype, device)
    gx = k.bwd_x(y, w, g, topo)
    _check("bwd_x", _rows(gx, case.plan.in1, case.layout_in1), name, dtype, "gx")


@pytest.mark.parametrize("need_gw,need_gy", [(True, True), (True, False), (False, True)], ids=["gw+gy", "gw", "gy"])
@pytest.mark.parametrize("name,dtype", PARAMS)
def test_bwd_edge(device, name, dtype, need_gw, need_gy):
    k, topo, (x, y, w, g), case = _setup(name, dtype, device)
    gw, gy = k.bwd_edge(x, y, w, g, topo, need_gw=need_gw, need_gy=need_gy)
    assert (gw is not None) == need_gw and (gy is not None) == need_gy
    entry = "bwd_edge(" + "+".join(n for n, on in (("gw", need_gw), ("gy", need_gy)) if on) + ")"
    if need_gw:
        _check(entry, gw, name, dtype, "gw")
    if need_gy:
        _check(entry, gy, name, dtype, "gy")


@pytest.mark.parametrize("name,dtype", ZEROS)
def test_exact_zeros(device, name, dtype):
    """The regions of the ``shared`` plan that no term reaches are there, and the kernels leave exact zeros in them."""
    k, topo, (x, y, w, g), case = _setup(name, dtype, device)
    m = case.plan.in1[0][0]
    out = _rows(k.fwd(x, y, w, topo), case.plan.out, case.layout_out)
    gx = _rows(k.bwd_x(y, w, g, topo), case.plan.in1, case.layout_in1)
    _, gy = k.bwd_edge(x, y, w, g, topo, need_gw=False, need_gy=True)
    ref = tc.reference(name, dtype)
    unwritten, unread, unused = slice(9 * m, 14 * m), slice(4 * m, 7 * m), slice(1, 7)  # 2o of out, 1e of in1, 2x1o of in2
    assert int(ref["out"].terms[:, unwritten].sum()) == 0 and bool((out[:, unwritten] == 0).all())
    assert int(ref["gx"].terms[:, unread].sum()) == 0 and bool((gx[:, unread] == 0).all())
    assert int(ref["gy"].terms[:, unused].sum()) == 0 and bool((gy.cpu()[:, unused] == 0).all())
    if case.num_edges:
        no_in = torch.bincount(case.dst, minlength=case.num_nodes) == 0
        no_out = torch.bincount(case.src, minlength=case.num_nodes) == 0
        assert bool(no_in.any()) and bool(no_out.any())
        assert bool((out[no_in] == 0).all()) and bool((gx[no_out] == 0).all())
        assert bool((out[~no_in][:, :9 * m] != 0).all()) and bool((gy.cpu()[:, [0, 7]] != 0).all())


@pytest.mark.parametrize("name,dtype", REPEAT)
def test_fwd_twice(device, name, dtype):
    """Own slots: an ordered register sum and one store, the same bits on every call.  Shared slots: atomics, both calls
    within the bound."""
    k, topo, (x, y, w, g), case = _setup(name, dtype, device)
    a, b = k.fwd(x, y, w, topo), k.fwd(x, y, w, topo)
    for out in (a, b):
        _check("fwd", _rows(out, case.plan.out, case.layout_out), name, dtype, "out")
    if not k.out_needs_zero:
        assert torch.equal(a, b)


def _module(case, dtype, device, dispatcher):
    from nequip_amd.model.nequip_models import torch_default_dtype
    from nequip_amd.nn import TensorProductScatter
    from nequip_amd.o3 import Irreps

    f_in, e_at, mid = case.plan.strings()
    with torch_default_dtype(dtype):
        return TensorProductScatter(Irreps(f_in), Irreps(e_at), Irreps(mid), [tuple(i) for i in case.plan.instructions],
                                    use_dispatcher_ops=dispatcher).to(device)


@functools.lru_cache(maxsize=None)
def _oracle_second_order(name, dtype):
    """The second-order gradients of ``test_tp_scatter_double_backward`` through ``oracle.tp.tp_scatter``, on the CPU."""
    case = tc.make_case(name)
    x, y, w, g = (t.to(dtype) for t in tc.inputs(case, dtype))
    f_in, e_at, mid = case.plan.strings()
    ins = [tuple(i) for i in case.plan.instructions]
    gen = torch.Generator().manual_seed(99)
    cs = tuple(torch.randn(t.shape, generator=gen, dtype=dtype) for t in (x, y, w))
    fn = lambda a, b, c: otp.tp_scatter(a, b, c, case.dst, case.src, f_in, e_at, mid, ins)  # noqa: E731
    return cs, _second_order(fn, (x, y, w), g, cs, lambda t: t)


def _second_order(fn, tensors, go, cs, to):
    xs = [to(t).clone().requires_grad_(True) for t in tensors]
    gout = to(go).clone().requires_grad_(True)
    out = fn(*xs)
    grads = torch.autograd.grad(out, xs, gout, create_graph=True)
    scalar = sum((gr * to(c)).sum() for gr, c in zip(grads, cs))
    return torch.autograd.grad(scalar, xs + [gout], allow_unused=True)


@pytest.mark.parametrize("dispatcher", [False, True], ids=["direct", "dispatcher"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("name", AUTOGRAD_CASES)
def test_autograd(device, name, dtype, dispatcher):
    """``TensorProductScatter`` on the same cases: first order against the restatement, second order against autograd
    through the oracle at the tolerances of ``test_tp_scatter_double_backward``."""
    case = tc.make_case(name)
    tps = _module(case, dtype, device, dispatcher)
    dev = lambda t: t.to(device)  # noqa: E731
    x, y, w, g = (t.to(dtype) for t in tc.inputs(case, dtype))
    dst, src = dev(case.dst), dev(case.src)
    xs = [dev(t).requires_grad_(True) for t in (x, y, w)]
    out = tps(*xs, dst, src)
    gx, gy, gw = torch.autograd.grad(out, xs, dev(g))
    form = "dispatcher" if dispatcher else "direct"
    for key, got in (("out", out), ("gx", gx), ("gy", gy), ("gw", gw)):
        _check(f"autograd-{form}", got, name, dtype, key)

    tol = {torch.float32: 2e-5, torch.float64: 1e-10}[dtype]
    cs, ref = _oracle_second_order(name, dtype)
    got = _second_order(lambda a, b, c: tps(a, b, c, dst, src), (x, y, w), g, cs, dev)
    for r, k in zip(ref, got):
        assert (r is None) == (k is None)
        if r is None:
            continue
        torch.testing.assert_close(r, k.cpu(), atol=tol * max(1.0, float(r.abs().max())), rtol=tol)
