"""Named cases and a float64 restatement for the any-irreps tensor-product kernels (``nequip_amd/csrc/tp_generic.hip``:
``tp_fwd_kernel``, ``tp_bwd_edge_kernel`` + ``tp_ypart_reduce_kernel``, ``tp_bwd_x_kernel``).  No GPU in this module.

The operation (``oracle/tp.py``, e3nn ``'uvu'`` with per-edge weights), for instruction ``p = (i1, i2, io, path_weight)``
with ``C = wigner_3j(l1, l2, l3)`` and ``c_p = sqrt((2 l3 + 1) / n_into[io] * path_weight)``::

    out[n, io, u, k] = sum_{e: dst[e] = n} sum_p c_p w[e, p, u] sum_ij C_ijk x[src[e], i1, u, i] y[e, i2, j]
    gx[s, i1, u, i]  = sum_{e: src[e] = s} sum_p c_p w[e, p, u] sum_jk C_ijk y[e, i2, j] g[dst[e], io, u, k]
    gw[e, p, u]      =                          c_p          sum_ijk C_ijk x[src[e], i1, u, i] y[e, i2, j] g[dst[e], io, u, k]
    gy[e, i2, j]     = sum_p sum_u              c_p w[e, p, u] sum_ik C_ijk x[src[e], i1, u, i] g[dst[e], io, u, k]

``reference`` evaluates the four in float64 on ``oracle.wigner.wigner_3j`` (not on the table the kernels' literals are
generated from) and returns, for every element, the value, the magnitude sum ``M`` of its terms (the same sums over the
absolute values of every factor) and ``terms``, the number of elementary products ``c_p w C_ijk x y`` summed into it (only
non-zero ``C_ijk`` count: the generated contraction has no statement for the others).

The bound.  Every element is held to::

    |got - ref| <= (terms + 6) u M        u = 2^-24 (float32), 2^-53 (float64)

A term is the product of five factors.  In the kernels it passes through at most four rounded multiplications
(``a * b``, ``C * p``, ``w * t``, ``c * acc`` in the forward; ``c * g`` / ``c * w`` take the place of the last one in the
adjoints) and the two constants ``C_ijk`` and ``c_p`` are each rounded once to the element type: six roundings.  The sum of
``terms`` values takes ``terms - 1`` additions when it is one chain; the register accumulation over a node's edges is that
chain, and the tree of ``wave_sum``, the partial columns of the grad_y reduction and the atomics of a shared output slot
only make the longest path through the additions shorter.  With ``(1 + u)^n - 1 <= n u / (1 - n u)`` and ``n u < 1e-4``
at the sizes used here the first-order form stands (the ``+ 6`` in place of ``+ 5`` absorbs the second-order remainder many
times over).  Inputs are rounded to the element type BEFORE the reference is evaluated, so no input rounding enters.

The reference is itself a float64 evaluation with the same count of roundings; its own error is below ``(terms + 6) 2^-53 M``
and is not added.  For float32 it is 2^-29 of the bound.  For float64 the worst cases of the two sides would add up to
twice the bound; it is kept as stated all the same, because that worst case needs every one of the ``terms + 5`` roundings
of a chain to fall in one direction on one side and in the other direction on the other (the ratios measured on the GPU
are in the docstring of ``test_tp_generic_kernels_gpu.py``: below one half in both element types).

float64 only: the kernels' literals come from ``nequip_amd.o3.wigner`` (exact rationals, printed with 17 digits), the
reference's from ``oracle.wigner`` (float Racah sums).  Their disagreement ``|dC_ijk| <= WIGNER_AGREEMENT * max|C|`` (asserted
on the CPU, ``test_tp_generic_cases.py::test_wigner_tables_agree``) moves a term by at most ``WIGNER_AGREEMENT * max|C| *
|c_p w x y|``, so the float64 bound adds ``WIGNER_AGREEMENT * Mc`` with ``Mc`` the magnitude sum taken with ``max|C|`` of the
triple in place of every non-zero ``|C_ijk|``.

Elements with ``terms == 0`` (unwritten output blocks, rows of nodes without edges, the gradient of an input block or an
edge-attribute column that no instruction reads) must be exactly zero.

Layouts: node rows are ``mul_ir`` here (column ``off + u (2l + 1) + i``); ``to_ir_mul`` / ``to_mul_ir`` permute the columns of
node rows to and from ``ir_mul`` (column ``off + i mul + u``).  The reference of an ``ir_mul`` plan is the ``mul_ir`` one with
permuted columns.
"""

import functools
import math
from typing import NamedTuple, Tuple

import torch

from oracle import irreps as oir
from oracle import tp as otp
from oracle.wigner import wigner_3j

U = {torch.float32: 2.0 ** -24, torch.float64: 2.0 ** -53}
WIGNER_AGREEMENT = 8 * 2.0 ** -53  # of the two Wigner tables, relative to max|C| of a triple
STRUCTURAL_ZERO = 1e-12  # |C_ijk| below this is a zero of the selection rules (the smallest coefficient for l <= 4 is > 1e-2)
MUL_IR, IR_MUL = 0, 1
LMAX = 4


# ---- tables ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(l1, l2, l3):
    """``oracle.wigner.wigner_3j`` with the float noise in its structural zeros removed."""
    C = wigner_3j(l1, l2, l3).clone()
    C[C.abs() < STRUCTURAL_ZERO] = 0.0
    return C


def path_coeff(l3, n_into, path_weight):
    return math.sqrt((2 * l3 + 1) / n_into * path_weight)


TRIPLES = tuple((l1, l2, l3) for l1 in range(LMAX + 1) for l2 in range(LMAX + 1)
                for l3 in range(abs(l1 - l2), min(l1 + l2, LMAX) + 1))


# ---- plans -------------------------------------------------------------------------------------------------------------
class Plan(NamedTuple):
    in1: Tuple[Tuple[int, int, int], ...]  # (mul, l, p) per block, as oracle.irreps
    in2: Tuple[Tuple[int, int, int], ...]
    out: Tuple[Tuple[int, int, int], ...]
    instructions: Tuple[tuple, ...]  # (i1, i2, io, "uvu", True, path_weight)
    uniform: bool = False  # a NequIP structure at one multiplicity: float32 has a specialised kernel, run float64 only

    @property
    def dims(self):
        return oir.dim(self.in1), oir.dim(self.in2), oir.dim(self.out)

    @property
    def weight_numel(self):
        return sum(self.in1[ins[0]][0] for ins in self.instructions)

    def strings(self):
        return oir.to_str(self.in1), oir.to_str(self.in2), oir.to_str(self.out)


def _six(instructions):
    return tuple(tuple(ins) + ((1.0,) if len(ins) == 5 else ()) for ins in instructions)


def built_plan(f_in, e_at, f_out, uniform=False):
    """The instruction list of a convolution as InteractionBlock builds it: every instruction has its own output slot."""
    mid, instructions = otp.build_instructions(f_in, e_at, f_out)
    return Plan(tuple(oir.parse(f_in)), tuple(oir.parse(e_at)), tuple(mid), _six(instructions), uniform)


def _p(l):
    return 1 if l % 2 == 0 else -1


def triple_plan(l1, l2, l3, mul=3):
    p1, p2 = _p(l1), _p(l2)
    return Plan(((mul, l1, p1),), ((1, l2, p2),), ((mul, l3, p1 * p2),), ((0, 0, 0, "uvu", True, 1.0),))


def chunks_plan(m):
    """Two multiplicities: no structure-specialised kernel, float32 runs the generic ones."""
    return built_plan(f"{m}x0e + {m}x1o + 7x2e", "0e + 1o + 2e", "0e + 1o + 2e")


def chunks_uniform_plan(m):
    """The ``l2n_mid`` structure (a middle layer at l_max = 2 without parity)."""
    return built_plan(f"{m}x0e + {m}x1o + {m}x2e", "0e + 1o + 2e", "0e + 1o + 2e", uniform=True)


def shared_plan(m):
    """Output slots written by 2 (0e), 1 (1o) and 3 (2e) instructions, path weights 0.5 / 1 / 2, the input block 1e that no
    instruction reads, the output block 2o that none writes, the attribute 2x1o that none uses."""
    in1 = ((m, 0, 1), (m, 1, -1), (m, 1, 1), (m, 2, 1))
    in2 = ((1, 0, 1), (2, 1, -1), (1, 2, 1))
    out = ((m, 0, 1), (m, 1, -1), (m, 2, 1), (m, 2, -1))
    ins = ((0, 2, 2, "uvu", True, 2.0),   # 0e x 2e -> 2e
           (0, 0, 0, "uvu", True, 0.5),   # 0e x 0e -> 0e
           (3, 0, 2, "uvu", True, 1.0),   # 2e x 0e -> 2e
           (1, 2, 1, "uvu", True, 1.0),   # 1o x 2e -> 1o   (its own slot, next to shared ones)
           (3, 2, 0, "uvu", True, 2.0),   # 2e x 2e -> 0e
           (3, 2, 2, "uvu", True, 0.5))   # 2e x 2e -> 2e
    return Plan(in1, in2, out, ins)


# ---- graphs ------------------------------------------------------------------------------------------------------------
def _shuffled(dst, src, seed):
    perm = torch.randperm(len(dst), generator=torch.Generator().manual_seed(seed))
    return torch.tensor(dst, dtype=torch.int64)[perm].contiguous(), torch.tensor(src, dtype=torch.int64)[perm].contiguous()


def small_graph():
    """5 nodes, 12 edges; in-degrees (0, 3, 3, 3, 3), out-degrees (1, 2, 3, 3, 3)."""
    dst = [1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4]
    src = [2, 3, 4, 0, 3, 4, 1, 2, 4, 1, 2, 3]
    return 5, _shuffled(dst, src, 11)


def degree_graph():
    """7 nodes, 49 edges in shuffled order.  In-degrees (0, 1, 2, 37, 3, 2, 4); node 5 is no edge's source; 0 -> 2 twice and
    every source of node 3 several times (repeated edges); 3 -> 3 and 4 -> 4 (self loops)."""
    dst, src = [], []
    for i in range(37):
        dst.append(3), src.append([0, 1, 2, 3, 4, 6][i % 6])
    for d, ss in ((1, [6]), (2, [0, 0]), (4, [4, 1, 2]), (5, [3, 6]), (6, [0, 1, 2, 4])):
        for s in ss:
            dst.append(d), src.append(s)
    return 7, _shuffled(dst, src, 12)


# ---- cases -------------------------------------------------------------------------------------------------------------
class Case(NamedTuple):
    name: str
    plan: Plan
    num_nodes: int
    dst: torch.Tensor
    src: torch.Tensor
    x: torch.Tensor  # float64, mul_ir; rounded to the element type by `inputs`
    y: torch.Tensor
    w: torch.Tensor
    g: torch.Tensor
    layout_in1: int = MUL_IR
    layout_out: int = MUL_IR

    @property
    def num_edges(self):
        return int(self.dst.numel())


def _case(name, plan, num_nodes, edges, seed, layout_in1=MUL_IR, layout_out=MUL_IR):
    dst, src = edges
    E = int(dst.numel())
    d1, d2, do = plan.dims
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(num_nodes, d1, generator=gen, dtype=torch.float64)
    y = torch.randn(E, d2, generator=gen, dtype=torch.float64)
    w = torch.randn(E, plan.weight_numel, generator=gen, dtype=torch.float64) / 4
    g = torch.randn(num_nodes, do, generator=gen, dtype=torch.float64)
    return Case(name, plan, num_nodes, dst, src, x, y, w, g, layout_in1, layout_out)


CHUNK_MULS = (1, 63, 64, 65, 130)
SHARED_MULS = (5, 65)
LAYOUT_FORMS = {"in": (IR_MUL, MUL_IR), "out": (MUL_IR, IR_MUL), "both": (IR_MUL, IR_MUL)}
_NO_EDGES = (torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64))

_BUILDERS = {}
for _i, (_l1, _l2, _l3) in enumerate(TRIPLES):
    _BUILDERS[f"triples-{_l1}{_l2}{_l3}"] = functools.partial(
        lambda n, t, s: _case(n, triple_plan(*t), small_graph()[0], small_graph()[1], s), f"triples-{_l1}{_l2}{_l3}",
        (_l1, _l2, _l3), 1000 + _i)
for _m in CHUNK_MULS:
    _BUILDERS[f"chunks-m{_m}"] = functools.partial(
        lambda n, m: _case(n, chunks_plan(m), degree_graph()[0], degree_graph()[1], 2000 + m), f"chunks-m{_m}", _m)
    _BUILDERS[f"chunks-uniform-m{_m}"] = functools.partial(
        lambda n, m: _case(n, chunks_uniform_plan(m), degree_graph()[0], degree_graph()[1], 3000 + m),
        f"chunks-uniform-m{_m}", _m)
for _m in SHARED_MULS:
    _BUILDERS[f"shared-m{_m}"] = functools.partial(
        lambda n, m: _case(n, shared_plan(m), degree_graph()[0], degree_graph()[1], 4000 + m), f"shared-m{_m}", _m)
for _form, (_li, _lo) in LAYOUT_FORMS.items():
    _BUILDERS[f"layouts-chunks-m65-{_form}"] = functools.partial(
        lambda n, li, lo: _case(n, chunks_plan(65), degree_graph()[0], degree_graph()[1], 5000 + 2 * li + lo, li, lo),
        f"layouts-chunks-m65-{_form}", _li, _lo)
    _BUILDERS[f"layouts-shared-m5-{_form}"] = functools.partial(
        lambda n, li, lo: _case(n, shared_plan(5), degree_graph()[0], degree_graph()[1], 6000 + 2 * li + lo, li, lo),
        f"layouts-shared-m5-{_form}", _li, _lo)
_BUILDERS["empty-edges"] = lambda: _case("empty-edges", shared_plan(5), 4, _NO_EDGES, 7000)
_BUILDERS["empty-nodes"] = lambda: _case("empty-nodes", shared_plan(5), 0, _NO_EDGES, 7001)

TRIPLE_CASES = tuple(n for n in _BUILDERS if n.startswith("triples-"))
CHUNK_CASES = tuple(f"chunks-m{m}" for m in CHUNK_MULS)
CHUNK_UNIFORM_CASES = tuple(f"chunks-uniform-m{m}" for m in CHUNK_MULS)
SHARED_CASES = tuple(f"shared-m{m}" for m in SHARED_MULS)
LAYOUT_CASES = tuple(n for n in _BUILDERS if n.startswith("layouts-"))
EMPTY_CASES = ("empty-edges", "empty-nodes")
ALL_CASES = tuple(_BUILDERS)
MUL_IR_CASES = tuple(n for n in ALL_CASES if n not in LAYOUT_CASES)


@functools.lru_cache(maxsize=None)
def make_case(name) -> Case:
    return _BUILDERS[name]()


def dtypes_of(name):
    """Uniform plans have a structure-specialised float32 kernel: the generic kernels run them in float64 only."""
    return (torch.float64,) if make_case(name).plan.uniform else (torch.float32, torch.float64)


def case_dtype_params():
    return [(n, dt) for n in ALL_CASES for dt in dtypes_of(n)]


def inputs(case, dtype):
    """(x, y, w, g) rounded to ``dtype`` and back to float64: what the kernels are given, exactly."""
    return tuple(t.to(dtype).to(torch.float64) for t in (case.x, case.y, case.w, case.g))


# ---- the restatement ---------------------------------------------------------------------------------------------------
def evaluate(plan, x, y, w, g, dst, src, tables=table, coeff=path_coeff):
    """``(out, gx, gy, gw)`` of one plan in the dtype of ``x`` (mul_ir).  ``tables(l1, l2, l3)`` gives ``C``, ``coeff(l3,
    n_into, path_weight)`` gives ``c_p``: the values, the magnitude sums and the term counts are this one function."""
    N, E = x.shape[0], y.shape[0]
    s1, s2, so = oir.slices(plan.in1), oir.slices(plan.in2), oir.slices(plan.out)
    n_into = [0] * len(plan.out)
    for i1, i2, io, *_ in plan.instructions:
        n_into[io] += plan.in2[i2][0]
    d_in1, d_in2, d_out = plan.dims
    out = x.new_zeros(N, d_out)
    gx = x.new_zeros(N, d_in1)
    gy = x.new_zeros(E, d_in2)
    gw = x.new_zeros(E, plan.weight_numel)
    x_e, g_e = x[src], g[dst]
    woff = 0
    for i1, i2, io, _, _, pw in plan.instructions:
        mul, l1, _ = plan.in1[i1]
        mul2, l2, _ = plan.in2[i2]
        _, l3, _ = plan.out[io]
        assert mul2 == 1 and plan.out[io][0] == mul
        C = tables(l1, l2, l3).to(x.dtype)
        c = coeff(l3, n_into[io], pw)
        xe = x_e[:, s1[i1]].reshape(E, mul, 2 * l1 + 1)
        ye = y[:, s2[i2]]
        ge = g_e[:, so[io]].reshape(E, mul, 2 * l3 + 1)
        cw = (c * w[:, woff:woff + mul])[:, :, None]
        t = torch.einsum("euij,ijk->euk", xe[:, :, :, None] * ye[:, None, None, :], C)
        out[:, so[io]] += x.new_zeros(N, mul, 2 * l3 + 1).index_add_(0, dst, cw * t).reshape(N, mul * (2 * l3 + 1))
        gw[:, woff:woff + mul] = c * (t * ge).sum(-1)
        r = torch.einsum("eujk,ijk->eui", ye[:, None, :, None] * ge[:, :, None, :], C)
        gx[:, s1[i1]] += x.new_zeros(N, mul, 2 * l1 + 1).index_add_(0, src, cw * r).reshape(N, mul * (2 * l1 + 1))
        q = torch.einsum("euik,ijk->euj", xe[:, :, :, None] * ge[:, :, None, :], C)
        gy[:, s2[i2]] += (cw * q).sum(1)
        woff += mul
    assert woff == plan.weight_numel
    return out, gx, gy, gw


class Quantity(NamedTuple):
    val: torch.Tensor    # float64
    mag: torch.Tensor    # M: the sum over |c_p| |w| |C_ijk| |x| |y| (|g|)
    mag_c: torch.Tensor  # Mc: the same with max|C| of the triple in place of every non-zero |C_ijk|
    terms: torch.Tensor  # number of elementary products summed into the element

    def permuted(self, fn):
        return Quantity(*(fn(t) for t in self))


NAMES = ("out", "gx", "gy", "gw")


def restate(plan, x, y, w, g, dst, src, tables=table):
    """``{name: Quantity}`` for float64 ``(x, y, w, g)``."""
    val = evaluate(plan, x, y, w, g, dst, src, tables)
    ab = [t.abs() for t in (x, y, w, g)]
    mag = evaluate(plan, *ab, dst, src, lambda *l: tables(*l).abs())
    mag_c = evaluate(plan, *ab, dst, src, lambda *l: (tables(*l) != 0).to(torch.float64) * tables(*l).abs().max())
    ones = [torch.ones_like(t) for t in (x, y, w, g)]
    terms = evaluate(plan, *ones, dst, src, lambda *l: (tables(*l) != 0).to(torch.float64), lambda *a: 1.0)
    return {n: Quantity(*q) for n, q in zip(NAMES, zip(val, mag, mag_c, terms))}


@functools.lru_cache(maxsize=None)
def reference(name, dtype):
    """The restatement of a case on the inputs as ``dtype`` holds them, in ``mul_ir`` columns."""
    case = make_case(name)
    return restate(case.plan, *inputs(case, dtype), case.dst, case.src)


def bound(q: Quantity, dtype):
    b = (q.terms + 6) * U[dtype] * q.mag
    if dtype == torch.float64:
        b = b + WIGNER_AGREEMENT * q.mag_c
    return b


def worst(got, q: Quantity, dtype):
    """``(ratio, message)``: the largest ``|got - ref| / bound`` over the elements that have terms, and what is wrong (None
    when every element is within the bound and every element without terms is exactly zero)."""
    got = got.detach().to("cpu", torch.float64)
    if got.shape != q.val.shape:
        return float("inf"), f"shape {tuple(got.shape)}, expected {tuple(q.val.shape)}"
    if got.numel() == 0:
        return 0.0, None
    err, b = (got - q.val).abs(), bound(q, dtype)
    none = q.terms == 0
    if bool((got[none] != 0).any()):
        idx = tuple(int(i) for i in ((got != 0) & none).nonzero()[0])
        return float("inf"), f"element {idx} has no terms and must be exactly zero, got {float(got[idx])!r}"
    ratio = torch.where(none, torch.zeros_like(err), err / b.clamp_min(1e-300))
    ratio = torch.where(torch.isfinite(got), ratio, torch.full_like(ratio, float("inf")))
    r = float(ratio.max())
    if not r <= 1.0:
        idx = tuple(int(i) for i in (ratio == ratio.max()).nonzero()[0])
        return r, (f"element {idx}: got {float(got[idx])!r}, reference {float(q.val[idx])!r}, error {float(err[idx]):.3e} "
                   f"= {r:.3f} x bound {float(b[idx]):.3e} ({int(q.terms[idx])} terms)")
    return r, None


def check(got, q: Quantity, dtype, what):
    r, msg = worst(got, q, dtype)
    assert msg is None, f"{what}: {msg}"
    return r


# ---- layouts -----------------------------------------------------------------------------------------------------------
def to_ir_mul(t, irreps):
    """Columns of node rows ``[..., dim]`` from mul_ir (``off + u (2l + 1) + i``) to ir_mul (``off + i mul + u``)."""
    cols = [t[:, sl].reshape(t.shape[0], mul, 2 * l + 1).transpose(1, 2).reshape(t.shape[0], mul * (2 * l + 1))
            for sl, (mul, l, _) in zip(oir.slices(irreps), irreps)]
    return torch.cat(cols, dim=1).contiguous() if cols else t.clone()


def to_mul_ir(t, irreps):
    cols = [t[:, sl].reshape(t.shape[0], 2 * l + 1, mul).transpose(1, 2).reshape(t.shape[0], mul * (2 * l + 1))
            for sl, (mul, l, _) in zip(oir.slices(irreps), irreps)]
    return torch.cat(cols, dim=1).contiguous() if cols else t.clone()


def in_layout(t, irreps, layout):
    return to_ir_mul(t, irreps) if layout == IR_MUL else t


# ---- the native plan of a case, and the facts the CPU test checks against nqa_plan_query -----------------------------------------------------------------
def native_plan(case):
    """``NativePlan`` of the case in its layouts (``nqa_plan_create``: host code, no GPU)."""
    from nequip_amd.o3 import Irreps
    from nequip_amd.o3.tensor_product import NativePlan, _normalize_instructions

    f_in, e_at, mid = case.plan.strings()
    return NativePlan(Irreps(f_in), Irreps(e_at), Irreps(mid), _normalize_instructions(case.plan.instructions),
                      layout_in1=case.layout_in1, layout_out=case.layout_out)


def expected_ypart_width(plan):
    return sum(-(-plan.in1[i1][0] // 64) * (2 * plan.in2[i2][1] + 1) for i1, i2, *_ in plan.instructions)


def num_chunks(plan):
    return sum(-(-plan.in1[i1][0] // 64) for i1, *_ in plan.instructions)
