"""Cases and the checker of the edge-embedding kernels (``nequip_amd/csrc/edge_embed.hip``), shared by
``tests/test_edge_embed.py`` (GPU launches, CPU tests of the checker itself).  A plain module: no fixtures, no pytest import.

The reference is always the float64 oracle (``oracle.nn.sh_edge_attrs`` / ``oracle.nn.bessel_embedding`` with
``model_dtype=torch.float64``) on the CPU, differentiated twice by ``torch.autograd.grad(..., create_graph=True)``.  For
float32 cases the cotangents are drawn in float32 and upcast: the kernel computes in float64 and rounds only its stores.

The checker works per edge: ``max_j |got_ej - ref_ej| <= tol * scale_e`` with ``scale_e = max(max_j |ref_ej|, floor_e)``.
``floor_e`` is computed from the inputs alone: the magnitude sum of the terms that form the row -- the cutoff polynomial and
its first two derivatives with every coefficient taken positive (at ``min(x, 1)``), times the bounds ``w``, ``pi w^2``,
``pi^2 w^3`` on the radial basis and its first two x-derivatives, times ``|factor| * rr^k`` and the absolute cotangents.
The transverse part of the second order, ``E'(r) / r``, enters through ``|b'(x)| <= pi^2 w^3 x / 3``, so the floor has no
division by ``r``.

Where the reference is the limit: at second order ``torch.sinc`` differentiates ``(a cos a - sin a) / a^2``, which is 0 / a^2
in float64 below ``a ~ 1e-8``, so on the clamped edge (``x = 1.4e-14``) the oracle's radial ``g_vec2`` is 0 where the numpy
longdouble restatement (``longdouble_radial``) gives ``E'' (u.c) u + E'/r (c - u (u.c))`` of size 2e-3 .. 5e3: an error of
100 %, 9e6 .. 2e8 times ``tol * scale_e`` (measured on the CPU over all cases; with harmonics of l >= 2 the row's scale is
1e24 and hides it).  On every other row of every case the oracle's radial second order stays below 0.01 of the bound.  As
the rule for this suite has it, on the rows where the reference's measured error exceeds a tenth of the bound -- that one
row, asserted in ``tests/test_edge_embed.py`` -- the bound is 10 x that measured error (``reference_limits``).  The kernel
itself is held to the plain bound there too: the cases without harmonics are also checked against the longdouble
restatement, whose second order is exact on that row.
"""

import ctypes
import dataclasses
import math
import os
import sys
import zlib
from typing import Optional

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import nn as onn  # noqa: E402

R_MAX = 4.5
E_FULL = 513  # three workgroups of 256, the last one ragged
TABLE = ((4.5, 3.0), (4.0, 3.0))  # per-edge-type cutoffs [centre][neighbour]: three distinct values; named edges are (0, 0)
TOL = {"fwd": 1e-12, "vjp": 1e-11, "second": 1e-9}  # tests/test_reference_golden.py (x2), tests/test_training_step.py
ORDER_OF = {"sh": "fwd", "emb": "fwd", "cutoff": "fwd", "g_vec": "vjp", "g_vec2": "second", "gg_sh": "second",
            "gg_emb": "second"}
STORED_AS_T = {"sh": 1, "emb": 5, "cutoff": 1, "gg_sh": 1, "gg_emb": 1}  # roundings to T of the float32 instantiation
EPS32 = 2.0 ** -24
SENTINEL = -12345.5
# fixed rows of the named edges
ROW_AXES, ROW_SHORT, ROW_CLAMPED, ROW_AT_CUT, ROW_BELOW_CUT, ROW_NEAR_CUT, ROW_BEYOND = 0, 100, 255, 256, 257, 300, 512
NAMED_ROWS = tuple(range(6)) + (ROW_SHORT, ROW_CLAMPED, ROW_AT_CUT, ROW_BELOW_CUT, ROW_NEAR_CUT, ROW_BEYOND)


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    dtype: str = "float64"  # the kernel's T
    lmax: int = 2
    weights: str = "roots8"  # one | roots8 | roots32 | trained8 | trained32 | ulp8 | ulp32 | direct32
    p: float = 6.0
    per_edge: bool = False  # per-edge reciprocal cutoffs (cfg["rmax_edge"]) from TABLE
    want_sh: bool = True
    want_emb: bool = True
    grads: str = "all"  # which inputs of the VJP require grad at second order: all | vec | cot
    E: int = E_FULL
    factor: str = "model"  # model: 2 pi / r_max^2 | one

    @property
    def torch_dtype(self):
        return torch.float32 if self.dtype == "float32" else torch.float64

    @property
    def nb(self):
        return 1 if self.weights == "one" else int(self.weights.lstrip("abcdefghijklmnopqrstuvwxyz"))

    @property
    def factor_value(self):
        return 1.0 if self.factor == "one" else 2 * math.pi / (R_MAX * R_MAX)


def _cases():
    out = []
    for dt in ("float64", "float32"):
        for lmax in range(5):
            out.append(Case(f"lmax{lmax}-{dt}", dtype=dt, lmax=lmax))
    for w in ("one", "roots32", "trained8", "trained32", "ulp8", "ulp32"):
        out.append(Case(f"w-{w}-float64", weights=w, lmax=1))
    out.append(Case("w-roots32-float32", dtype="float32", weights="roots32", lmax=1))
    out.append(Case("w-trained32-float32", dtype="float32", weights="trained32", lmax=1))
    for p in (2.0, 2.5, 48.0, 64.0):  # p = 6 is everywhere else
        out.append(Case(f"p{p:g}-float64", p=p, lmax=1))
        out.append(Case(f"p{p:g}-embonly-float64", p=p, lmax=0, want_sh=False))
    out.append(Case("p2.5-roots32-float32", dtype="float32", p=2.5, weights="roots32", lmax=1))
    for dt in ("float64", "float32"):
        out.append(Case(f"peredge-{dt}", dtype=dt, per_edge=True, weights="trained8"))
        out.append(Case(f"peredge-embonly-{dt}", dtype=dt, per_edge=True, want_sh=False, lmax=0))
        out.append(Case(f"shonly-{dt}", dtype=dt, lmax=4, want_emb=False))
        out.append(Case(f"embonly-{dt}", dtype=dt, lmax=0, want_sh=False, weights="roots32"))
        for grads in ("vec", "cot"):
            out.append(Case(f"grads-{grads}-{dt}", dtype=dt, lmax=3, grads=grads))
    out.append(Case("grads-cot-embonly-float64", want_sh=False, lmax=0, grads="cot"))
    out.append(Case("grads-cot-shonly-float64", want_emb=False, lmax=2, grads="cot"))
    for E in (0, 1, 255, 256, 257):
        out.append(Case(f"E{E}-float32", dtype="float32", E=E, lmax=1))
    out.append(Case("factor-one-float64", factor="one", lmax=1))
    out.append(Case("factor-one-float32", dtype="float32", factor="one", want_sh=False, lmax=0))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def _generator(name: str) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _unit(gen, n):
    v = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    return v / v.norm(dim=1, keepdim=True)


def edge_set() -> torch.Tensor:
    """The 513 edge vectors every case uses (its first ``E`` rows): random bulk, named edges at fixed rows."""
    gen = _generator("edge-set")
    r = 0.05 + (1.15 * R_MAX - 0.05) * torch.rand(E_FULL, 1, generator=gen, dtype=torch.float64)
    vec = _unit(gen, E_FULL) * r
    for k, (axis, sign, length) in enumerate(((0, 1, 1.5), (0, -1, 2.5), (1, 1, 3.5), (1, -1, 0.7), (2, 1, 4.0),
                                              (2, -1, 4.4))):
        vec[ROW_AXES + k] = 0.0
        vec[ROW_AXES + k, axis] = sign * length
    d = torch.tensor([1.5, 3.0, 3.0], dtype=torch.float64)  # |d| = 4.5 exactly, with or without fused multiply-adds
    u = torch.tensor([0.48, -0.6, 0.64], dtype=torch.float64)
    vec[ROW_SHORT] = 1e-3 * u
    vec[ROW_CLAMPED] = torch.tensor([3e-14, -5e-14, 2e-14], dtype=torch.float64)
    vec[ROW_AT_CUT] = d
    vec[ROW_BELOW_CUT] = d * (1.0 - 1e-12)
    vec[ROW_NEAR_CUT] = 4.4999 * u
    vec[ROW_BEYOND] = -1.2 * d
    return vec


def bessel_weights(case: Case) -> torch.Tensor:
    nb = case.nb
    bw = torch.linspace(1.0, nb, nb, dtype=torch.float64)
    kind = case.weights.rstrip("0123456789")
    if kind == "trained":
        bw = bw + 0.07 * torch.randn(nb, generator=_generator(f"bw{nb}"), dtype=torch.float64)
    elif kind == "ulp":  # only the last root moved, by one ulp: the whole launch leaves the angle-addition path
        bw[-1] = float(np.nextafter(float(nb), np.inf))
    elif kind == "direct":  # the last root far off: certainly one sin/cos per basis function
        bw[-1] = nb + 0.5
    return bw


def make_inputs(case: Case):
    """Everything a launch and the reference read, on the CPU, a function of the case's name."""
    gen = _generator(case.name)
    E, T = case.E, case.torch_dtype
    inp = dict(vec=edge_set()[:E].clone(), bw=bessel_weights(case), rmax_edge=None, table=None, edge_types=None)
    if case.per_edge:
        et = torch.randint(0, 2, (2, E), generator=gen)
        named = torch.tensor([r for r in NAMED_ROWS if r < E and r != ROW_SHORT], dtype=torch.long)
        et[:, named] = 0  # r_cut = 4.5 for the named edges (the short one keeps its random type)
        table = torch.tensor(TABLE, dtype=torch.float64)
        inp.update(table=table, edge_types=et,
                   rmax_edge=torch.index_select(table.reciprocal().view(-1), 0, et[0] * 2 + et[1]).contiguous())
    S = (case.lmax + 1) ** 2
    inp["g_sh"] = torch.randn(E, S, generator=gen, dtype=T) if case.want_sh else None
    inp["g_emb"] = torch.randn(E, case.nb, generator=gen, dtype=T) if case.want_emb else None
    inp["c"] = torch.randn(E, 3, generator=gen, dtype=torch.float64)
    return inp


def recip_cutoff(case: Case, inp) -> torch.Tensor:
    """[E, 1] reciprocal cutoffs as the kernel and the oracle form them."""
    if case.per_edge:
        return inp["rmax_edge"].view(-1, 1)
    return torch.full((inp["vec"].shape[0], 1), 1.0 / R_MAX, dtype=torch.float64)


def outside(case: Case, inp) -> torch.Tensor:
    """[E] bool: x >= 1, with x as the oracle computes it."""
    r = inp["vec"].square().sum(1, keepdim=True).sqrt()
    return ~((r * recip_cutoff(case, inp)).view(-1) < 1.0)


def cfg_of(case: Case, inp, device=None):
    cfg = dict(dtype=case.torch_dtype, lmax=case.lmax, want_sh=case.want_sh, want_emb=case.want_emb, nb=case.nb,
               rmax_recip=1.0 / R_MAX, p=float(case.p), factor=case.factor_value)
    if case.per_edge:
        cfg["rmax_edge"] = inp["rmax_edge"].to(device) if device is not None else inp["rmax_edge"]
    return cfg


# ---- the oracle, with the mutations the checker has to reject ---------------------------------------------------------------
MUTATIONS = {  # name -> orders at which it is visible
    "coefficient": ("fwd", "vjp", "second"),  # middle cutoff coefficient p (p + 2) -> p (p + 1)
    "last-column": ("fwd", "vjp", "second"),  # last basis column * (1 + 1e-7): recurrence drift at nb = 32
    "global-cutoff": ("fwd", "vjp", "second"),  # per-edge cutoffs ignored
    "harmonic-sign": ("fwd", "vjp", "second"),  # one l = 4 harmonic with its sign flipped
    "no-mask": ("fwd", "vjp", "second"),  # cutoff mask x < 1 removed
}
MUTATION_CASE = {"coefficient": "p2-embonly-float64", "last-column": "embonly-float64", "global-cutoff": "peredge-float64",
                 "harmonic-sign": "lmax4-float64", "no-mask": "embonly-float64"}


def oracle_embed(case: Case, inp, v, mutation: Optional[str] = None):
    """(sh | None, emb | None, cutoff) of the float64 oracle for edge vectors ``v``; ``mutation`` restates
    ``bessel_embedding`` with one thing wrong (without a mutation it IS ``oracle.nn.bessel_embedding``)."""
    sh = emb = cut = None
    if case.want_sh:
        sh = onn.sh_edge_attrs(v, case.lmax, torch.float64) + 0.0 * v.sum()  # lmax = 0: Y_0 = 1 is constant
        if mutation == "harmonic-sign":
            flip = torch.ones(sh.shape[1], dtype=torch.float64)
            flip[16 + 5] = -1.0
            sh = sh * flip
    if case.want_emb:
        bw = inp["bw"].unsqueeze(0)
        kw = {}
        if case.per_edge and mutation != "global-cutoff":
            kw = dict(per_edge_type_cutoff=inp["table"], edge_types=inp["edge_types"])
        if mutation in (None, "global-cutoff", "harmonic-sign"):  # ("restated": the branch below with nothing changed)
            emb, cut = onn.bessel_embedding(v, R_MAX, case.nb, case.p, torch.float64, bessel_weights=bw, **kw)
        else:
            p = float(case.p)
            r = v.square().sum(1, keepdim=True).sqrt()
            x = r * recip_cutoff(case, inp)
            bessel = torch.sinc(x * bw) * bw
            if mutation == "last-column":
                scale = torch.ones(case.nb, dtype=torch.float64)
                scale[-1] = 1.0 + 1e-7
                bessel = bessel * scale
            mid = p * (p + 1.0) if mutation == "coefficient" else p * (p + 2.0)
            cut = 1.0 - (((p + 1.0) * (p + 2.0) / 2.0) * torch.pow(x, p)) + (mid * torch.pow(x, p + 1.0)) \
                - ((p * (p + 1.0) / 2) * torch.pow(x, p + 2.0))
            if mutation != "no-mask":
                cut = cut * (x < 1.0)
            emb = (2 * math.pi) / (R_MAX * R_MAX) * (bessel * cut)
        if case.factor == "one":
            emb = emb * (R_MAX * R_MAX / (2 * math.pi))
    return sh, emb, cut


# ---- the three orders through autograd (oracle, autograd Functions, dispatcher ops alike) -------------------------------------
def run_chain(case: Case, inp, embed, vjp=None, device=None, grads: Optional[str] = None):
    """``embed(v) -> (sh | None, emb | None)`` differentiable in ``v``; ``vjp(v, g_sh, g_emb) -> g_vec`` differentiable in
    all three (needed for ``grads = "cot"``, where the vector must not require grad).  Returns the outputs on the CPU:
    sh, emb, g_vec, and of the second order those that ``grads`` asks for."""
    grads = grads or case.grads
    to = (lambda t: t.to(device)) if device is not None else (lambda t: t)
    v = to(inp["vec"]).clone().requires_grad_(True)
    sh, emb = embed(v)
    outs = [t for t in (sh, emb) if t is not None]
    cot_grad = grads in ("all", "cot")
    a = to(inp["g_sh"]).clone().requires_grad_(cot_grad) if sh is not None else None
    b = to(inp["g_emb"]).clone().requires_grad_(cot_grad) if emb is not None else None
    cots = [t for t in (a, b) if t is not None]
    if grads == "cot" and vjp is not None:
        gv = vjp(v.detach(), a, b)
    else:
        (gv,) = torch.autograd.grad(outs, [v], cots, create_graph=True)
    targets = ([("g_vec2", v)] if grads in ("all", "vec") else []) + \
              ([(n, t) for n, t in (("gg_sh", a), ("gg_emb", b)) if t is not None] if cot_grad else [])
    second = torch.autograd.grad([gv], [t for _, t in targets], [to(inp["c"])], allow_unused=True)
    res = dict(sh=sh, emb=emb, g_vec=gv)
    for (name, t), g in zip(targets, second):
        res[name] = g if g is not None else torch.zeros_like(t)
    return {k: t.detach().cpu() for k, t in res.items() if t is not None}


def oracle_outputs(case: Case, inp, mutation: Optional[str] = None):
    """All outputs of the float64 oracle (``cutoff`` included) for ``inp``, its cotangents upcast to float64."""
    inp64 = dict(inp, **{k: inp[k].double() for k in ("g_sh", "g_emb") if inp[k] is not None})
    ref = run_chain(case, inp64, lambda v: oracle_embed(case, inp64, v, mutation)[:2], grads="all")
    if case.want_emb:
        ref["cutoff"] = oracle_embed(case, inp64, inp64["vec"], mutation)[2].view(-1, 1)
    assert all(t.dtype == torch.float64 for t in ref.values())
    return ref


_REF_CACHE = {}


def reference(case: Case, mutation: Optional[str] = None):
    """(inputs, float64 reference outputs) of a case; computed once, never modified."""
    key = (case.name, mutation)
    if key not in _REF_CACHE:
        inp = make_inputs(case)
        _REF_CACHE[key] = (inp, oracle_outputs(case, inp, mutation))
    return _REF_CACHE[key]


# ---- floors ----------------------------------------------------------------------------------------------------------------------
def floors(case: Case, inp):
    """name -> [E] cancellation floor of that output's rows, from the inputs alone (see the module docstring)."""
    E = inp["vec"].shape[0]
    zero = torch.zeros(E, dtype=torch.float64)
    out = {k: zero for k in ORDER_OF}
    if not case.want_emb:
        return out
    p, f = float(case.p), abs(case.factor_value)
    rr = recip_cutoff(case, inp)  # [E, 1]
    x = inp["vec"].square().sum(1, keepdim=True).sqrt() * rr
    xc = x.clamp(max=1.0)
    A, B, C = (p + 1.0) * (p + 2.0) / 2.0, p * (p + 2.0), p * (p + 1.0) / 2.0
    C0 = 1.0 + A * xc ** p + B * xc ** (p + 1.0) + C * xc ** (p + 2.0)
    C1 = A * p * xc ** (p - 1.0) + B * (p + 1.0) * xc ** p + C * (p + 2.0) * xc ** (p + 1.0)
    C2 = A * p * (p - 1.0) * xc ** (p - 2.0) + B * (p + 1.0) * p * xc ** (p - 1.0) + C * (p + 2.0) * (p + 1.0) * xc ** p
    w = inp["bw"].abs().view(1, -1)

    B0, B1, B2 = w, math.pi * w ** 2, math.pi ** 2 * w ** 3  # bounds on b, b', b''
    g = inp["g_emb"].double().abs()
    cn = inp["c"].norm(dim=1, keepdim=True)
    out["emb"] = (f * C0 * w.max()).view(-1)
    out["cutoff"] = C0.view(-1)
    out["g_vec"] = (f * rr * (g * (B1 * C0 + B0 * C1)).sum(1, keepdim=True)).view(-1)
    first = B1 * C0 + B0 * C1
    out["gg_emb"] = (f * rr * cn * first.max(dim=1, keepdim=True).values).view(-1)
    # E''(r) along u, and E'(r) / r across it: |b'| <= pi^2 w^3 x / 3 and c'(x) / x with positive coefficients (p >= 2)
    C1x = A * p * xc ** (p - 2.0) + B * (p + 1.0) * xc ** (p - 1.0) + C * (p + 2.0) * xc ** p
    out["g_vec2"] = (cn * f * rr * rr * (g * (B2 * C0 + 2.0 * B1 * C1 + B0 * C2 + B2 * C0 / 3.0 + B0 * C1x))
                     .sum(1, keepdim=True)).view(-1)
    return out


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def reference_limits(case: Case, inp, ref):
    """name -> [E]: the float64 oracle's own row error in the radial part of the second-order outputs, measured against
    the longdouble restatement, on the rows where it exceeds a tenth of ``tol * scale_e`` (zero elsewhere)."""
    if not case.want_emb or inp["vec"].shape[0] == 0:
        return {}
    radial = dataclasses.replace(case, want_sh=False)
    inp_r = dict(inp, g_sh=None)
    rad = oracle_outputs(radial, inp_r) if case.want_sh else ref
    ld, fl, out = longdouble_radial(radial, inp_r), floors(case, inp), {}
    for name in ("g_vec2", "gg_emb"):
        err = (rad[name] - ld[name]).abs().amax(dim=1)
        bound = TOL["second"] * torch.maximum(ref[name].abs().amax(dim=1), fl[name])
        out[name] = torch.where(err > 0.1 * bound, err, torch.zeros_like(err))
    return out


def check(case: Case, inp, ref, got, names=None, ref_is_oracle=True):
    """Failure strings and ``order -> max error / bound`` of ``got`` (name -> CPU tensor) against ``ref``.  Per edge:
    ``|got - ref|_ej <= tol * max(max_j |ref_ej|, floor_e)``, plus, for values the float32 kernel stores as float32, the
    ``n * 2^-24 |ref_ej|`` of its ``n`` roundings; rows of edges with ``x >= 1`` that hold radial terms only must be zero.
    With the oracle as ``ref``, rows on which the oracle itself is the limit get 10 x its measured error as their bound."""
    second = any(n in ("g_vec2", "gg_emb") for n in (names or got.keys()))
    limits = reference_limits(case, inp, ref) if (ref_is_oracle and second) else {}
    fl = floors(case, inp)
    out_mask = outside(case, inp)
    fails, ratios = [], {}
    for name in (names or got.keys()):
        order = ORDER_OF[name]
        g, r = got[name].double(), ref[name]
        if g.shape != r.shape:
            fails.append(f"{case.name}: {name} has shape {tuple(g.shape)}, expected {tuple(r.shape)}")
            continue
        if g.numel() == 0:
            continue
        if not torch.isfinite(r).all():
            fails.append(f"{case.name}: the reference's {name} is not finite")
            continue
        scale = torch.maximum(r.abs().amax(dim=1), fl[name])
        bound = (TOL[order] * scale).view(-1, 1).expand_as(r).clone()
        if name in limits:
            bound = torch.maximum(bound, (10.0 * limits[name]).view(-1, 1))
        if case.dtype == "float32" and name in STORED_AS_T:
            bound = bound + STORED_AS_T[name] * EPS32 * r.abs()
        err = (g - r).abs()
        err = torch.where(torch.isfinite(err), err, torch.full_like(err, float("inf")))
        ratio = torch.where(bound > 0, err / bound, torch.where(err > 0, torch.full_like(err, float("inf")), err))
        worst = float(ratio.max())
        ratios[order] = max(ratios.get(order, 0.0), worst)
        if not worst <= 1.0:
            e, j = (int(i) for i in (ratio == ratio.max()).nonzero()[0])
            fails.append(f"{case.name}: {name}[{e}, {j}] = {float(g[e, j])!r}, reference {float(r[e, j])!r}: error "
                         f"{float(err[e, j]):.3e} is {worst:.3g} x the bound {float(bound[e, j]):.3e} "
                         f"({int((ratio > 1).any(dim=1).sum())} edges fail)")
        radial_only = name in ("emb", "gg_emb", "cutoff") or (name in ("g_vec", "g_vec2") and not case.want_sh)
        if radial_only and torch.count_nonzero(g[out_mask]):
            fails.append(f"{case.name}: {name} is not exactly zero on {int((g[out_mask] != 0).any(dim=1).sum())} edges with "
                         f"x >= 1")
    return fails, ratios


# ---- numpy longdouble restatement of the radial part (closed forms: comment above BesselBasis in edge_embed.hip) ----------------
LD = np.longdouble
PI_LD = LD("3.14159265358979323846264338327950288")


def _sinc_derivatives(a):
    """sin(a)/a and its first two derivatives in longdouble: the series below a = 1 (30 terms), closed forms above."""
    small = a < LD(1)
    t = np.where(small, a, LD(0))
    s0, s1, s2 = np.zeros_like(a), np.zeros_like(a), np.zeros_like(a)
    fact = LD(1)  # (2k + 1)!
    for k in range(30):
        if k:
            fact = fact * LD(2 * k) * LD(2 * k + 1)
        sign = LD(-1) ** k
        s0 = s0 + sign * t ** (2 * k) / fact
        if k:
            s1 = s1 + sign * LD(2 * k) * t ** (2 * k - 1) / fact
            s2 = s2 + sign * LD(2 * k) * LD(2 * k - 1) * t ** (2 * k - 2) / fact
    b = np.where(small, LD(1), a)
    sn, cs = np.sin(b), np.cos(b)
    return (np.where(small, s0, sn / b), np.where(small, s1, (b * cs - sn) / b ** 2),
            np.where(small, s2, -sn / b - 2 * cs / b ** 2 + 2 * sn / b ** 3))


def longdouble_radial(case: Case, inp):
    """The radial part in numpy longdouble, for the case's ``g_emb`` and ``c``: emb [E, nb], cutoff [E, 1], g_vec =
    E'(r) u, g_vec2 = E''(r) (u.c) u + E'(r)/r (c - u (u.c)) and gg_emb = factor rr (b' cut + b cut') (u.c), with u = v/|v|,
    b_n = w_n S(a), b_n' = pi w_n^2 S'(a), b_n'' = pi^2 w_n^3 S''(a), S(a) = sin(a)/a, a = pi x w_n."""
    v = inp["vec"].numpy().astype(LD)
    cv = inp["c"].numpy().astype(LD)
    w = inp["bw"].numpy().astype(LD)[None, :]
    rr = recip_cutoff(case, inp).numpy().astype(LD)
    g = inp["g_emb"].double().numpy().astype(LD)
    p, f = LD(case.p), LD(case.factor_value)
    r = np.sqrt((v * v).sum(1, keepdims=True))
    x = r * rr
    s0, s1, s2 = _sinc_derivatives(PI_LD * x * w)
    b, db, ddb = w * s0, PI_LD * w ** 2 * s1, PI_LD ** 2 * w ** 3 * s2
    A, B, C = (p + 1) * (p + 2) / 2, p * (p + 2), p * (p + 1) / 2
    inside = x < 1
    cut = np.where(inside, 1 - A * x ** p + B * x ** (p + 1) - C * x ** (p + 2), LD(0))
    dcut = np.where(inside, -A * p * x ** (p - 1) + B * (p + 1) * x ** p - C * (p + 2) * x ** (p + 1), LD(0))
    ddcut = np.where(inside, -A * p * (p - 1) * x ** (p - 2) + B * (p + 1) * p * x ** (p - 1)
                     - C * (p + 2) * (p + 1) * x ** p, LD(0))
    u = v / r
    uc = (u * cv).sum(1, keepdims=True)
    first = db * cut + b * dcut
    d1 = f * rr * (g * first).sum(1, keepdims=True)  # E'(r)
    d2 = f * rr * rr * (g * (ddb * cut + 2 * db * dcut + b * ddcut)).sum(1, keepdims=True)  # E''(r)
    as64 = lambda t: torch.from_numpy(np.asarray(t, dtype=np.float64).copy())  # noqa: E731
    return dict(emb=as64(f * b * cut), cutoff=as64(cut), g_vec=as64(d1 * u),
                g_vec2=as64(d2 * uc * u + d1 / r * (cv - u * uc)), gg_emb=as64(f * rr * first * uc))



# ---- launches through the C ABI (ctypes) ---------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p()


def padded(rows: int, cols: int, dtype, device):
    """An output buffer one row longer than the launch needs, prefilled with the sentinel."""
    return torch.full((rows + 1, cols), SENTINEL, dtype=dtype, device=device)


def raw_common(case: Case, inp, device):
    vec, bw = inp["vec"].to(device).contiguous(), inp["bw"].to(device)
    re = inp["rmax_edge"].to(device) if case.per_edge else None
    dt = 0 if case.dtype == "float32" else 1  # NQA_F32 / NQA_F64
    head = (dt, case.lmax, _p(vec), vec.shape[0], 1.0 / R_MAX, _p(re), case.nb, _p(bw), float(case.p), case.factor_value)
    return head, (vec, bw, re)


def run_raw(case: Case, inp, lib, device, stream=None, with_cutoff=True):
    """All three orders through ``nqa_edge_embed_fwd / _bwd / _bwd_bwd`` with padded, sentinel-filled outputs.  Returns
    (outputs on the CPU without the pad row, failure strings of return codes and touched pad rows)."""
    E, T, S, nb = case.E, case.torch_dtype, (case.lmax + 1) ** 2, case.nb
    stream = stream if stream is not None else ctypes.c_void_p()
    head, keep = raw_common(case, inp, device)
    g_sh = inp["g_sh"].to(device) if case.want_sh else None
    g_emb = inp["g_emb"].to(device) if case.want_emb else None
    c = inp["c"].to(device)
    bufs = dict(sh=padded(E, S, T, device) if case.want_sh else None,
                emb=padded(E, nb, T, device) if case.want_emb else None,
                cutoff=padded(E, 1, T, device) if (case.want_emb and with_cutoff) else None,
                g_vec=padded(E, 3, torch.float64, device),
                g_vec2=padded(E, 3, torch.float64, device) if case.grads in ("all", "vec") else None,
                gg_sh=padded(E, S, T, device) if (case.want_sh and case.grads in ("all", "cot")) else None,
                gg_emb=padded(E, nb, T, device) if (case.want_emb and case.grads in ("all", "cot")) else None)
    fails = []
    rcs = [lib.nqa_edge_embed_fwd(*head, _p(bufs["sh"]), _p(bufs["emb"]), _p(bufs["cutoff"]), stream),
           lib.nqa_edge_embed_bwd(*head, _p(g_sh), _p(g_emb), _p(bufs["g_vec"]), stream),
           lib.nqa_edge_embed_bwd_bwd(*head, _p(g_sh), _p(g_emb), _p(c), _p(bufs["gg_sh"]), _p(bufs["gg_emb"]),
                                      _p(bufs["g_vec2"]), stream)]
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    for fn, rc in zip(("fwd", "bwd", "bwd_bwd"), rcs):
        if rc != 0:
            fails.append(f"{case.name}: nqa_edge_embed_{fn} returned {rc}: {lib.nqa_last_error().decode()}")
    got = {}
    for name, buf in bufs.items():
        if buf is None:
            continue
        host = buf.cpu()
        if not bool((host[E] == SENTINEL).all()):
            fails.append(f"{case.name}: {name}: the row after the last edge was written")
        got[name] = host[:E].clone()
    del keep
    return got, fails
