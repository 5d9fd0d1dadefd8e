"""Cases, float64 restatements and the checker of the fused radial MLP (``nequip_amd/csrc/radial_mlp.hip``,
``radial_mlp_pipe.h``), shared by ``tests/test_radial_mlp_reference.py`` (CPU) and ``tests/test_radial_mlp_launches.py``
(GPU).  A plain module: no fixtures, no pytest import.

Every output of every C entry point is restated from the formulas of ``include/nequip_amd.h`` with ``W_i = w_i alpha_i``:

    P = emb W0, G = g W1^T, Q = c W0, sig = sigmoid(P)
    silu(P) = P sig      silu'(P) = sig (1 + P (1 - sig))      silu''(P) = sig (1 - sig) (2 + P (1 - 2 sig))

    fwd        out         = silu(P) W1
    bwd        g_emb       = (G silu'(P)) W0^T                 (``paired``: g = g_a + g_b, added while loading)
    train1     g_emb as bwd, hidden = silu(P), parts[t] = emb_t^T (G silu'(P))_t             per 128-row tile t
    train2     g_emb = (Q G silu''(P)) W0^T, hidden = Q silu'(P),
               parts[t] = emb_t^T (Q G silu''(P))_t + c_t^T (G silu'(P))_t
    tangent    out         = (Q silu'(P)) W1
    last_fwd   out         = silu(pre) W
    last_bwd   grad_pre    = ((g_a + g_b) W^T) silu'(pre)

Each value travels with its MAGNITUDE SUM: the same expression with absolute values at every product (``VM`` below; the
sigmoid factors are positive and enter as they are, so silu and its derivatives are the products written above, with
``|P| -> |emb| |W0|``).  ``rho(X) = max |X - ref64| / magnitude_sum`` over ALL elements; where the magnitude sum is zero
the result has to be exactly zero.  The bound is the project's "as accurate as fp32":

    rho(kernel) <= 3 max(rho(float32 CPU evaluation of the same restatement), rho(exact-fp32 kernel) where there is one)
                   + floor(kind)

``floor(kind)``: at E = 1 or nb = 1 the float32 CPU error can be zero by luck, so every bound gets the largest
rho(float32 CPU) of all cases of that output kind on top (``floor``; from the reference alone, never from a kernel).

DATA FORMS (``Case.data``).  Every form has one all-zero row z = E // 2 (for E >= 3): emb, g (both streams) and pre are
zero there, the cotangent c is not.  What that row must hold is ``ZERO_ROW`` below.
    randn   plain normal data
    rows    embedding / pre rows times 2^k, k in [-66, 0]; gradient rows times 2^k, k in [-33, 33]; cotangent rows
            times 2^k, k in [-20, 20] (20 orders of magnitude each)
    cols    32-column groups of the second-layer weight times 2^k, k in [-33, 33], and of the gradient times 2^k,
            k in [-20, 20]  (the groups are the kernels' column tiles / K chunks: the fp16 split scales per group)
    tiny, pos30, neg30 (last layers only)   pre-activation rows around 1e-12, +30 and -30 (silu(-30) = -2.8e-12,
            silu'(-30) = -2.7e-12)
"""

import ctypes
import dataclasses
import math
import os
import sys
import zlib
from typing import Dict, Optional, Tuple

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RHO_FACTOR = 3.0  # as in tests/wgrad_cases.py and tests/test_radial_mlp.py
FLOOR_LIMIT = 1e-6  # the absolute level the older tests assert; one fp16 / bf16 plane is 2-3 orders above
TILE_ROWS = 128  # kMlpRows
GUARD = 4096  # floats of sentinel on each side of every output
SENTINEL_BITS = 0x7FC12345  # a NaN with a payload: no finite data gives it, and no arithmetic produces this payload
NQA_OK, NQA_ERR_INVALID, NQA_ERR_UNSUPPORTED, NQA_ERR_LAUNCH, NQA_ERR_WORKSPACE = 0, -1, -2, -3, -4
FP32, BF16X6, F16X3 = 0, 1, 2  # NQA_MLP_*
MODE_NAMES = {FP32: "fp32", BF16X6: "bf16x6", F16X3: "f16x3"}

ROW_EDGES = (1, 31, 32, 33, 127, 128, 129, 257, 1000)
REAL_FORMS = ("randn", "rows", "cols")
PRE_FORMS = ("tiny", "pos30", "neg30")

# op -> (output names, modes the entry point accepts)
OPS = {
    "fwd": (("out",), (FP32, BF16X6, F16X3)),
    "bwd": (("g_emb",), (FP32, BF16X6, F16X3)),
    "paired": (("g_emb",), (BF16X6, F16X3)),
    "train1": (("g_emb", "hidden", "parts"), (BF16X6, F16X3)),
    "train2": (("g_emb", "hidden", "parts"), (BF16X6, F16X3)),
    "tangent": (("out",), (BF16X6,)),
    "last_fwd": (("out",), (F16X3,)),
    "last_bwd": (("grad_pre",), (F16X3,)),
    "last_bwd2": (("grad_pre",), (F16X3,)),  # with the second stream grad_out2
}
# output kind (what the floor is taken over): bwd and paired, last_bwd and last_bwd2 are the same output
KIND_OF_OP = {"paired": "bwd", "last_bwd2": "last_bwd"}
# the all-zero row z: what each output must hold there ("0": exact zeros; "formula": whatever the restatement gives, which
# is not zero -- Q silu'(0) = Q / 2 with Q = c W0 of the non-zero cotangent row)
ZERO_ROW = {
    ("fwd", "out"): "0", ("bwd", "g_emb"): "0", ("paired", "g_emb"): "0",
    ("train1", "g_emb"): "0", ("train1", "hidden"): "0",
    ("train2", "g_emb"): "0", ("train2", "hidden"): "formula", ("tangent", "out"): "formula",
    ("last_fwd", "out"): "0", ("last_bwd", "grad_pre"): "0", ("last_bwd2", "grad_pre"): "0",
}  # (parts is indexed by tile, not by row: the zero row adds nothing to it)


@dataclasses.dataclass(frozen=True)
class Case:
    op: str
    nb: int  # 0: the last-layer entry points
    H: int
    W: int
    E: int
    data: str = "randn"

    @property
    def name(self):
        return f"{self.op}-nb{self.nb}-H{self.H}-W{self.W}-E{self.E}-{self.data}"

    @property
    def problem(self):  # inputs are shared by all ops on one shape
        return ("last" if self.nb == 0 else "mlp", self.nb, self.H, self.W, self.E, self.data)


def kind(case_or_op, out: str) -> str:
    op = case_or_op.op if isinstance(case_or_op, Case) else case_or_op
    return f"{KIND_OF_OP.get(op, op)}.{out}"


def zero_row(E: int) -> Optional[int]:
    return E // 2 if E >= 3 else None


def tiles(E: int) -> int:
    return -(-E // TILE_ROWS)


# ---- the case lists ------------------------------------------------------------------------------------------------------
SWEEP_NB = (1, 3, 5, 7, 8)
SWEEP_HW = ((64, 36), (64, 160), (128, 64), (128, 100), (128, 192))
SWEEP_OPS = ("fwd", "bwd", "paired", "train1", "train2", "tangent")
TRAIN_HW = ((64, 64), (64, 36), (128, 192), (128, 100))
TRAIN_OPS = ("train1", "train2")
LAST_H = (64, 128)
LAST_W = (4, 36, 160, 256)
LAST_OPS = ("last_fwd", "last_bwd", "last_bwd2")
VARIANT_NB = (5, 8)
VARIANT_SHAPES = ((300, 128, 64), (300, 128, 192), (300, 64, 64))  # (E, H, W)
# more work units than the persistent kernels have workgroups (two per CU, 256 CUs), so that a workgroup walks a range:
# forward units = 128-row blocks x 32-column tiles = 17 x 32; backward units = 128-row blocks = 514
MANY_UNITS_FWD = tuple(Case("fwd", 5, H, 1024, 2100, "randn") for H in (64, 128))
MANY_UNITS_BWD = tuple(Case("bwd", 5, H, 64, 65700, "randn") for H in (64, 128))


def sweep_rows(nb: int, H: int, W: int):
    """E = 1 and E = 129 always, one more row edge that rotates over the sweep; the three data forms in turn."""
    i = SWEEP_NB.index(nb) + 2 * SWEEP_HW.index((H, W))
    rest = tuple(e for e in ROW_EDGES if e not in (1, 129))
    return ((1, "randn"), (129, "rows"), (rest[i % len(rest)], ("cols", "randn", "rows")[i % 3]))


def sweep_cases(op: str, nb: int, H: int, W: int):
    return [Case(op, nb, H, W, E, data) for E, data in sweep_rows(nb, H, W)]


def train_cases(op: str, H: int, W: int, data: str):
    return [Case(op, 8, H, W, E, data) for E in ROW_EDGES]


def last_cases(op: str, H: int, W: int, data: str):
    return [Case(op, 0, H, W, E, data) for E in ROW_EDGES]


def variant_cases(op: str, E: int, H: int, W: int):
    return [Case(op, nb, H, W, E, "randn") for nb in VARIANT_NB]


def all_cases():
    out = []
    for nb in SWEEP_NB:
        for H, W in SWEEP_HW:
            for op in SWEEP_OPS:
                out += sweep_cases(op, nb, H, W)
    for H, W in TRAIN_HW:
        for data in REAL_FORMS:
            for op in TRAIN_OPS + ("tangent",):
                out += train_cases(op, H, W, data)
    for H in LAST_H:
        for W in LAST_W:
            for data in REAL_FORMS + PRE_FORMS:
                for op in LAST_OPS:
                    out += last_cases(op, H, W, data)
    for E, H, W in VARIANT_SHAPES:
        for op in ("fwd", "bwd"):
            out += variant_cases(op, E, H, W)
    out += MANY_UNITS_FWD + MANY_UNITS_BWD
    seen, uniq = set(), []
    for c in out:
        if c not in seen:
            seen.add(c)
            uniq.append(c)
    return uniq


ALL_CASES = all_cases()


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def alphas(nb: int, H: int) -> Tuple[float, float]:
    """ScalarMLPFunction's: 1 / sqrt(fan_in) for the first layer, sqrt(2) / sqrt(fan_in) after a SiLU."""
    return (1.0 / math.sqrt(nb) if nb else 1.0), math.sqrt(2.0) / math.sqrt(H)


def _exp2_int(lo: int, hi: int, shape, gen) -> torch.Tensor:
    return torch.exp2(torch.randint(lo, hi + 1, shape, generator=gen).float())


_PROBLEMS: Dict[tuple, dict] = {}


def make_inputs(case: Case) -> dict:
    """float32 CPU inputs of the case's shape and data form (a function of these alone, shared by all ops):
    two layers: emb [E, nb], c [E, nb], w0 [nb, H], w1 [H, W], g_a, g_b [E, W] (g = g_a + g_b; the one-stream entry points
    get ``g``, the float32 sum); last layers: pre [E, H], w1 [H, W], g_a, g_b."""
    key = case.problem
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    _, nb, H, W, E, data = key
    gen = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
    p = {}
    uni = lambda *s: (torch.rand(*s, generator=gen) * 2 - 1) * math.sqrt(3.0)  # ScalarLinearLayer's init
    p["w1"] = uni(H, W)
    g = torch.randn(E, W, generator=gen)
    if nb:
        p["w0"] = uni(nb, H)
        lead = torch.randn(E, nb, generator=gen) * 0.7
        p["c"] = torch.randn(E, nb, generator=gen)
    else:
        lead = torch.randn(E, H, generator=gen)
    if data == "rows":
        lead = lead * _exp2_int(-66, 0, (E, 1), gen)
        g = g * _exp2_int(-33, 33, (E, 1), gen)
        if nb:
            p["c"] = p["c"] * _exp2_int(-20, 20, (E, 1), gen)
    elif data == "cols":
        groups = -(-W // 32)
        p["w1"] = p["w1"] * _exp2_int(-33, 33, (groups,), gen).repeat_interleave(32)[:W]
        g = g * _exp2_int(-20, 20, (groups,), gen).repeat_interleave(32)[:W]
    elif data in PRE_FORMS:
        assert nb == 0, "pre-activation forms belong to the last-layer entry points"
        centre = {"tiny": 1e-12, "pos30": 30.0, "neg30": -30.0}[data]
        jitter = 1.0 + (torch.rand(E, H, generator=gen) * 2 - 1) / 64
        lead = centre * jitter * (torch.sign(lead) if data == "tiny" else 1.0)
    elif data != "randn":
        raise ValueError(data)
    g_a = g * 0.25  # exact
    g_b = g - g_a
    z = zero_row(E)
    if z is not None:
        lead[z] = 0.0
        g_a[z] = 0.0
        g_b[z] = 0.0
    p["g_a"], p["g_b"] = g_a.contiguous(), g_b.contiguous()
    p["g"] = (g_a + g_b).contiguous()  # what the one-stream entry points read (float32, exactly representable input)
    p["emb" if nb else "pre"] = lead.contiguous()
    p = {k: v.float().contiguous() for k, v in p.items()}
    _PROBLEMS[key] = p
    return p


# ---- restatements ------------------------------------------------------------------------------------------------------------
class VM:
    """A value and its magnitude sum.  Products and sums of VMs give the value and the same expression with absolute
    values at every product."""

    def __init__(self, v: torch.Tensor, m: Optional[torch.Tensor] = None):
        self.v, self.m = v, (v.abs() if m is None else m)

    def __matmul__(self, o):
        return VM(self.v @ o.v, self.m @ o.m)

    def __mul__(self, o):
        return VM(self.v * o.v, self.m * o.m)

    def __add__(self, o):
        return VM(self.v + o.v, self.m + o.m)

    @property
    def T(self):
        return VM(self.v.t(), self.m.t())

    def rows(self, lo, hi):
        return VM(self.v[lo:hi], self.m[lo:hi])


def _silu_parts(P: VM):
    """silu(P), silu'(P), silu''(P) as VMs: products of P with positive sigmoid factors."""
    sig = torch.sigmoid(P.v)
    one, two = VM(torch.ones_like(sig)), VM(torch.full_like(sig, 2.0))
    S, C, D = VM(sig), VM(1.0 - sig), VM(1.0 - 2.0 * sig)
    return P * S, S * (one + P * C), S * C * (two + P * D)


def _per_tile(f, E: int) -> VM:
    parts = [f(t * TILE_ROWS, min(E, (t + 1) * TILE_ROWS)) for t in range(tiles(E))]
    return VM(torch.stack([x.v for x in parts]), torch.stack([x.m for x in parts]))


def restate(case: Case, dtype=torch.float64, inputs: Optional[dict] = None) -> Dict[str, VM]:
    """Outputs of ``case.op`` as VMs, evaluated in ``dtype`` on the CPU."""
    p = make_inputs(case) if inputs is None else inputs
    op, nb, H, E = case.op, case.nb, case.H, case.E
    a0, a1 = alphas(nb, H)
    t = lambda x: VM(x.to(dtype))
    scaled = lambda w, a: VM(w.to(dtype) * torch.tensor(a, dtype=dtype))
    W1 = scaled(p["w1"], a1)
    two_streams = op in ("paired", "last_bwd2")
    g = (t(p["g_a"]) + t(p["g_b"])) if two_streams else t(p["g"])
    if nb == 0:
        s0, s1, _ = _silu_parts(t(p["pre"]))
        if op == "last_fwd":
            return {"out": s0 @ W1}
        return {"grad_pre": (g @ W1.T) * s1}
    W0 = scaled(p["w0"], a0)
    emb, c = t(p["emb"]), t(p["c"])
    s0, s1, s2 = _silu_parts(emb @ W0)
    if op == "fwd":
        return {"out": s0 @ W1}
    Q = c @ W0
    if op == "tangent":
        return {"out": (Q * s1) @ W1}
    G = g @ W1.T
    GP = G * s1
    if op in ("bwd", "paired"):
        return {"g_emb": GP @ W0.T}
    if op == "train1":
        return {"g_emb": GP @ W0.T, "hidden": s0,
                "parts": _per_tile(lambda lo, hi: emb.rows(lo, hi).T @ GP.rows(lo, hi), E)}
    if op == "train2":
        X = Q * G * s2
        return {"g_emb": X @ W0.T, "hidden": Q * s1,
                "parts": _per_tile(lambda lo, hi: emb.rows(lo, hi).T @ X.rows(lo, hi) + c.rows(lo, hi).T @ GP.rows(lo, hi),
                                   E)}
    raise ValueError(op)


# ---- measure, bound, checker ---------------------------------------------------------------------------------------------------
def rho(x: torch.Tensor, ref: torch.Tensor, mag: torch.Tensor) -> float:
    """max |x - ref| / mag over ALL elements; where mag is zero (an all-zero row) x must be exactly zero."""
    x = x.double()
    if x.shape != ref.shape or not bool(torch.isfinite(x).all()):
        return float("inf")
    live = mag > 0
    if torch.count_nonzero(x[~live]):
        return float("inf")
    if not bool(live.any()):
        return 0.0
    return float(((x - ref).abs()[live] / mag[live]).max())


@dataclasses.dataclass
class Reference:
    ref: Dict[str, torch.Tensor]  # float64
    mag: Dict[str, torch.Tensor]
    f32: Dict[str, torch.Tensor]  # the float32 CPU evaluation
    rho32: Dict[str, float]


_REFERENCES: Dict[Case, Reference] = {}


def reference(case: Case) -> Reference:
    """Computed once per case and never changed."""
    if case not in _REFERENCES:
        r64 = restate(case, torch.float64)
        r32 = restate(case, torch.float32)
        ref = {k: v.v for k, v in r64.items()}
        mag = {k: v.m for k, v in r64.items()}
        f32 = {k: v.v for k, v in r32.items()}
        _REFERENCES[case] = Reference(ref, mag, f32, {k: rho(f32[k], ref[k], mag[k]) for k in ref})
    return _REFERENCES[case]


_FLOORS: Dict[str, float] = {}


def floors() -> Dict[str, float]:
    """Per output kind the largest rho(float32 CPU) over ALL_CASES."""
    if not _FLOORS:
        acc: Dict[str, float] = {}
        for case in ALL_CASES:
            for out, r in reference(case).rho32.items():
                k = kind(case, out)
                acc[k] = max(acc.get(k, 0.0), r)
        _FLOORS.update(acc)
    return _FLOORS


def bound(case: Case, out: str, rho_exact: Optional[float] = None) -> float:
    base = max(reference(case).rho32[out], rho_exact or 0.0)
    return RHO_FACTOR * base + floors()[kind(case, out)]


def check(case: Case, out: str, x: torch.Tensor, rho_exact: Optional[float] = None, tag: str = ""):
    """-> (failure strings, rho(x)) of one output: the bound over every element, and the all-zero row."""
    r = reference(case)
    fails = []
    want = r.ref[out]
    if tuple(x.shape) != tuple(want.shape):
        return [f"{case.name} {tag} {out}: shape {tuple(x.shape)} != {tuple(want.shape)}"], float("inf")
    rk = rho(x, want, r.mag[out])
    b = bound(case, out, rho_exact)
    if not rk <= b:
        fails.append(f"{case.name} {tag} {out}: rho = {rk:.3e} > bound {b:.3e} (rho fp32 CPU {r.rho32[out]:.3e}, "
                     f"floor {floors()[kind(case, out)]:.3e})")
    z = zero_row(case.E)
    rule = ZERO_ROW.get((case.op, out))
    if z is not None and rule is not None:
        row = x[z].double()
        if rule == "0" and torch.count_nonzero(row):
            fails.append(f"{case.name} {tag} {out}: the all-zero row {z} is not exactly zero")
        if rule == "formula" and not torch.count_nonzero(row):
            fails.append(f"{case.name} {tag} {out}: row {z} must hold Q silu'(0) = Q / 2 terms, it is zero")
    return fails, rk


# ---- launches (GPU) ------------------------------------------------------------------------------------------------------------
class Guarded:
    """An output in the middle of a buffer filled with the sentinel."""

    def __init__(self, shape, device):
        self.shape = tuple(shape)
        self.n = int(math.prod(self.shape))
        self.bits = torch.full((self.n + 2 * GUARD,), SENTINEL_BITS, dtype=torch.int32, device=device)

    def pointer(self):
        return ctypes.c_void_p(self.bits.data_ptr() + 4 * GUARD)

    def inspect(self):
        """-> (guards bit-identical?, number of output elements still holding the sentinel, the output as float32 CPU)."""
        bits = self.bits.cpu()
        inner = bits[GUARD:GUARD + self.n]
        guards_ok = bool((bits[:GUARD] == SENTINEL_BITS).all()) and bool((bits[GUARD + self.n:] == SENTINEL_BITS).all())
        return guards_ok, int((inner == SENTINEL_BITS).sum()), inner.view(torch.float32).reshape(self.shape).clone()


def output_shapes(case: Case):
    E, nb, H, W = case.E, case.nb, case.H, case.W
    return {"out": (E, W), "g_emb": (E, nb), "hidden": (E, H), "parts": (tiles(E), nb, H), "grad_pre": (E, H)}


def is_backward(op: str) -> int:
    return 0 if op in ("fwd", "tangent", "last_fwd") else 1


class Workspace:
    """A weight image buffer large enough for every mode of the direction, and the byte count the mode asks for."""

    def __init__(self, case: Case, mode: int, device):
        from nequip_amd import _lib

        lib = _lib.load()
        sizes = [lib.nqa_radial_mlp_workspace_bytes(m, is_backward(case.op), case.H, case.W) for m in (FP32, BF16X6, F16X3)]
        self.needed = int(lib.nqa_radial_mlp_workspace_bytes(mode & 0xFF, is_backward(case.op), case.H, case.W))
        self.buffer = torch.zeros(max(max(sizes), 256), dtype=torch.uint8, device=device)


def launch(case: Case, mode: int, device, *, expect: int = NQA_OK, workspace: Optional[Workspace] = None, ready: int = 0,
           short_by: int = 0, null_cotangent: bool = False, H_arg: Optional[int] = None):
    """One direct call of the case's C entry point.  Returns (outputs {name: float32 CPU tensor}, failure strings,
    workspace).  Asserts nothing itself; the failure strings name: a return code other than ``expect``, a changed guard
    element, and -- after NQA_OK -- an output element that still holds the sentinel or is not finite (after an error
    code: an output element that does NOT hold the sentinel any more).  ``short_by``: bytes the call is told the workspace is
    short of what the mode needs.  ``H_arg``: the hidden width the call is told (refusal tests)."""
    from nequip_amd import _lib

    lib = _lib.load()
    P = _lib.ptr
    p = {k: v.to(device) for k, v in make_inputs(case).items()}
    op, nb, H, W, E = case.op, case.nb, case.H if H_arg is None else H_arg, case.W, case.E
    a0, a1 = alphas(nb, case.H)
    names = OPS[op][0]
    shapes = output_shapes(case)
    outs = {n: Guarded(shapes[n], device) for n in names}
    ws = workspace or Workspace(case, mode, device)
    tail = (P(ws.buffer), ws.needed - short_by, ready, _lib.stream_ptr(device))
    F = _lib.NQA_F32
    cot = None if (op != "train2" and op != "tangent") or null_cotangent else p["c"]
    with torch.cuda.device(device):
        if op == "fwd":
            rc = lib.nqa_radial_mlp_fwd(F, mode, P(p["emb"]), P(p["w0"]), a0, P(p["w1"]), a1, nb, H, W, E,
                                        outs["out"].pointer(), *tail)
        elif op == "tangent":
            rc = lib.nqa_radial_mlp_fwd_tangent(F, mode, P(p["emb"]), P(cot), P(p["w0"]), a0, P(p["w1"]), a1, nb, H, W, E,
                                                outs["out"].pointer(), *tail)
        elif op == "bwd":
            rc = lib.nqa_radial_mlp_bwd(F, mode, P(p["emb"]), P(p["w0"]), a0, P(p["w1"]), a1, P(p["g"]), nb, H, W, E,
                                        outs["g_emb"].pointer(), *tail)
        elif op == "paired":
            rc = lib.nqa_radial_mlp_bwd_paired(F, mode, P(p["emb"]), P(p["w0"]), a0, P(p["w1"]), a1, P(p["g_a"]),
                                               P(p["g_b"]), nb, H, W, E, outs["g_emb"].pointer(), *tail)
        elif op in ("train1", "train2"):
            rc = lib.nqa_radial_mlp_bwd_train(F, mode, P(p["emb"]), P(cot), P(p["w0"]), a0, P(p["w1"]), a1, P(p["g"]), nb,
                                              H, W, E, outs["g_emb"].pointer(), outs["hidden"].pointer(),
                                              outs["parts"].pointer(), *tail)
        elif op == "last_fwd":
            rc = lib.nqa_radial_mlp_last_fwd(F, mode, P(p["pre"]), P(p["w1"]), a1, H, W, E, outs["out"].pointer(), *tail)
        elif op in ("last_bwd", "last_bwd2"):
            ga, gb = (p["g_a"], p["g_b"]) if op == "last_bwd2" else (p["g"], None)
            rc = lib.nqa_radial_mlp_last_bwd(F, mode, P(p["pre"]), P(p["w1"]), a1, P(ga), P(gb), H, W, E,
                                             outs["grad_pre"].pointer(), *tail)
        else:
            raise ValueError(op)
        torch.cuda.synchronize(device)
    tag = f"{case.name} [{MODE_NAMES.get(mode & 0xFF, mode)}]"
    fails = []
    if rc != expect:
        msg = lib.nqa_last_error()
        fails.append(f"{tag}: return code {rc}, expected {expect} ({msg.decode() if msg else ''})")
    got = {}
    for n, buf in outs.items():
        guards_ok, left, x = buf.inspect()
        got[n] = x
        if not guards_ok:
            fails.append(f"{tag} {n}: elements outside the output were written")
        if expect == NQA_OK and rc == NQA_OK:
            if left:
                fails.append(f"{tag} {n}: {left} of {buf.n} output elements were never written")
            elif not bool(torch.isfinite(x).all()):
                fails.append(f"{tag} {n}: output is not finite")
        elif expect != NQA_OK and left != buf.n:
            fails.append(f"{tag} {n}: a refused call wrote {buf.n - left} output elements")
    return got, fails, ws


def run_and_check(case: Case, mode: int, device, rho_exact: Optional[Dict[str, float]] = None, table=None, **kw):
    """Launch, then the checker on every output.  -> (failure strings, {out: rho}).  ``table``: a dict that collects, per
    (kind, mode), the largest rho(kernel), rho(float32 CPU) and ratio seen (``record``)."""
    got, fails, _ = launch(case, mode, device, **kw)
    rhos = {}
    if fails:
        return fails, rhos
    for out, x in got.items():
        f, rk = check(case, out, x, (rho_exact or {}).get(out), tag=f"[{MODE_NAMES[mode & 0xFF]}]")
        fails += f
        rhos[out] = rk
        record(table, case, out, mode, rk, rho_exact=(rho_exact or {}).get(out))
    return fails, rhos


def record(table, case: Case, out: str, mode: int, rk: float, label: Optional[str] = None,
           rho_exact: Optional[float] = None):
    """Per (entry.output, mode): the largest rho(kernel), rho(float32 CPU), ratio of the two and rho(kernel) / bound."""
    if table is None:
        return
    key = (f"{label or case.op}.{out}", MODE_NAMES[mode & 0xFF])
    r32 = reference(case).rho32[out]
    ratio = rk / r32 if r32 > 0 else 0.0  # (rho32 = 0 by luck, E = 1 or nb = 1: the floor alone is the bound)
    old = table.get(key, (0.0, 0.0, 0.0, 0.0, 0))
    table[key] = (max(old[0], rk), max(old[1], r32), max(old[2], ratio), max(old[3], rk / bound(case, out, rho_exact)),
                  old[4] + 1)


def format_table(table) -> str:
    lines = [f"{'entry.output':38s} mode    rho(kernel)  rho(fp32 CPU)  ratio  rho/bound  cases   (each the largest seen)"]
    for (k, m), (rk, r32, ratio, margin, n) in sorted(table.items()):
        lines.append(f"{k:38s} {m:7s} {rk:.3e}    {r32:.3e}      {ratio:5.2f}  {margin:5.2f}      {n}")
    lines.append("floors: " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(floors().items())))
    return "\n".join(lines)
