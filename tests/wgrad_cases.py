"""Cases and checkers of ``nqa_wgrad`` (``nequip_amd/csrc/wgrad.hip``), shared by ``tests/test_wgrad.py``,
``tests/test_wgrad_host.py`` and the child processes these start (the environment switch of the kernel choice is read
once per process).  A plain module: no fixtures, no pytest import.

The reference is float64 and built by index: ``ref[t] = A[types == t]^T B[types == t]`` per record, the ``d`` components of
a record's rows through ``view(Z, mul, d)``.

* EXACT data: integers in [-8, 8].  Every product and every partial sum is an integer below 2^24 (``Z * d * 64 < 2^24`` for
  all cases here), bf16 holds the operands exactly (the mid and lo planes of the split are zero), so EVERY kernel variant
  and every summation order has to reproduce the reference bit for bit.  All structure cases use it: no tolerance an
  indexing, masking or tiling mistake could hide behind.
* REAL data: zero-mean floats in three forms (``randn``; rows scaled by 2^k on A and 2^-k on B; columns scaled by 2^k),
  measured as ``rho(X) = max_ij |X - ref64|_ij / (|A|^T |B|)_ij`` and bounded by ``3 * rho(float32 CPU A^T B)``.
"""

import ctypes
import dataclasses
import os
import struct
import sys
import zlib
from typing import Optional, Sequence, Tuple

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RHO_FACTOR = 3.0  # "as accurate as fp32": the factor tests/test_radial_mlp.py uses for the same claim
SENTINEL = 12345.0  # what forced-S launches put into the partial tiles before the kernel runs
MAX_RECORDS = 64  # kMaxWgradInstr


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    Z: int
    records: Tuple[Tuple[int, int, int, int, int, int], ...]  # (a_off, b_off, M, N, d, out_off)
    lda: int
    ldb: int
    out_stride: int
    T: int = 1
    types: str = "none"  # none | random | missing | single | sorted | alternating
    data: str = "exact"  # exact | randn | rows | cols
    S: Optional[int] = None  # forced split count: the launch goes through ctypes, partials are summed in float64 here


def packed(blocks: Sequence[Tuple[int, int, int]]):
    """Records of consecutive (M, N, d) blocks: operands and outputs packed without gaps -> records, lda, ldb, out_stride."""
    recs, ao, bo, oo = [], 0, 0, 0
    for M, N, d in blocks:
        recs.append((ao, bo, M, N, d, oo))
        ao, bo, oo = ao + M * d, bo + N * d, oo + M * N
    return tuple(recs), ao, bo, oo


def _case(name, Z, blocks, **kw):
    recs, lda, ldb, stride = packed(blocks)
    return Case(name, Z, recs, lda, ldb, stride, **kw)


# ---- the case lists --------------------------------------------------------------------------------------------------------
# kernel choice (wgrad_rb): widest M <= 32 -> wgrad_kernel<1>, <= 64 -> wgrad_kernel<2>, wider -> the split form
# wgrad_kernel<2, *, true> (or wgrad_kernel<4> under NQA_WGRAD_EXACT_FP32=1); T > 1 with types -> TYPED.
SPLIT_M, SPLIT_N, SPLIT_D = (65, 100, 128, 130), (1, 63, 64, 65, 129), (1, 3, 5, 7)
MIXED = ((8, 40, 3), (33, 65, 1), (64, 64, 5), (100, 63, 7))  # an 8-row record in the wide kernel, one launch
NARROW = ((8, 40, 3), (33, 65, 1), (64, 64, 5))
TABLES = {
    "m8": ((8, 65, 3),),  # wgrad_kernel<1>
    "m32": ((32, 64, 1),),  # wgrad_kernel<1>, full tile
    "m33": ((33, 63, 5),),  # wgrad_kernel<2>, second row block masked to one row
    "m64": ((64, 129, 7),),  # wgrad_kernel<2>
    "mixed": MIXED,
}
for _k in range(4):  # the full product M x N x d of the wide kernel in four launches of 20 records
    TABLES[f"split{_k}"] = tuple((M, N, SPLIT_D[(i + j + _k) % 4]) for i, M in enumerate(SPLIT_M)
                                 for j, N in enumerate(SPLIT_N))
LAYOUTS = ("missing", "single", "sorted", "alternating")
ROW_EDGES = (1, 15, 16, 17, 63, 65, 255, 256, 257, 1000, 4099)
FORCED = ((100, 3), (20, 7), (33, 1))  # (Z, S): trailing wavefront ranges of a workgroup empty / whole workgroups empty


def _layout_case(name, blocks_a, blocks_b, recs, Z, **kw):
    """Operand rows wider than the blocks (junk in between), offsets > 0, ``recs`` = (a block, b block, d, out_off)."""
    gap = 3
    a_off, off = [], gap
    for w in blocks_a:
        a_off.append(off)
        off += w + gap
    lda = off + 5
    b_off, off = [], 2 * gap
    for w in blocks_b:
        b_off.append(off)
        off += w + gap
    ldb = off + 1
    records, end = [], 0
    for ia, ib, d, oo in recs:
        M, N = blocks_a[ia] // d, blocks_b[ib] // d
        records.append((a_off[ia], b_off[ib], M, N, d, oo))
        end = max(end, oo + M * N)
    return Case(name, Z, tuple(records), lda, ldb, end + 7, **kw)


def _layout_cases():
    out = []
    for tag, m in (("narrow", 40), ("wide", 100)):
        # A block 0 (m x 3) feeds records 0 and 2; output gaps before, between and after the records
        blocks_a, blocks_b = (m * 3, 33), (27 * 3, 65, 70 * 3)
        recs = ((0, 0, 3, 11), (1, 1, 1, 11 + m * 27 + 5), (0, 2, 3, 11 + m * 27 + 5 + 33 * 65 + 9))
        for T, types in ((1, "none"), (5, "random")):
            out.append(_layout_case(f"layout-{tag}-T{T}", blocks_a, blocks_b, recs, 277, T=T, types=types))
            out.append(dataclasses.replace(out[-1], name=f"layout-{tag}-T{T}-S5", Z=150, S=5))
    return out


def _exact_cases():
    out = []
    for tab, blocks in TABLES.items():
        out.append(_case(f"{tab}-T1", 277, blocks))
        for lay in LAYOUTS:
            out.append(_case(f"{tab}-T5-{lay}", 277, blocks, T=5, types=lay))
    for Z in ROW_EDGES:
        for tag, blocks in (("narrow", NARROW), ("mixed", MIXED)):
            out.append(_case(f"rows{Z}-{tag}-T1", Z, blocks))
            out.append(_case(f"rows{Z}-{tag}-T5", Z, blocks, T=5, types="random"))
    for Z, S in FORCED:
        for tag, blocks in (("narrow", NARROW), ("mixed", MIXED)):
            out.append(_case(f"forced-Z{Z}-S{S}-{tag}-T1", Z, blocks, S=S))
            out.append(_case(f"forced-Z{Z}-S{S}-{tag}-T5", Z, blocks, T=5, types="random", S=S))
    out += _layout_cases()
    # 64 records in one launch (the limit): narrow, and with one wide record that moves all of them to the wide kernel
    many = tuple((1 + (5 * i) % 33, 1 + (7 * i) % 70, (1, 3)[i % 2]) for i in range(MAX_RECORDS))
    out.append(_case("records64-narrow", 100, many, T=5, types="random"))
    out.append(_case("records64-wide", 100, many[:-1] + ((70, 9, 1),)))
    return out


EXACT_CASES = _exact_cases()
EXACT_BY_NAME = {c.name: c for c in EXACT_CASES}
assert len(EXACT_BY_NAME) == len(EXACT_CASES)
assert all(c.Z * max(r[4] for r in c.records) * 64 < 2 ** 24 for c in EXACT_CASES)

ACCURACY_SHAPES = {
    "dense128": dict(blocks=((128, 96, 1),), T=1, types="none"),  # wide kernel, both row blocks full
    "typed128": dict(blocks=((128, 80, 3),), T=5, types="random"),  # wide kernel, TYPED, d = 3
    "dense64": dict(blocks=((64, 80, 1),), T=1, types="none"),  # wgrad_kernel<2>
}
ACCURACY_Z = (67, 1000, 4099)
REAL_KINDS = ("randn", "rows", "cols")
ACCURACY_CASES = [_case(f"{shape}-Z{Z}-{kind}", Z, spec["blocks"], T=spec["T"], types=spec["types"], data=kind)
                  for shape, spec in ACCURACY_SHAPES.items() for Z in ACCURACY_Z for kind in REAL_KINDS]


# ---- inputs and references ---------------------------------------------------------------------------------------------------
def _generator(case: Case) -> torch.Generator:
    return torch.Generator().manual_seed(zlib.crc32(case.name.encode()))


def _covered_columns(case: Case, which: int, width: int) -> torch.Tensor:
    mask = torch.zeros(width, dtype=torch.bool)
    for r in case.records:
        rows = r[2] if which == 0 else r[3]
        mask[r[which]:r[which] + rows * r[4]] = True
    return mask


def make_types(case: Case, gen: torch.Generator) -> Optional[torch.Tensor]:
    Z, T = case.Z, case.T
    if case.types == "none":
        return None
    if case.types == "random":
        return torch.randint(0, T, (Z,), generator=gen)
    if case.types == "missing":  # no row has type 2
        t = torch.randint(0, T - 1, (Z,), generator=gen)
        return t + (t >= 2).long()
    if case.types == "single":
        return torch.full((Z,), 3, dtype=torch.int64)
    if case.types == "sorted":
        return torch.randint(0, T, (Z,), generator=gen).sort().values
    if case.types == "alternating":
        return torch.arange(Z) % T
    raise ValueError(case.types)


def make_inputs(case: Case):
    """``a [Z, lda]``, ``b [Z, ldb]`` (float32) and ``types`` (int64 or None) on the CPU, a function of the case's name."""
    gen = _generator(case)
    Z = case.Z
    if case.data == "exact":
        a = torch.randint(-8, 9, (Z, case.lda), generator=gen).float()
        b = torch.randint(-8, 9, (Z, case.ldb), generator=gen).float()
        # columns no record reads: large integers (a read that strays there cannot stay unnoticed)
        for x, which in ((a, 0), (b, 1)):
            junk = ~_covered_columns(case, which, x.shape[1])
            x[:, junk] = 1.0e6 + torch.randint(0, 1000, (Z, int(junk.sum())), generator=gen).float()
    else:
        a = torch.randn(Z, case.lda, generator=gen)
        b = torch.randn(Z, case.ldb, generator=gen)
        if case.data == "rows":
            k = torch.randint(-12, 13, (Z, 1), generator=gen).float()
            a, b = a * torch.exp2(k), b * torch.exp2(-k)
        elif case.data == "cols":
            a = a * torch.exp2(torch.randint(-20, 21, (1, case.lda), generator=gen).float())
            b = b * torch.exp2(torch.randint(-20, 21, (1, case.ldb), generator=gen).float())
        elif case.data != "randn":
            raise ValueError(case.data)
    return a, b, make_types(case, gen)


def atb(case: Case, a: torch.Tensor, b: torch.Tensor, types: Optional[torch.Tensor], dtype=torch.float64, matmul=None):
    """``[T, out_stride]`` in ``dtype``, by index: per type the rows of that type, per record ``A_blk^T B_blk`` with the
    ``d`` components folded into the reduction.  Elements no record covers are zero."""
    matmul = matmul or (lambda x, y: x.t() @ y)
    out = torch.zeros(case.T, case.out_stride, dtype=dtype)
    for t in range(case.T):
        if case.T > 1:
            idx = (types == t).nonzero().flatten()
            at, bt = a[idx].to(dtype), b[idx].to(dtype)
        else:
            at, bt = a.to(dtype), b.to(dtype)
        n = at.shape[0]
        for ao, bo, M, N, d, oo in case.records:
            ab = at[:, ao:ao + M * d].reshape(n, M, d).transpose(1, 2).reshape(n * d, M)
            bb = bt[:, bo:bo + N * d].reshape(n, N, d).transpose(1, 2).reshape(n * d, N)
            out[t, oo:oo + M * N] = matmul(ab, bb).reshape(-1)
    return out


def covered_mask(case: Case) -> torch.Tensor:
    mask = torch.zeros(case.out_stride, dtype=torch.bool)
    for _, _, M, N, _, oo in case.records:
        mask[oo:oo + M * N] = True
    return mask


# ---- launches ------------------------------------------------------------------------------------------------------------------
def table_buffer(records):
    raw = b"".join(struct.pack("<6i", *r) for r in records)
    return ctypes.create_string_buffer(raw, max(len(raw), 1))


def launch(case: Case, a, b, types, device):
    """The kernel's result ``[T, out_stride]`` as float64 on the CPU, and the untouched-partials check of forced-S
    launches (a list of failure strings)."""
    from nequip_amd import _lib
    from nequip_amd.utils import wgrad as wg

    ad, bd = a.to(device), b.to(device)
    td = types.to(device) if types is not None else None
    if case.S is None:
        got = wg.wgrad(ad, bd, wg.WgradTable(case.records, case.out_stride), td, case.T)
        return got.cpu().double(), []
    lib = _lib.load()
    buf = table_buffer(case.records)
    partials = torch.full((case.S, case.T, case.out_stride), SENTINEL, dtype=torch.float32, device=device)
    rc = lib.nqa_wgrad(_lib.NQA_F32, _lib.ptr(ad), _lib.ptr(bd), _lib.ptr(td if case.T > 1 else None),
                       ctypes.cast(buf, ctypes.c_void_p), len(case.records), case.lda, case.ldb, case.Z, case.T,
                       case.out_stride, case.S, _lib.ptr(partials), _lib.stream_ptr(device))
    _lib.check(rc, "nqa_wgrad")
    torch.cuda.synchronize(device)
    p = partials.cpu().double()
    cov = covered_mask(case)
    fails = []
    if not torch.equal(p[:, :, ~cov], torch.full_like(p[:, :, ~cov], SENTINEL)):
        fails.append(f"{case.name}: partial elements outside every record were written")
    got = p.sum(0)  # float64, on the host
    got[:, ~cov] = 0.0
    return got, fails


def check_exact(case: Case, device):
    """Failure strings of one exact-data case (empty: bit-for-bit equal to the float64 reference, gaps zero)."""
    assert case.data == "exact"
    a, b, types = make_inputs(case)
    ref = atb(case, a, b, types)
    got, fails = launch(case, a, b, types, device)
    if got.shape != ref.shape:
        return fails + [f"{case.name}: shape {tuple(got.shape)} != {tuple(ref.shape)}"]
    cov = covered_mask(case)
    if torch.count_nonzero(got[:, ~cov]):
        fails.append(f"{case.name}: output gaps are not zero")
    if not torch.equal(got, ref):
        for i, (_, _, M, N, d, oo) in enumerate(case.records):
            bad = (got[:, oo:oo + M * N] != ref[:, oo:oo + M * N]).reshape(case.T, M, N)
            if bad.any():
                t, r, c = (int(v) for v in bad.nonzero()[0])
                fails.append(f"{case.name}: record {i} (M={M} N={N} d={d}): {int(bad.sum())} of {bad.numel()} elements "
                             f"differ, first at type {t} row {r} column {c}: got "
                             f"{float(got[t, oo + r * N + c])} expected {float(ref[t, oo + r * N + c])}")
    return fails


def rho(case: Case, x: torch.Tensor, ref: torch.Tensor, denom: torch.Tensor) -> float:
    """max |x - ref| / (|A|^T |B|) over the covered elements whose denominator is not zero (a type without rows: zero rows
    summed, the result must be exactly zero there)."""
    cov = covered_mask(case).expand_as(ref)
    live = cov & (denom > 0)
    dead = cov & ~live
    if torch.count_nonzero(x[dead]):
        return float("inf")
    return float(((x - ref).abs()[live] / denom[live]).max())


_REAL_CACHE = {}


def real_reference(case: Case):
    """Inputs, float64 reference, |A|^T|B| and rho of the float32 CPU product of a real-data case (computed once)."""
    if case.name not in _REAL_CACHE:
        a, b, types = make_inputs(case)
        ref = atb(case, a, b, types)
        denom = atb(case, a.abs(), b.abs(), types)
        rho32 = rho(case, atb(case, a, b, types, dtype=torch.float32).double(), ref, denom)
        _REAL_CACHE[case.name] = (a, b, types, ref, denom, rho32)
    return _REAL_CACHE[case.name]


def check_accuracy(case: Case, device):
    """-> (failure strings, rho(kernel), rho(float32 CPU)) of one real-data case."""
    a, b, types, ref, denom, rho32 = real_reference(case)
    got, fails = launch(case, a, b, types, device)
    rk = rho(case, got, ref, denom)
    if not rk <= RHO_FACTOR * rho32:
        fails.append(f"{case.name}: rho(kernel) = {rk:.3e} > {RHO_FACTOR} * rho(fp32 CPU) = {rho32:.3e} "
                     f"(ratio {rk / rho32:.2f})")
    return fails, rk, rho32


# ---- CPU emulation of the six-product scheme (mfma_split.h: x = hi + mid + lo in bf16, fp32 products) ------------------------
PRODUCTS = ("mid.mid", "hi.lo", "lo.hi", "hi.mid", "mid.hi", "hi.hi")  # the order of the split form's mfma_bf16 lines


def bf16_planes(x: torch.Tensor):
    hi = x.bfloat16().float()
    r = x - hi
    mid = r.bfloat16().float()
    lo = (r - mid).bfloat16().float()
    return {"hi": hi, "mid": mid, "lo": lo}


def emulate_split(a: torch.Tensor, b: torch.Tensor, drop: Optional[str] = None) -> torch.Tensor:
    """``a^T b`` as the sum of the six (five with ``drop``) bf16 partial products, each an fp32 product, added in fp32."""
    pa, pb = bf16_planes(a), bf16_planes(b)
    acc = torch.zeros(a.shape[1], b.shape[1], dtype=torch.float32)
    for name in PRODUCTS:
        if name != drop:
            x, y = name.split(".")
            acc = acc + pa[x].t() @ pb[y]
    return acc


def emulation_case(Z: int, kind: str) -> Case:
    return _case(f"emulation-Z{Z}-{kind}", Z, ((96, 80, 1),), data=kind)


# ---- the switch -----------------------------------------------------------------------------------------------------------------
SWITCH_SETTINGS = ("0", "1")  # NQA_WGRAD_EXACT_FP32
PROBE_WIDE = ((0, 0, 128, 64, 1, 0),)  # two 64-row tiles in the wide kernel, one 128-row tile on the fp32 path
PROBE_ONE_TILE = ((0, 0, 64, 64, 1, 0),)
# nqa_wgrad_splits(PROBE_WIDE, T = 1, Z = 10^6) and (PROBE_ONE_TILE, 1, 10^5) per exact_fp32
PROBE_LITERALS = {False: (256, 391), True: (512, 391)}


def switches_from_env(env=None):
    """exact_fp32 as ``wgrad.hip`` parses the environment."""
    env = os.environ if env is None else env
    e = env.get("NQA_WGRAD_EXACT_FP32", "")
    return e != "" and e[0] != "0"


def expected_splits(records, T: int, Z: int, exact_fp32: bool) -> int:
    """The formula of ``nqa_wgrad_splits``."""
    max_m = max(r[2] for r in records)
    split = max_m > 64 and not exact_fp32
    rb = 1 if max_m <= 32 else (2 if (max_m <= 64 or split) else 4)
    tiles = T * sum(-(-r[2] // (32 * rb)) * -(-r[3] // 64) for r in records)
    wpu = 4  # wavefronts per partial: the four of a workgroup share one
    S = -(-(2048 // wpu) // tiles)
    return max(1, min(S, -(-Z // (64 * wpu))))


def library_splits(records, T: int, Z: int) -> int:
    from nequip_amd import _lib

    return _lib.load().nqa_wgrad_splits(ctypes.cast(table_buffer(records), ctypes.c_void_p), len(records), T, Z)


def check_switches():
    """Failure strings: did this process's environment switch reach the library?  Host-visible only (the split counts)."""
    exact_fp32 = switches_from_env()
    fails = []
    lit = PROBE_LITERALS[exact_fp32]
    probes = [(PROBE_WIDE, 1, 10 ** 6, lit[0]), (PROBE_ONE_TILE, 1, 10 ** 5, lit[1]),
              (PROBE_WIDE, 1, 10 ** 5, None), (PROBE_WIDE, 5, 10 ** 6, None), (PROBE_ONE_TILE, 1, 10 ** 6, None)]
    for records, T, Z, literal in probes:
        want = expected_splits(records, T, Z, exact_fp32)
        got = library_splits(records, T, Z)
        if literal is not None and want != literal:
            fails.append(f"expected_splits({records}, {T}, {Z}) = {want}, the literal says {literal}")
        if got != want:
            fails.append(f"nqa_wgrad_splits({records}, {T}, {Z}) = {got}, expected {want} for exact_fp32={exact_fp32}")
    return fails


def child_env(exact_fp32: str):
    return dict(os.environ, NQA_WGRAD_EXACT_FP32=exact_fp32)


def child_command(entry: str):
    code = f"import sys; sys.path.insert(0, {os.path.dirname(os.path.abspath(__file__))!r}); import wgrad_cases; " \
           f"sys.exit(wgrad_cases.{entry}())"
    return [sys.executable, "-c", code]


def child_host_main() -> int:
    """Child process without a GPU: the switch probes only."""
    fails = check_switches()
    for f in fails:
        print("FAIL", f)
    return 1 if fails else 0


def child_gpu_main() -> int:
    """Child process on the GPU: prove the switch took effect, then the exact-data list and the accuracy cases."""
    fails = check_switches()
    if fails:  # the wrong kernels would run: nothing below would mean what it claims
        for f in fails:
            print("FAIL", f)
        return 1
    device = torch.device("cuda:0")
    setting = "exact_fp32=%d" % switches_from_env()
    for case in EXACT_CASES:
        fails += check_exact(case, device)
    for case in ACCURACY_CASES:
        f, rk, r32 = check_accuracy(case, device)
        print(f"RHO [{setting}] {case.name}: kernel {rk:.3e} fp32-cpu {r32:.3e} ratio {rk / r32:.2f}")
        fails += f
    for f in fails:
        print("FAIL", f)
    print(f"[{setting}] {len(EXACT_CASES)} exact cases, {len(ACCURACY_CASES)} accuracy cases, {len(fails)} failures")
    return 1 if fails else 0
