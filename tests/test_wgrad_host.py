"""Host side of ``nqa_wgrad`` (``nequip_amd/csrc/wgrad.hip``, ``nequip_amd/utils/wgrad.py``) without a GPU: the split count
``nqa_wgrad_splits`` suggests, the calls that ``nqa_wgrad`` refuses before any launch, the environment switch of the
kernel choice (read once per process, so probed in child processes), ``WgradTable.covered``, and the CPU emulation of the
six-product bf16 split that shows the accuracy bound of ``tests/test_wgrad.py`` can fail."""

import ctypes
import subprocess

import pytest
import torch

import wgrad_cases as wc

ERR_INVALID, ERR_UNSUPPORTED = -1, -2


def _lib():
    from nequip_amd import _lib

    return _lib


def _tab(records):
    return ctypes.cast(wc.table_buffer(records), ctypes.c_void_p), len(records)


def test_return_codes_match_the_header():
    import os
    import re

    text = open(os.path.join(wc.ROOT, "include", "nequip_amd.h")).read()
    assert int(re.search(r"NQA_ERR_INVALID\s*=?\s*(-?\d+)", text).group(1)) == ERR_INVALID
    assert int(re.search(r"NQA_ERR_UNSUPPORTED\s*=?\s*(-?\d+)", text).group(1)) == ERR_UNSUPPORTED


TABLES = [((0, 0, 8, 8, 1, 0),), ((0, 0, 32, 64, 1, 0),), ((0, 0, 64, 65, 3, 0),), wc.PROBE_WIDE, ((0, 0, 128, 704, 1, 0),),
          wc.packed(wc.MIXED)[0], wc.packed(wc.TABLES["split0"])[0]]


def test_splits_bounds_and_formula():
    """1 <= S <= ceil(Z / (64 wpu)) for Z > 0, S = 1 for Z = 0, and the documented formula -- for the switch of this
    process, whatever it is."""
    exact_fp32 = wc.switches_from_env()
    wpu = 4
    for records in TABLES:
        for T in (1, 5):
            for Z in (0, 1, 63, 64, 65, 255, 256, 257, 1000, 4099, 10 ** 5, 10 ** 6, 10 ** 9):
                S = wc.library_splits(records, T, Z)
                assert S >= 1, (records, T, Z, S)
                if Z > 0:
                    assert S <= -(-Z // (64 * wpu)), (records, T, Z, S)
                assert S == wc.expected_splits(records, T, Z, exact_fp32), (records, T, Z, S)


def test_splits_do_not_grow_with_the_tile_count():
    for Z in (1000, 10 ** 5, 10 ** 6):
        last = None
        for n in (1, 2, 3, 7, 20, 64):  # n records of one 64 x 64 tile each, then more types
            for T in (1, 2, 5):
                S = wc.library_splits(wc.packed(((64, 64, 1),) * n)[0], T, Z)
                if T == 1:
                    assert last is None or S <= last, (Z, n, S, last)
                    last = S
                else:
                    assert S <= last, (Z, n, T, S, last)
        by_n = [wc.library_splits(((0, 0, 64, N, 1, 0),), 1, Z) for N in (1, 64, 65, 128, 129, 704)]
        assert by_n == sorted(by_n, reverse=True), (Z, by_n)


def test_splits_refuses_invalid_tables():
    lib = _lib().load()
    tab, n = _tab(wc.PROBE_WIDE)
    assert lib.nqa_wgrad_splits(None, 1, 1, 100) == ERR_INVALID
    assert lib.nqa_wgrad_splits(tab, 0, 1, 100) == ERR_INVALID
    many, _ = _tab(((0, 0, 8, 8, 1, 0),) * 65)
    assert lib.nqa_wgrad_splits(many, 65, 1, 100) == ERR_INVALID
    assert lib.nqa_wgrad_splits(many, 64, 1, 100) >= 1
    assert lib.nqa_wgrad_splits(tab, n, 0, 100) == ERR_INVALID
    assert lib.nqa_wgrad_splits(tab, n, 1, -1) == ERR_INVALID


def test_invalid_arguments_are_refused_before_any_launch():
    """``nqa_wgrad`` with rows to reduce and dummy non-null pointers (never dereferenced on the host): every refusal comes
    before the first launch -- this runs without a GPU -- and ``nqa_last_error`` names the cause."""
    L = _lib()
    lib = L.load()
    dummy = ctypes.c_void_p(0x1000)

    def call(records, dtype=L.NQA_F32, types=None, lda=64, ldb=64, Z=100, T=1, stride=64 * 64, n=None, S=2):
        tab, count = _tab(records)
        rc = lib.nqa_wgrad(dtype, dummy, dummy, types, tab, count if n is None else n, lda, ldb, Z, T, stride, S, dummy, None)
        return rc, lib.nqa_last_error() or b""

    ok = ((0, 0, 64, 64, 1, 0),)
    rc, msg = call(ok, dtype=L.NQA_F64)
    assert rc == ERR_UNSUPPORTED and b"float32" in msg
    rc, msg = call(ok, T=3, types=None)
    assert rc == ERR_INVALID and b"row_types" in msg
    rc, msg = call(ok, lda=(1 << 24) + 1)
    assert rc == ERR_INVALID and b"lda" in msg and b"2^24" in msg
    rc, msg = call(ok, ldb=(1 << 24) + 1)
    assert rc == ERR_INVALID and b"ldb" in msg
    rc, msg = call(((1, 0, 64, 64, 1, 0),))  # a_off + M*d = 65 > lda
    assert rc == ERR_INVALID and b"instruction 0 runs past lda" in msg
    rc, msg = call(ok + ((0, 0, 16, 22, 3, 0),), stride=64 * 64)  # N*d = 66 > ldb, in the second record
    assert rc == ERR_INVALID and b"instruction 1 runs past ldb" in msg
    rc, msg = call(((0, 0, 64, 64, 1, 1),))  # out_off + M*N = stride + 1
    assert rc == ERR_INVALID and b"runs past out_stride" in msg
    rc, msg = call(((0, 0, 64, 64, 0, 0),))
    assert rc == ERR_INVALID and b"d < 1" in msg
    rc, msg = call(((0, 0, 8, 8, 1, 0),) * 65)
    assert rc == ERR_INVALID and b"64 records" in msg
    rc, msg = call(ok, n=0)
    assert rc == ERR_INVALID and b"64 records" in msg
    rc, msg = call(ok, S=0)
    assert rc == ERR_INVALID


def test_expected_splits_literals():
    """The formula restated in ``wgrad_cases.expected_splits`` against the split counts named in the kernel's design notes:
    M = 128, N = 64 at Z = 10^6 and one tile at Z = 10^5 (there ``ceil(Z / (64 wpu))`` is the limit)."""
    assert set(wc.PROBE_LITERALS) == {False, True}
    for exact_fp32, (wide, one_tile) in wc.PROBE_LITERALS.items():
        assert wc.expected_splits(wc.PROBE_WIDE, 1, 10 ** 6, exact_fp32) == wide
        assert wc.expected_splits(wc.PROBE_ONE_TILE, 1, 10 ** 5, exact_fp32) == one_tile
    assert wc.switches_from_env({}) is False
    assert wc.switches_from_env({"NQA_WGRAD_EXACT_FP32": ""}) is False
    assert wc.switches_from_env({"NQA_WGRAD_EXACT_FP32": "0"}) is False
    assert wc.switches_from_env({"NQA_WGRAD_EXACT_FP32": "1"}) is True


def test_switches_reach_the_library_in_a_fresh_process():
    """The two settings of NQA_WGRAD_EXACT_FP32, one child process after another: each asserts the split counts its setting
    implies.  Stops at the first child that fails."""
    for exact_fp32 in wc.SWITCH_SETTINGS:
        done = subprocess.run(wc.child_command("child_host_main"), timeout=120, env=wc.child_env(exact_fp32),
                              capture_output=True, text=True)
        assert done.returncode == 0, (exact_fp32, done.returncode, done.stdout[-2000:], done.stderr[-2000:])


def test_the_removed_wg_reduce_switch_is_no_longer_honoured():
    """NQA_WGRAD_WG_REDUCE=0 once selected one partial tile per wavefront (split counts 1024 / 1563 and 2048 / 1563 at the
    probes).  The switch is gone: a fresh process with it in the environment still gives the counts of four wavefronts per
    partial, under both settings of the switch that stays."""
    for exact_fp32 in wc.SWITCH_SETTINGS:
        env = dict(wc.child_env(exact_fp32), NQA_WGRAD_WG_REDUCE="0")
        done = subprocess.run(wc.child_command("child_host_main"), timeout=120, env=env, capture_output=True, text=True)
        assert done.returncode == 0, (exact_fp32, done.returncode, done.stdout[-2000:], done.stderr[-2000:])


def test_covered_means_an_exact_tiling():
    from nequip_amd.utils.wgrad import WgradTable

    assert WgradTable([(0, 0, 4, 5, 1, 0), (0, 0, 3, 2, 1, 20)], 26).covered
    assert WgradTable([(0, 0, 3, 2, 1, 20), (0, 0, 4, 5, 1, 0)], 26).covered  # any order
    # equal sums M*N == out_stride that are no tiling: two records at one place, a record missing and a gap of its size
    assert not WgradTable([(0, 0, 4, 5, 1, 0), (0, 0, 4, 5, 1, 0)], 40).covered
    assert not WgradTable([(0, 0, 4, 5, 1, 0), (0, 0, 4, 5, 1, 10)], 40).covered
    assert not WgradTable([(0, 0, 4, 5, 1, 20)], 40).covered
    assert not WgradTable([(0, 0, 4, 5, 1, 0), (0, 0, 4, 5, 1, 21)], 41).covered
    assert not WgradTable([(0, 0, 4, 5, 1, 0)], 26).covered
    assert not WgradTable([(0, 0, 4, 5, 1, 6)], 20).covered
    for case in wc.EXACT_CASES:
        gaps = not bool(wc.covered_mask(case).all())
        assert WgradTable(case.records, case.out_stride).covered == (not gaps), case.name


def test_case_list_reaches_every_shape_the_kernels_branch_on():
    """The case list itself: the widths at which the host picks another kernel, edge tiles of the wide kernel, mixed
    widths, forced splits, and exact data that stays exact (asserted at import)."""
    names = set(wc.EXACT_BY_NAME)
    widest = {max(r[2] for r in c.records) for c in wc.EXACT_CASES}
    assert {8, 32, 33, 64, 100, 130} <= widest
    triples = {(r[2], r[3], r[4]) for c in wc.EXACT_CASES if c.name.startswith("split") for r in c.records}
    assert triples == {(M, N, d) for M in wc.SPLIT_M for N in wc.SPLIT_N for d in wc.SPLIT_D}
    for tab in wc.TABLES:
        assert {f"{tab}-T1"} | {f"{tab}-T5-{lay}" for lay in wc.LAYOUTS} <= names
    assert {c.Z for c in wc.EXACT_CASES if c.name.startswith("rows")} == set(wc.ROW_EDGES)
    assert {(c.Z, c.S) for c in wc.EXACT_CASES if c.name.startswith("forced")} == set(wc.FORCED)
    assert max(len(c.records) for c in wc.EXACT_CASES) == wc.MAX_RECORDS
    assert len(wc.ACCURACY_CASES) == 27
    c = wc.EXACT_BY_NAME["split0-T5-missing"]
    assert 2 not in set(wc.make_inputs(c)[2].tolist()) and len(set(wc.make_inputs(c)[2].tolist())) == 4


@pytest.mark.parametrize("kind", wc.REAL_KINDS)
@pytest.mark.parametrize("Z", wc.ACCURACY_Z)
def test_emulated_split_meets_the_bound_and_every_five_product_variant_misses_it(Z, kind):
    """The six-product scheme (bf16 planes of ``x.bfloat16()``, fp32 products) on the CPU at M = 96, N = 80: within
    ``3 * rho(fp32)``, and outside it as soon as any one partial product is dropped -- the bound of the GPU accuracy
    tests can fail, for the mistake it is there to catch."""
    case = wc.emulation_case(Z, kind)
    a, b, _ = wc.make_inputs(case)
    ref = wc.atb(case, a, b, None)
    denom = wc.atb(case, a.abs(), b.abs(), None)
    rho32 = wc.rho(case, wc.atb(case, a, b, None, dtype=torch.float32).double(), ref, denom)
    full = wc.rho(case, wc.emulate_split(a, b).double().reshape(1, -1), ref, denom)
    print(f"Z={Z} {kind}: rho(fp32) {rho32:.3e}, six products {full / rho32:.2f}x")
    assert full <= wc.RHO_FACTOR * rho32, (full, rho32)
    for drop in wc.PRODUCTS:
        r = wc.rho(case, wc.emulate_split(a, b, drop).double().reshape(1, -1), ref, denom)
        print(f"    without {drop}: {r / rho32:.1f}x")
        assert r > wc.RHO_FACTOR * rho32, (drop, r, rho32)
