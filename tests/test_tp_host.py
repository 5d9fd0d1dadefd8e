"""Host side of the tensor-product scatter (``nequip_amd/csrc/tp_generic.hip``), no GPU: the workspace sizes and the
kernel queries of every prebuilt structure, and the calls that are refused -- or accepted as empty -- before anything
touches the device.

The literals were printed by the library as it was before the host code was folded into one operand filler, one
workspace layout and one driver per family: ``python tests/test_tp_host.py`` prints the three tables from whatever
library is built in the tree, and was run on that commit.  They pin the workspace layout and, for each of the 12 launch
entry points (every ``nqa_tp_scatter_*`` of ``include/nequip_amd.h``), the order of the argument checks, the return
codes and the ``nqa_last_error()`` texts of the C ABI."""

import ctypes
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", "nequip_amd", "csrc"))
import gen_spec  # noqa: E402

F32, F64 = 0, 1
EDGES = (0, 1, 2, 7, 1000, 200278)
MULS = (64, 128)  # 128: two 64-channel chunks per node, so grad_y goes through partial rows in the workspace
BIG = 1 << 40
QUERIES = ("nqa_tp_bwd_edge_workspace_bytes", "nqa_tp_bwd_fused_workspace_bytes", "nqa_tp_bwd_pairs_workspace_bytes")
FLAGS = ("nqa_tp_bwd_pairs_dual_supported", "nqa_tp_fwd_jvp_supported")

# argument names of the launch entry points, in the order of include/nequip_amd.h
HEAD = ("plan", "image", "dtype")
CSR = ("rowptr", "eid", "nbr")
OWNER = ("orow", "oth", "prow", "ein", "eout")
WS = ("ws", "ws_bytes")
ROWS = ("rows", "P")
TAIL = ("N", "E")
ENTRY = {
    "fwd": HEAD + ("x", "y", "w") + CSR + ("out",) + TAIL + ("stream",),
    "bwd_edge": HEAD + ("x", "y", "w", "g") + CSR + ("gw", "gy") + WS + TAIL + ("stream",),
    "bwd_fused": HEAD + ("x", "y", "w", "g") + CSR + ("rowptr2", "eid2", "gw", "gy", "gx") + WS + TAIL + ("stream",),
    "bwd_x": HEAD + ("y", "w", "g") + CSR + ("gx",) + TAIL + ("stream",),
    "bwd_pairs": HEAD + ("x", "y", "w", "g") + OWNER + ("trow", "tslot", "gw", "gy", "gx") + WS + TAIL + ("stream",),
    "bwd_pairs_dual": HEAD + ("x", "xc", "y", "yc", "w", "wc", "g") + OWNER + ("gw", "gy") + WS + TAIL + ("stream",),
    "fwd_jvp": HEAD + ("x", "y", "w", "xc", "yc", "wc") + CSR + ("out",) + TAIL + ROWS + ("stream",),
    "bwd_x_dual": HEAD + ("y", "w", "yc", "wc", "g") + CSR + ("gx",) + TAIL + ROWS + ("stream",),
}
for _family in ("fwd", "bwd_edge", "bwd_fused", "bwd_x"):
    ENTRY[_family + "_paired"] = ENTRY[_family][:-1] + ROWS + ("stream",)
SCALARS = dict(dtype=F32, N=10, E=20, P=10, ws_bytes=BIG, stream=None)
# a NULL here is a valid request (fewer results, an absent cotangent, per-edge weight rows): that call is launched
MAY_BE_NULL = {"bwd_edge": ("gw", "gy"), "bwd_edge_paired": ("gw", "gy"), "bwd_pairs": ("gx",), "bwd_pairs_dual": ("wc",),
               "fwd_jvp": ("xc", "yc", "wc", "rows"), "bwd_x_dual": ("rows",)}
NEEDS_SPEC = ("bwd_fused", "bwd_fused_paired", "bwd_pairs", "bwd_pairs_dual", "fwd_jvp", "bwd_x_dual")

# the plans of the refusals: (feature irreps in, l_max of the harmonics, feature irreps out)
PLANS = {
    "spec": ("128x0e+128x1o+128x2e", 2, "128x0e+128x1o+128x2e"),  # every kernel, the pair kernels unsplit (dual form too)
    "split": ("64x0e+64x1o+64x2e+64x3o", 3, "64x0e+64x1o+64x2e+64x3o"),  # pair kernel split by input block: no dual form
    "generic": ("64x0e+32x1o", 1, "64x0e+32x1o"),  # two multiplicities: no specialised kernel
}


def _native_plan(f_in, lmax, f_out):
    """The plan of a convolution as ``TensorProductScatter`` builds it (``nqa_plan_create``; host only)."""
    from nequip_amd.nn import TensorProductScatter
    from nequip_amd.o3 import Irreps
    from oracle import tp as otp

    e_at = str(Irreps.spherical_harmonics(lmax))
    mid, instructions = otp.build_instructions(f_in, e_at, f_out)
    mid_s = "+".join(f"{m}x{l}{'e' if p == 1 else 'o'}" for m, l, p in mid)
    return TensorProductScatter(Irreps(f_in), Irreps(e_at), Irreps(mid_s), instructions)._plan


def _structure_plans():
    """``(name, mul) -> plan`` for every prebuilt structure at both channel counts, and the plan without one."""
    seen, out = set(), {}
    for name, f_in, lmax, f_out in gen_spec.baseline_irreps():
        st = gen_spec.nequip_structure(f_in, lmax, f_out, name)
        if st.instr and st.key() not in seen:
            seen.add(st.key())
            for mul in MULS:
                out[name, mul] = _native_plan(f_in.replace("1x", f"{mul}x"), lmax, f_out.replace("1x", f"{mul}x"))
    assert len(seen) == len(gen_spec.baseline_structures())
    out["generic", 0] = _native_plan(*PLANS["generic"])
    return out


def _queries(lib, plan):
    """Per dtype: the three workspace sizes over EDGES, then the two kernel queries."""
    return tuple(tuple(tuple(getattr(lib, q)(plan.handle, dt, e) for e in EDGES) for q in QUERIES)
                 + tuple(getattr(lib, f)(plan.handle, dt) for f in FLAGS) for dt in (F32, F64))


def _call(lib, entry, plans, p, plan="spec", **over):
    """One call of ``nqa_tp_scatter_<entry>``: valid arguments (every pointer = the host buffer ``p`` that nothing reads, a
    workspace declared large enough, 10 nodes, 20 edges, 10 pairs) with ``over`` on top."""
    vals = dict(SCALARS, plan=plans[plan].handle if plan else None)
    vals.update(over)
    return getattr(lib, "nqa_tp_scatter_" + entry)(*[vals.get(name, p) for name in ENTRY[entry]])


def _refusals(lib, plans):
    """``(name, call)``: calls that return before the first device call: every one breaks a precondition that is checked
    ahead of the launch."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for entry, names in ENTRY.items():
        paired = entry.endswith("_paired")
        cases = [("null plan", dict(plan=None)), ("null image", dict(image=None)), ("dtype 7", dict(dtype=7)),
                 ("null plan and dtype 7", dict(plan=None, dtype=7)), ("dtype 7 and every operand null",
                                                                      dict({n: None for n in names[3:] if n not in SCALARS}, dtype=7))]
        for n in names[3:]:
            if n not in SCALARS and n != "ws" and n not in MAY_BE_NULL.get(entry, ()):
                cases.append((f"null {n}", {n: None}))
        if "ws" in names:
            cases += [("null workspace", dict(ws=None)), ("one-byte workspace", dict(ws_bytes=1)),
                      ("no workspace bytes", dict(ws_bytes=0)), ("null y and one-byte workspace", dict(y=None, ws_bytes=1))]
        if entry.startswith("bwd_pairs"):
            cases += [("odd edge count", dict(E=21)), ("odd edge count and null y", dict(E=21, y=None)),
                      ("float64", dict(dtype=F64)), ("plan without a specialised kernel", dict(plan="generic"))]
        if entry == "bwd_pairs":
            cases += [("null grad_x and null gw", dict(gx=None, gw=None))]
        if entry == "bwd_pairs_dual":
            cases += [("split pair kernel", dict(plan="split")), ("split pair kernel, null y", dict(plan="split", y=None))]
        if entry in NEEDS_SPEC and not entry.startswith("bwd_pairs"):
            cases += [("float64", dict(dtype=F64)), ("plan without a specialised kernel", dict(plan="generic")),
                      ("plan without a specialised kernel, null y", dict(plan="generic", y=None))]
        if "rows" in names:
            cases += [("num_pairs = 0", dict(P=0)), ("num_pairs = 2^30", dict(P=1 << 30)), ("num_pairs = -1", dict(P=-1))]
        if paired and entry not in NEEDS_SPEC:
            cases += [("plan without a specialised kernel", dict(plan="generic")), ("float64", dict(dtype=F64)),
                      ("plan without a specialised kernel, null y", dict(plan="generic", y=None))]
        if paired:
            cases += [("num_pairs = 0 and null plan", dict(P=0, plan=None)),
                      ("null rows and dtype 7", dict(rows=None, dtype=7))]
        if entry in ("fwd", "fwd_paired", "fwd_jvp"):
            cases += [("num_nodes = -1", dict(N=-1)), ("num_edges = -1", dict(E=-1))]
        if entry == "fwd_jvp":
            cases += [("no cotangent", dict(xc=None, yc=None, wc=None)),
                      ("no cotangent, plan without a specialised kernel", dict(xc=None, yc=None, wc=None, plan="generic"))]
        if entry == "bwd_edge_paired":
            cases += [("no gradient asked for, num_pairs = 0", dict(gw=None, gy=None, P=0))]
        for what, over in cases:
            yield f"{entry}: {what}", (lambda entry=entry, over=over: _call(lib, entry, plans, p, **over))


def _empty(lib, plans):
    """``(name, call)``: calls with nothing to do, which return NQA_OK without a launch."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for entry, names in ENTRY.items():
        null = {n: None for n in names[3:] if n not in SCALARS and n != "rows"}
        yield f"{entry}: no nodes", (lambda entry=entry: _call(lib, entry, plans, p, N=0))
        yield f"{entry}: no nodes, no edges, null operands", (
            lambda entry=entry, null=null: _call(lib, entry, plans, p, N=0, E=0, ws_bytes=0, **null))
        if entry in ("fwd", "bwd_x", "bwd_edge"):
            yield f"{entry}: generic kernels, no nodes, no edges, null operands", (
                lambda entry=entry, null=null: _call(lib, entry, plans, p, plan="generic", N=0, E=0, ws_bytes=0, **null))
        if entry.startswith("bwd_edge"):
            yield f"{entry}: no gradient asked for", (lambda entry=entry: _call(lib, entry, plans, p, gw=None, gy=None))
            yield f"{entry}: no gradient asked for, float64", (
                lambda entry=entry: _call(lib, entry, plans, p, gw=None, gy=None, dtype=F64))
    yield "bwd_edge: generic kernels, no gradient asked for", (
        lambda: _call(lib, "bwd_edge", plans, p, plan="generic", gw=None, gy=None, x=None))


# (name, mul) -> per dtype (float32, float64): bwd_edge / bwd_fused / bwd_pairs workspace bytes over EDGES, then
# nqa_tp_bwd_pairs_dual_supported and nqa_tp_fwd_jvp_supported
WORKSPACE = {('generic', 0): (((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0),
                  ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_first', 64): (((0, 16, 32, 112, 16000, 3204448), (0, 256, 512, 1792, 256000, 51271168),
                      (0, -1, 256, -1, 128000, 25635584), 1, 1),
                     ((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_first', 128): (((0, 32, 64, 224, 32000, 6408896), (0, 768, 1280, 3840, 544000, 108951296),
                       (0, -1, 768, -1, 288000, 57680128), 1, 1),
                      ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_last', 64): (((0, 16, 32, 112, 16000, 3204448), (0, 1024, 2048, 7168, 1024000, 205084672),
                     (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                    ((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_last', 128): (((0, 32, 64, 224, 32000, 6408896), (0, 2304, 4352, 14592, 2080000, 416578304),
                      (0, -1, 2304, -1, 1056000, 211493632), 1, 1),
                     ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_last_k1', 64): (((0, 16, 32, 112, 16000, 3204448), (0, 256, 512, 1792, 256000, 51271168),
                        (0, -1, 256, -1, 128000, 25635584), 1, 1),
                       ((0, 8, 16, 56, 8000, 1602224), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_last_k1', 128): (((0, 32, 64, 224, 32000, 6408896), (0, 768, 1280, 3840, 544000, 108951296),
                         (0, -1, 768, -1, 288000, 57680128), 1, 1),
                        ((0, 16, 32, 112, 16000, 3204448), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_mid', 64): (((0, 32, 64, 224, 32000, 6408896), (0, 1024, 2048, 7168, 1024000, 205084672),
                    (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                   ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1n_mid', 128): (((0, 64, 128, 448, 64000, 12817792), (0, 2304, 4352, 14592, 2080000, 416578304),
                     (0, -1, 2304, -1, 1056000, 211493632), 1, 1),
                    ((0, 128, 256, 896, 128000, 25635584), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1p_last', 64): (((0, 16, 32, 112, 16000, 3204448), (0, 2048, 4096, 14336, 2048000, 410169344),
                     (0, -1, 2048, -1, 1024000, 205084672), 1, 1),
                    ((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1p_last', 128): (((0, 32, 64, 224, 32000, 6408896), (0, 4352, 8448, 28928, 4128000, 826747648),
                      (0, -1, 4352, -1, 2080000, 416578304), 1, 1),
                     ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1p_mid', 64): (((0, 88, 176, 616, 88000, 17624464), (0, 2048, 4096, 14336, 2048000, 410169344),
                    (0, -1, 2048, -1, 1024000, 205084672), 1, 1),
                   ((0, 176, 352, 1232, 176000, 35248928), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1p_mid', 128): (((0, 176, 352, 1232, 176000, 35248928), (0, 4352, 8448, 28928, 4128000, 826747648),
                     (0, -1, 4352, -1, 2080000, 416578304), 1, 1),
                    ((0, 352, 704, 2464, 352000, 70497856), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                     0)),
 ('l1p_second', 64): (((0, 44, 88, 308, 44000, 8812232), (0, 1024, 2048, 7168, 1024000, 205084672),
                       (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                      ((0, 88, 176, 616, 88000, 17624464), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l1p_second', 128): (((0, 88, 176, 616, 88000, 17624464), (0, 2304, 4352, 14592, 2080000, 416578304),
                        (0, -1, 2304, -1, 1056000, 211493632), 1, 1),
                       ((0, 176, 352, 1232, 176000, 35248928), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                        0)),
 ('l2n_first', 64): (((0, 36, 72, 252, 36000, 7210008), (0, 256, 512, 1792, 256000, 51271168),
                      (0, -1, 256, -1, 128000, 25635584), 1, 1),
                     ((0, 72, 144, 504, 72000, 14420016), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2n_first', 128): (((0, 72, 144, 504, 72000, 14420016), (0, 768, 1280, 4096, 584192, 116962560),
                       (0, -1, 768, -1, 328192, 65691392), 1, 1),
                      ((0, 144, 288, 1008, 144000, 28840032), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l2n_last', 64): (((0, 36, 72, 252, 36000, 7210008), (0, 2304, 4608, 16128, 2304000, 461440512),
                     (0, -1, 2304, -1, 1152000, 230720256), 1, 1),
                    ((0, 72, 144, 504, 72000, 14420016), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2n_last', 128): (((0, 72, 144, 504, 72000, 14420016), (0, 4864, 9472, 32768, 4680192, 937301248),
                      (0, -1, 4864, -1, 2376192, 475860736), 1, 1),
                     ((0, 144, 288, 1008, 144000, 28840032), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l2n_last_k1', 64): (((0, 36, 72, 252, 36000, 7210008), (0, 256, 512, 1792, 256000, 51271168),
                        (0, -1, 256, -1, 128000, 25635584), 1, 1),
                       ((0, 8, 16, 56, 8000, 1602224), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2n_last_k1', 128): (((0, 72, 144, 504, 72000, 14420016), (0, 768, 1280, 4096, 584192, 116962560),
                         (0, -1, 768, -1, 328192, 65691392), 1, 1),
                        ((0, 16, 32, 112, 16000, 3204448), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2n_last_k2', 64): (((0, 36, 72, 252, 36000, 7210008), (0, 1024, 2048, 7168, 1024000, 205084672),
                        (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                       ((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2n_last_k2', 128): (((0, 72, 144, 504, 72000, 14420016), (0, 2304, 4352, 14848, 2120192, 424589568),
                         (0, -1, 2304, -1, 1096192, 219504896), 1, 1),
                        ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                         0)),
 ('l2n_mid', 64): (((0, 140, 280, 980, 140000, 28038920), (0, 2304, 4608, 16128, 2304000, 461440512),
                    (0, -1, 2304, -1, 1152000, 230720256), 1, 1),
                   ((0, 280, 560, 1960, 280000, 56077840), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2n_mid', 128): (((0, 280, 560, 1960, 280000, 56077840), (0, 4864, 9472, 32768, 4680192, 937301248),
                     (0, -1, 4864, -1, 2376192, 475860736), 1, 1),
                    ((0, 560, 1120, 3920, 560000, 112155680), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                     0)),
 ('l2n_mid_k2', 64): (((0, 84, 168, 588, 84000, 16823352), (0, 1024, 2048, 7168, 1024000, 205084672),
                       (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                      ((0, 168, 336, 1176, 168000, 33646704), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l2n_mid_k2', 128): (((0, 168, 336, 1176, 168000, 33646704), (0, 2304, 4352, 14848, 2120192, 424589568),
                        (0, -1, 2304, -1, 1096192, 219504896), 1, 1),
                       ((0, 336, 672, 2352, 336000, 67293408), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                        0)),
 ('l2p_last', 64): (((0, 36, 72, 252, 36000, 7210008), (0, 4608, 9216, 32256, 4608000, 922881024),
                     (0, -1, 4608, -1, 2304000, 461440512), 1, 1),
                    ((0, 72, 144, 504, 72000, 14420016), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l2p_last', 128): (((0, 72, 144, 504, 72000, 14420016), (0, 9472, 18688, 65024, 9288192, 1860182272),
                      (0, -1, 9472, -1, 4680192, 937301248), 1, 1),
                     ((0, 144, 288, 1008, 144000, 28840032), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l2p_mid', 64): (((0, 408, 816, 2856, 408000, 81713424), (0, 4608, 9216, 32256, 4608000, 922881024),
                    (0, -1, 5120, -1, 2484224, 497490688), 0, 1),
                   ((0, 816, 1632, 5712, 816000, 163426848), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                    0)),
 ('l2p_mid', 128): (((0, 816, 1632, 5712, 816000, 163426848), (0, 9472, 18688, 65024, 9288192, 1860182272),
                     (0, -1, 9984, -1, 4968192, 994981120), 0, 1),
                    ((0, 1632, 3264, 11424, 1632000, 326853696), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                     0, 0)),
 ('l2p_second', 64): (((0, 204, 408, 1428, 204000, 40856712), (0, 2304, 4608, 16128, 2304000, 461440512),
                       (0, -1, 2560, -1, 1260032, 252350464), 0, 1),
                      ((0, 408, 816, 2856, 408000, 81713424), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l2p_second', 128): (((0, 408, 816, 2856, 408000, 81713424), (0, 4864, 9472, 32768, 4680192, 937301248),
                        (0, -1, 5120, -1, 2520064, 504700672), 0, 1),
                       ((0, 816, 1632, 5712, 816000, 163426848), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                        0, 0)),
 ('l3n_first', 64): (((0, 64, 128, 448, 64000, 12817792), (0, 256, 512, 1792, 256000, 51271168),
                      (0, -1, 256, -1, 128000, 25635584), 1, 1),
                     ((0, 128, 256, 896, 128000, 25635584), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l3n_first', 128): (((0, 128, 256, 896, 128000, 25635584), (0, 768, 1280, 4608, 640000, 128177920),
                       (0, -1, 768, -1, 384000, 76906752), 1, 1),
                      ((0, 256, 512, 1792, 256000, 51271168), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l3n_last', 64): (((0, 64, 128, 448, 64000, 12817792), (0, 4096, 8192, 28672, 4096000, 820338688),
                     (0, -1, 4096, -1, 2048000, 410169344), 1, 1),
                    ((0, 128, 256, 896, 128000, 25635584), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l3n_last', 128): (((0, 128, 256, 896, 128000, 25635584), (0, 8448, 16640, 58368, 8320000, 1666312960),
                      (0, -1, 8448, -1, 4224000, 845974272), 1, 1),
                     ((0, 256, 512, 1792, 256000, 51271168), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l3n_last_k1', 64): (((0, 64, 128, 448, 64000, 12817792), (0, 256, 512, 1792, 256000, 51271168),
                        (0, -1, 256, -1, 128000, 25635584), 1, 1),
                       ((0, 8, 16, 56, 8000, 1602224), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l3n_last_k1', 128): (((0, 128, 256, 896, 128000, 25635584), (0, 768, 1280, 4608, 640000, 128177920),
                         (0, -1, 768, -1, 384000, 76906752), 1, 1),
                        ((0, 16, 32, 112, 16000, 3204448), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l3n_last_k2', 64): (((0, 64, 128, 448, 64000, 12817792), (0, 1024, 2048, 7168, 1024000, 205084672),
                        (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                       ((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l3n_last_k2', 128): (((0, 128, 256, 896, 128000, 25635584), (0, 2304, 4352, 15360, 2176000, 435804928),
                         (0, -1, 2304, -1, 1152000, 230720256), 1, 1),
                        ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                         0)),
 ('l3n_last_k3', 64): (((0, 64, 128, 448, 64000, 12817792), (0, 2304, 4608, 16128, 2304000, 461440512),
                        (0, -1, 2304, -1, 1152000, 230720256), 1, 1),
                       ((0, 72, 144, 504, 72000, 14420016), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                        0)),
 ('l3n_last_k3', 128): (((0, 128, 256, 896, 128000, 25635584), (0, 4864, 9472, 33280, 4736000, 948516608),
                         (0, -1, 4864, -1, 2432000, 487076096), 1, 1),
                        ((0, 144, 288, 1008, 144000, 28840032), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                         0)),
 ('l3n_mid', 64): (((0, 396, 792, 2772, 396000, 79310088), (0, 4096, 8192, 28672, 4096000, 820338688),
                    (0, -1, 4608, -1, 2304000, 461440512), 0, 1),
                   ((0, 792, 1584, 5544, 792000, 158620176), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                    0)),
 ('l3n_mid', 128): (((0, 792, 1584, 5544, 792000, 158620176), (0, 8448, 16640, 58368, 8320000, 1666312960),
                     (0, -1, 9216, -1, 4608000, 922881024), 0, 1),
                    ((0, 1584, 3168, 11088, 1584000, 317240352), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                     0, 0)),
 ('l3n_mid_k2', 64): (((0, 160, 320, 1120, 160000, 32044480), (0, 1024, 2048, 7168, 1024000, 205084672),
                       (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                      ((0, 320, 640, 2240, 320000, 64088960), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l3n_mid_k2', 128): (((0, 320, 640, 2240, 320000, 64088960), (0, 2304, 4352, 15360, 2176000, 435804928),
                        (0, -1, 2304, -1, 1152000, 230720256), 1, 1),
                       ((0, 640, 1280, 4480, 640000, 128177920), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                        0, 0)),
 ('l3n_mid_k3', 64): (((0, 284, 568, 1988, 284000, 56878952), (0, 2304, 4608, 16128, 2304000, 461440512),
                       (0, -1, 2816, -1, 1344000, 269173760), 0, 1),
                      ((0, 568, 1136, 3976, 568000, 113757904), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l3n_mid_k3', 128): (((0, 568, 1136, 3976, 568000, 113757904), (0, 4864, 9472, 33280, 4736000, 948516608),
                        (0, -1, 5376, -1, 2688000, 538347264), 0, 1),
                       ((0, 1136, 2272, 7952, 1136000, 227515808), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                        0, 0)),
 ('l3p_last', 64): (((0, 64, 128, 448, 64000, 12817792), (0, 8192, 16384, 57344, 8192000, 1640677376),
                     (0, -1, 8192, -1, 4096000, 820338688), 1, 1),
                    ((0, 128, 256, 896, 128000, 25635584), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l3p_last', 128): (((0, 128, 256, 896, 128000, 25635584), (0, 16640, 33024, 115712, 16512000, 3306990336),
                      (0, -1, 16640, -1, 8320000, 1666312960), 1, 1),
                     ((0, 256, 512, 1792, 256000, 51271168), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l3p_mid', 64): (((0, 1248, 2496, 8736, 1248000, 249946944), (0, 8192, 16384, 57344, 8192000, 1640677376),
                    (-1, -1, -1, -1, -1, -1), 0, 1),
                   ((0, 2496, 4992, 17472, 2496000, 499893888), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                    0)),
 ('l3p_mid', 128): (((0, 2496, 4992, 17472, 2496000, 499893888), (0, 16640, 33024, 115712, 16512000, 3306990336),
                     (-1, -1, -1, -1, -1, -1), 0, 1),
                    ((0, 4992, 9984, 34944, 4992000, 999787776), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                     0, 0)),
 ('l3p_second', 64): (((0, 624, 1248, 4368, 624000, 124973472), (0, 4096, 8192, 28672, 4096000, 820338688),
                       (-1, -1, -1, -1, -1, -1), 0, 1),
                      ((0, 1248, 2496, 8736, 1248000, 249946944), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                       0, 0)),
 ('l3p_second', 128): (((0, 1248, 2496, 8736, 1248000, 249946944), (0, 8448, 16640, 58368, 8320000, 1666312960),
                        (-1, -1, -1, -1, -1, -1), 0, 1),
                       ((0, 2496, 4992, 17472, 2496000, 499893888), (-1, -1, -1, -1, -1, -1),
                        (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l4n_first', 64): (((0, 100, 200, 700, 100000, 20027800), (0, 256, 512, 1792, 256000, 51271168),
                      (0, -1, 256, -1, 128000, 25635584), 1, 1),
                     ((0, 200, 400, 1400, 200000, 40055600), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l4n_first', 128): (((0, 200, 400, 1400, 200000, 40055600), (0, 768, 1536, 5120, 712192, 142598144),
                       (0, -1, 1024, -1, 456192, 91326976), 1, 1),
                      ((0, 400, 800, 2800, 400000, 80111200), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l4n_last', 64): (((0, 100, 200, 700, 100000, 20027800), (0, 6400, 12800, 44800, 6400000, 1281779200),
                     (0, -1, 6400, -1, 3200000, 640889600), 1, 1),
                    ((0, 200, 400, 1400, 200000, 40055600), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                     0)),
 ('l4n_last', 128): (((0, 200, 400, 1400, 200000, 40055600), (0, 13056, 26112, 91136, 13000192, 2603614208),
                      (0, -1, 13312, -1, 6600192, 1321835008), 1, 1),
                     ((0, 400, 800, 2800, 400000, 80111200), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                      0)),
 ('l4n_last_k1', 64): (((0, 100, 200, 700, 100000, 20027800), (0, 256, 512, 1792, 256000, 51271168),
                        (0, -1, 256, -1, 128000, 25635584), 1, 1),
                       ((0, 8, 16, 56, 8000, 1602224), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l4n_last_k1', 128): (((0, 200, 400, 1400, 200000, 40055600), (0, 768, 1536, 5120, 712192, 142598144),
                         (0, -1, 1024, -1, 456192, 91326976), 1, 1),
                        ((0, 16, 32, 112, 16000, 3204448), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l4n_last_k2', 64): (((0, 100, 200, 700, 100000, 20027800), (0, 1024, 2048, 7168, 1024000, 205084672),
                        (0, -1, 1024, -1, 512000, 102542336), 1, 1),
                       ((0, 32, 64, 224, 32000, 6408896), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l4n_last_k2', 128): (((0, 200, 400, 1400, 200000, 40055600), (0, 2304, 4608, 15872, 2248192, 450225152),
                         (0, -1, 2560, -1, 1224192, 245140480), 1, 1),
                        ((0, 64, 128, 448, 64000, 12817792), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                         0)),
 ('l4n_last_k3', 64): (((0, 100, 200, 700, 100000, 20027800), (0, 2304, 4608, 16128, 2304000, 461440512),
                        (0, -1, 2304, -1, 1152000, 230720256), 1, 1),
                       ((0, 72, 144, 504, 72000, 14420016), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                        0)),
 ('l4n_last_k3', 128): (((0, 200, 400, 1400, 200000, 40055600), (0, 4864, 9728, 33792, 4808192, 962936832),
                         (0, -1, 5120, -1, 2504192, 501496320), 1, 1),
                        ((0, 144, 288, 1008, 144000, 28840032), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                         0)),
 ('l4n_last_k4', 64): (((0, 100, 200, 700, 100000, 20027800), (0, 4096, 8192, 28672, 4096000, 820338688),
                        (0, -1, 4096, -1, 2048000, 410169344), 1, 1),
                       ((0, 128, 256, 896, 128000, 25635584), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                        0)),
 ('l4n_last_k4', 128): (((0, 200, 400, 1400, 200000, 40055600), (0, 8448, 16896, 58880, 8392192, 1680733184),
                         (0, -1, 8704, -1, 4296192, 860394496), 1, 1),
                        ((0, 256, 512, 1792, 256000, 51271168), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                         0)),
 ('l4n_mid', 64): (((0, 920, 1840, 6440, 920000, 184255760), (0, 6400, 12800, 44800, 6400000, 1281779200),
                    (-1, -1, -1, -1, -1, -1), 0, 1),
                   ((0, 1840, 3680, 12880, 1840000, 368511520), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                    0)),
 ('l4n_mid', 128): (((0, 1840, 3680, 12880, 1840000, 368511520), (0, 13056, 26112, 91136, 13000192, 2603614208),
                     (-1, -1, -1, -1, -1, -1), 0, 1),
                    ((0, 3680, 7360, 25760, 3680000, 737023040), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                     0, 0)),
 ('l4n_mid_k2', 64): (((0, 260, 520, 1820, 260000, 52072280), (0, 1024, 2048, 7168, 1024000, 205084672),
                       (0, -1, 1536, -1, 712192, 142598144), 0, 1),
                      ((0, 520, 1040, 3640, 520000, 104144560), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l4n_mid_k2', 128): (((0, 520, 1040, 3640, 520000, 104144560), (0, 2304, 4608, 15872, 2248192, 450225152),
                        (0, -1, 3072, -1, 1424128, 285196032), 0, 1),
                       ((0, 1040, 2080, 7280, 1040000, 208289120), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                        0, 0)),
 ('l4n_mid_k3', 64): (((0, 476, 952, 3332, 476000, 95332328), (0, 2304, 4608, 16128, 2304000, 461440512),
                       (-1, -1, -1, -1, -1, -1), 0, 1),
                      ((0, 952, 1904, 6664, 952000, 190664656), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1), 0,
                       0)),
 ('l4n_mid_k3', 128): (((0, 952, 1904, 6664, 952000, 190664656), (0, 4864, 9728, 33792, 4808192, 962936832),
                        (-1, -1, -1, -1, -1, -1), 0, 1),
                       ((0, 1904, 3808, 13328, 1904000, 381329312), (-1, -1, -1, -1, -1, -1),
                        (-1, -1, -1, -1, -1, -1), 0, 0)),
 ('l4n_mid_k4', 64): (((0, 700, 1400, 4900, 700000, 140194600), (0, 4096, 8192, 28672, 4096000, 820338688),
                       (-1, -1, -1, -1, -1, -1), 0, 1),
                      ((0, 1400, 2800, 9800, 1400000, 280389200), (-1, -1, -1, -1, -1, -1), (-1, -1, -1, -1, -1, -1),
                       0, 0)),
 ('l4n_mid_k4', 128): (((0, 1400, 2800, 9800, 1400000, 280389200), (0, 8448, 16896, 58880, 8392192, 1680733184),
                        (-1, -1, -1, -1, -1, -1), 0, 1),
                       ((0, 2800, 5600, 19600, 2800000, 560778400), (-1, -1, -1, -1, -1, -1),
                        (-1, -1, -1, -1, -1, -1), 0, 0))}

REFUSED = {'bwd_edge: dtype 7': (-2, 'nqa_tp_scatter_bwd_edge: unsupported dtype'),
 'bwd_edge: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_bwd_edge: unsupported dtype'),
 'bwd_edge: no workspace bytes': (-4, 'nqa_tp_scatter_bwd_edge: workspace missing or too small'),
 'bwd_edge: null eid': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null g': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null image': (-1, 'nqa_tp_scatter_bwd_edge: NULL plan or plan image'),
 'bwd_edge: null nbr': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null plan': (-1, 'nqa_tp_scatter_bwd_edge: NULL plan or plan image'),
 'bwd_edge: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_edge: NULL plan or plan image'),
 'bwd_edge: null rowptr': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null w': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null workspace': (-4, 'nqa_tp_scatter_bwd_edge: workspace missing or too small'),
 'bwd_edge: null x': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null y': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: null y and one-byte workspace': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge: one-byte workspace': (-4, 'nqa_tp_scatter_bwd_edge: workspace missing or too small'),
 'bwd_edge_paired: dtype 7': (-2, 'nqa_tp_scatter_bwd_edge: unsupported dtype'),
 'bwd_edge_paired: dtype 7 and every operand null': (-1,
                                                     'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs '
                                                     'missing or out of range'),
 'bwd_edge_paired: float64': (-2,
                              'nqa_tp_scatter_bwd_edge_paired: no structure-specialised float32 kernel for this '
                              'plan'),
 'bwd_edge_paired: no gradient asked for, num_pairs = 0': (-1,
                                                           'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs '
                                                           'missing or out of range'),
 'bwd_edge_paired: no workspace bytes': (-4, 'nqa_tp_scatter_bwd_edge: workspace missing or too small'),
 'bwd_edge_paired: null eid': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null g': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null image': (-1, 'nqa_tp_scatter_bwd_edge: NULL plan or plan image'),
 'bwd_edge_paired: null nbr': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null plan': (-1, 'nqa_tp_scatter_bwd_edge: NULL plan or plan image'),
 'bwd_edge_paired: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_edge: NULL plan or plan image'),
 'bwd_edge_paired: null rowptr': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null rows': (-1,
                                'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing or out of range'),
 'bwd_edge_paired: null rows and dtype 7': (-1,
                                            'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing or out '
                                            'of range'),
 'bwd_edge_paired: null w': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null workspace': (-4, 'nqa_tp_scatter_bwd_edge: workspace missing or too small'),
 'bwd_edge_paired: null x': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null y': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: null y and one-byte workspace': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_edge_paired: num_pairs = -1': (-1,
                                     'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing or out of '
                                     'range'),
 'bwd_edge_paired: num_pairs = 0': (-1,
                                    'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing or out of '
                                    'range'),
 'bwd_edge_paired: num_pairs = 0 and null plan': (-1,
                                                  'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing '
                                                  'or out of range'),
 'bwd_edge_paired: num_pairs = 2^30': (-1,
                                       'nqa_tp_scatter_bwd_edge_paired: weight_rows / num_pairs missing or out of '
                                       'range'),
 'bwd_edge_paired: one-byte workspace': (-4, 'nqa_tp_scatter_bwd_edge: workspace missing or too small'),
 'bwd_edge_paired: plan without a specialised kernel': (-2,
                                                        'nqa_tp_scatter_bwd_edge_paired: no structure-specialised '
                                                        'float32 kernel for this plan'),
 'bwd_edge_paired: plan without a specialised kernel, null y': (-1, 'nqa_tp_scatter_bwd_edge: NULL operand'),
 'bwd_fused: dtype 7': (-2, 'nqa_tp_scatter_bwd_fused: unsupported dtype'),
 'bwd_fused: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_bwd_fused: unsupported dtype'),
 'bwd_fused: float64': (-2, 'nqa_tp_scatter_bwd_fused: no structure-specialised float32 kernel for this plan'),
 'bwd_fused: no workspace bytes': (-4, 'nqa_tp_scatter_bwd_fused: workspace missing or too small'),
 'bwd_fused: null eid': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null eid2': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null g': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null gw': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null gx': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null gy': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null image': (-1, 'nqa_tp_scatter_bwd_fused: NULL plan or plan image'),
 'bwd_fused: null nbr': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null plan': (-1, 'nqa_tp_scatter_bwd_fused: NULL plan or plan image'),
 'bwd_fused: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_fused: NULL plan or plan image'),
 'bwd_fused: null rowptr': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null rowptr2': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null w': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null workspace': (-4, 'nqa_tp_scatter_bwd_fused: workspace missing or too small'),
 'bwd_fused: null x': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null y': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: null y and one-byte workspace': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused: one-byte workspace': (-4, 'nqa_tp_scatter_bwd_fused: workspace missing or too small'),
 'bwd_fused: plan without a specialised kernel': (-2,
                                                  'nqa_tp_scatter_bwd_fused: no structure-specialised float32 kernel '
                                                  'for this plan'),
 'bwd_fused: plan without a specialised kernel, null y': (-2,
                                                          'nqa_tp_scatter_bwd_fused: no structure-specialised '
                                                          'float32 kernel for this plan'),
 'bwd_fused_paired: dtype 7': (-2, 'nqa_tp_scatter_bwd_fused: unsupported dtype'),
 'bwd_fused_paired: dtype 7 and every operand null': (-1,
                                                      'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs '
                                                      'missing or out of range'),
 'bwd_fused_paired: float64': (-2, 'nqa_tp_scatter_bwd_fused: no structure-specialised float32 kernel for this plan'),
 'bwd_fused_paired: no workspace bytes': (-4, 'nqa_tp_scatter_bwd_fused: workspace missing or too small'),
 'bwd_fused_paired: null eid': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null eid2': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null g': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null gw': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null gx': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null gy': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null image': (-1, 'nqa_tp_scatter_bwd_fused: NULL plan or plan image'),
 'bwd_fused_paired: null nbr': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null plan': (-1, 'nqa_tp_scatter_bwd_fused: NULL plan or plan image'),
 'bwd_fused_paired: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_fused: NULL plan or plan image'),
 'bwd_fused_paired: null rowptr': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null rowptr2': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null rows': (-1,
                                 'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing or out of range'),
 'bwd_fused_paired: null rows and dtype 7': (-1,
                                             'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing or '
                                             'out of range'),
 'bwd_fused_paired: null w': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null workspace': (-4, 'nqa_tp_scatter_bwd_fused: workspace missing or too small'),
 'bwd_fused_paired: null x': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null y': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: null y and one-byte workspace': (-1, 'nqa_tp_scatter_bwd_fused: NULL operand'),
 'bwd_fused_paired: num_pairs = -1': (-1,
                                      'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing or out of '
                                      'range'),
 'bwd_fused_paired: num_pairs = 0': (-1,
                                     'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing or out of '
                                     'range'),
 'bwd_fused_paired: num_pairs = 0 and null plan': (-1,
                                                   'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing '
                                                   'or out of range'),
 'bwd_fused_paired: num_pairs = 2^30': (-1,
                                        'nqa_tp_scatter_bwd_fused_paired: weight_rows / num_pairs missing or out of '
                                        'range'),
 'bwd_fused_paired: one-byte workspace': (-4, 'nqa_tp_scatter_bwd_fused: workspace missing or too small'),
 'bwd_fused_paired: plan without a specialised kernel': (-2,
                                                         'nqa_tp_scatter_bwd_fused: no structure-specialised float32 '
                                                         'kernel for this plan'),
 'bwd_fused_paired: plan without a specialised kernel, null y': (-2,
                                                                 'nqa_tp_scatter_bwd_fused: no structure-specialised '
                                                                 'float32 kernel for this plan'),
 'bwd_pairs: dtype 7': (-2, 'nqa_tp_scatter_bwd_pairs: unsupported dtype'),
 'bwd_pairs: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_bwd_pairs: unsupported dtype'),
 'bwd_pairs: float64': (-2,
                        'nqa_tp_scatter_bwd_pairs: no pair-centric float32 kernel for this plan (or an odd edge '
                        'count)'),
 'bwd_pairs: no workspace bytes': (-4, 'nqa_tp_scatter_bwd_pairs: workspace missing or too small'),
 'bwd_pairs: null ein': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null eout': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null g': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null grad_x and null gw': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null gw': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null gy': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null image': (-1, 'nqa_tp_scatter_bwd_pairs: NULL plan or plan image'),
 'bwd_pairs: null orow': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null oth': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null plan': (-1, 'nqa_tp_scatter_bwd_pairs: NULL plan or plan image'),
 'bwd_pairs: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_pairs: NULL plan or plan image'),
 'bwd_pairs: null prow': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null trow': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null tslot': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null w': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null workspace': (-4, 'nqa_tp_scatter_bwd_pairs: workspace missing or too small'),
 'bwd_pairs: null x': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null y': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: null y and one-byte workspace': (-1, 'nqa_tp_scatter_bwd_pairs: NULL operand'),
 'bwd_pairs: odd edge count': (-2,
                               'nqa_tp_scatter_bwd_pairs: no pair-centric float32 kernel for this plan (or an odd '
                               'edge count)'),
 'bwd_pairs: odd edge count and null y': (-2,
                                          'nqa_tp_scatter_bwd_pairs: no pair-centric float32 kernel for this plan '
                                          '(or an odd edge count)'),
 'bwd_pairs: one-byte workspace': (-4, 'nqa_tp_scatter_bwd_pairs: workspace missing or too small'),
 'bwd_pairs: plan without a specialised kernel': (-2,
                                                  'nqa_tp_scatter_bwd_pairs: no pair-centric float32 kernel for this '
                                                  'plan (or an odd edge count)'),
 'bwd_pairs_dual: dtype 7': (-2, 'nqa_tp_scatter_bwd_pairs_dual: unsupported dtype'),
 'bwd_pairs_dual: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_bwd_pairs_dual: unsupported dtype'),
 'bwd_pairs_dual: float64': (-2,
                             'nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel for this plan (or an odd '
                             'edge count)'),
 'bwd_pairs_dual: no workspace bytes': (-4, 'nqa_tp_scatter_bwd_pairs_dual: workspace missing or too small'),
 'bwd_pairs_dual: null ein': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null eout': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null g': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null gw': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null gy': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null image': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL plan or plan image'),
 'bwd_pairs_dual: null orow': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null oth': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null plan': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL plan or plan image'),
 'bwd_pairs_dual: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL plan or plan image'),
 'bwd_pairs_dual: null prow': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null w': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null workspace': (-4, 'nqa_tp_scatter_bwd_pairs_dual: workspace missing or too small'),
 'bwd_pairs_dual: null x': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null xc': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null y': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null y and one-byte workspace': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: null yc': (-1, 'nqa_tp_scatter_bwd_pairs_dual: NULL operand'),
 'bwd_pairs_dual: odd edge count': (-2,
                                    'nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel for this plan (or an '
                                    'odd edge count)'),
 'bwd_pairs_dual: odd edge count and null y': (-2,
                                               'nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel for this '
                                               'plan (or an odd edge count)'),
 'bwd_pairs_dual: one-byte workspace': (-4, 'nqa_tp_scatter_bwd_pairs_dual: workspace missing or too small'),
 'bwd_pairs_dual: plan without a specialised kernel': (-2,
                                                       'nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel '
                                                       'for this plan (or an odd edge count)'),
 'bwd_pairs_dual: split pair kernel': (-2,
                                       'nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel for this plan (or '
                                       'an odd edge count)'),
 'bwd_pairs_dual: split pair kernel, null y': (-2,
                                               'nqa_tp_scatter_bwd_pairs_dual: no dual pair-centric kernel for this '
                                               'plan (or an odd edge count)'),
 'bwd_x: dtype 7': (-2, 'nqa_tp_scatter_bwd_x: unsupported dtype'),
 'bwd_x: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_bwd_x: unsupported dtype'),
 'bwd_x: null eid': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x: null g': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x: null gx': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x: null image': (-1, 'nqa_tp_scatter_bwd_x: NULL plan or plan image'),
 'bwd_x: null nbr': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x: null plan': (-1, 'nqa_tp_scatter_bwd_x: NULL plan or plan image'),
 'bwd_x: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_x: NULL plan or plan image'),
 'bwd_x: null rowptr': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x: null w': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x: null y': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_dual: dtype 7': (-2, 'nqa_tp_scatter_bwd_x_dual: unsupported dtype'),
 'bwd_x_dual: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_bwd_x_dual: unsupported dtype'),
 'bwd_x_dual: float64': (-2, 'nqa_tp_scatter_bwd_x_dual: no structure-specialised float32 kernel for this plan'),
 'bwd_x_dual: null eid': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null g': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null gx': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null image': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL plan or plan image'),
 'bwd_x_dual: null nbr': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null plan': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL plan or plan image'),
 'bwd_x_dual: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL plan or plan image'),
 'bwd_x_dual: null rowptr': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null w': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null wc': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null y': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: null yc': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: num_pairs = -1': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: num_pairs = 0': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: num_pairs = 2^30': (-1, 'nqa_tp_scatter_bwd_x_dual: NULL operand'),
 'bwd_x_dual: plan without a specialised kernel': (-2,
                                                   'nqa_tp_scatter_bwd_x_dual: no structure-specialised float32 '
                                                   'kernel for this plan'),
 'bwd_x_dual: plan without a specialised kernel, null y': (-2,
                                                           'nqa_tp_scatter_bwd_x_dual: no structure-specialised '
                                                           'float32 kernel for this plan'),
 'bwd_x_paired: dtype 7': (-2, 'nqa_tp_scatter_bwd_x: unsupported dtype'),
 'bwd_x_paired: dtype 7 and every operand null': (-1,
                                                  'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or '
                                                  'out of range'),
 'bwd_x_paired: float64': (-2, 'nqa_tp_scatter_bwd_x_paired: no structure-specialised float32 kernel for this plan'),
 'bwd_x_paired: null eid': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: null g': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: null gx': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: null image': (-1, 'nqa_tp_scatter_bwd_x: NULL plan or plan image'),
 'bwd_x_paired: null nbr': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: null plan': (-1, 'nqa_tp_scatter_bwd_x: NULL plan or plan image'),
 'bwd_x_paired: null plan and dtype 7': (-1, 'nqa_tp_scatter_bwd_x: NULL plan or plan image'),
 'bwd_x_paired: null rowptr': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: null rows': (-1, 'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out of range'),
 'bwd_x_paired: null rows and dtype 7': (-1,
                                         'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out of '
                                         'range'),
 'bwd_x_paired: null w': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: null y': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'bwd_x_paired: num_pairs = -1': (-1, 'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out of range'),
 'bwd_x_paired: num_pairs = 0': (-1, 'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out of range'),
 'bwd_x_paired: num_pairs = 0 and null plan': (-1,
                                               'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out '
                                               'of range'),
 'bwd_x_paired: num_pairs = 2^30': (-1,
                                    'nqa_tp_scatter_bwd_x_paired: weight_rows / num_pairs missing or out of range'),
 'bwd_x_paired: plan without a specialised kernel': (-2,
                                                     'nqa_tp_scatter_bwd_x_paired: no structure-specialised float32 '
                                                     'kernel for this plan'),
 'bwd_x_paired: plan without a specialised kernel, null y': (-1, 'nqa_tp_scatter_bwd_x: NULL operand'),
 'fwd: dtype 7': (-2, 'nqa_tp_scatter_fwd: unsupported dtype'),
 'fwd: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_fwd: unsupported dtype'),
 'fwd: null eid': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: null image': (-1, 'nqa_tp_scatter_fwd: NULL plan or plan image'),
 'fwd: null nbr': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: null out': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: null plan': (-1, 'nqa_tp_scatter_fwd: NULL plan or plan image'),
 'fwd: null plan and dtype 7': (-1, 'nqa_tp_scatter_fwd: NULL plan or plan image'),
 'fwd: null rowptr': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: null w': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: null x': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: null y': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: num_edges = -1': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd: num_nodes = -1': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_jvp: dtype 7': (-2, 'nqa_tp_scatter_fwd_jvp: unsupported dtype'),
 'fwd_jvp: dtype 7 and every operand null': (-2, 'nqa_tp_scatter_fwd_jvp: unsupported dtype'),
 'fwd_jvp: float64': (-2, 'nqa_tp_scatter_fwd_jvp: no structure-specialised float32 kernel for this plan'),
 'fwd_jvp: no cotangent': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: no cotangent, plan without a specialised kernel': (-2,
                                                              'nqa_tp_scatter_fwd_jvp: no structure-specialised '
                                                              'float32 kernel for this plan'),
 'fwd_jvp: null eid': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: null image': (-1, 'nqa_tp_scatter_fwd_jvp: NULL plan or plan image'),
 'fwd_jvp: null nbr': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: null out': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: null plan': (-1, 'nqa_tp_scatter_fwd_jvp: NULL plan or plan image'),
 'fwd_jvp: null plan and dtype 7': (-1, 'nqa_tp_scatter_fwd_jvp: NULL plan or plan image'),
 'fwd_jvp: null rowptr': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: null w': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: null x': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: null y': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: num_edges = -1': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: num_nodes = -1': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: num_pairs = -1': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: num_pairs = 0': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: num_pairs = 2^30': (-1, 'nqa_tp_scatter_fwd_jvp: NULL operand (at least one cotangent is required)'),
 'fwd_jvp: plan without a specialised kernel': (-2,
                                                'nqa_tp_scatter_fwd_jvp: no structure-specialised float32 kernel for '
                                                'this plan'),
 'fwd_jvp: plan without a specialised kernel, null y': (-2,
                                                        'nqa_tp_scatter_fwd_jvp: no structure-specialised float32 '
                                                        'kernel for this plan'),
 'fwd_paired: dtype 7': (-2, 'nqa_tp_scatter_fwd: unsupported dtype'),
 'fwd_paired: dtype 7 and every operand null': (-1,
                                                'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out '
                                                'of range'),
 'fwd_paired: float64': (-2, 'nqa_tp_scatter_fwd_paired: no structure-specialised float32 kernel for this plan'),
 'fwd_paired: null eid': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: null image': (-1, 'nqa_tp_scatter_fwd: NULL plan or plan image'),
 'fwd_paired: null nbr': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: null out': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: null plan': (-1, 'nqa_tp_scatter_fwd: NULL plan or plan image'),
 'fwd_paired: null plan and dtype 7': (-1, 'nqa_tp_scatter_fwd: NULL plan or plan image'),
 'fwd_paired: null rowptr': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: null rows': (-1, 'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of range'),
 'fwd_paired: null rows and dtype 7': (-1,
                                       'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of range'),
 'fwd_paired: null w': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: null x': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: null y': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: num_edges = -1': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: num_nodes = -1': (-1, 'nqa_tp_scatter_fwd: NULL operand'),
 'fwd_paired: num_pairs = -1': (-1, 'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of range'),
 'fwd_paired: num_pairs = 0': (-1, 'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of range'),
 'fwd_paired: num_pairs = 0 and null plan': (-1,
                                             'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of '
                                             'range'),
 'fwd_paired: num_pairs = 2^30': (-1, 'nqa_tp_scatter_fwd_paired: weight_rows / num_pairs missing or out of range'),
 'fwd_paired: plan without a specialised kernel': (-2,
                                                   'nqa_tp_scatter_fwd_paired: no structure-specialised float32 '
                                                   'kernel for this plan'),
 'fwd_paired: plan without a specialised kernel, null y': (-1, 'nqa_tp_scatter_fwd: NULL operand')}


def _refusal_plans():
    return {k: _native_plan(*v) for k, v in PLANS.items()}


def test_every_launch_entry_point_of_the_header_is_covered():
    header = open(os.path.join(HERE, "..", "include", "nequip_amd.h")).read()
    declared = set(re.findall(r"\bnqa_tp_scatter_(\w+)\s*\(", header))
    assert declared == set(ENTRY) and len(ENTRY) == 12
    from nequip_amd import _lib

    for entry, names in ENTRY.items():  # (and the argument lists above are the header's)
        assert len(_lib.SIGNATURES["nqa_tp_scatter_" + entry][1]) == len(names), entry


def test_workspace_bytes_and_kernel_queries_of_every_structure():
    from nequip_amd import _lib

    lib = _lib.load()
    plans = _structure_plans()
    assert set(plans) == set(WORKSPACE)
    for key, plan in plans.items():
        assert _queries(lib, plan) == WORKSPACE[key], key
    for q in QUERIES + FLAGS:  # no plan, a negative edge count
        assert getattr(lib, q)(None, F32, *(() if q in FLAGS else (8,))) == (0 if q in FLAGS else -1), q
    for q in QUERIES:
        assert getattr(lib, q)(plans["l2n_mid", 64].handle, F32, -2) == -1, q
    # the plan without a specialised kernel: the generic bwd_edge workspace only
    f32, f64 = WORKSPACE["generic", 0]
    assert f32[1] == f32[2] == (-1,) * len(EDGES) and f32[3:] == (0, 0) and all(2 * a == b for a, b in zip(f32[0], f64[0]))
    # the partial rows are padded to whole 256-byte units in front of the grad_x rows; one chunk per node needs none
    for (name, mul), (f32, f64) in WORKSPACE.items():
        assert f64[1] == f64[2] == (-1,) * len(EDGES) and f64[3:] == (0, 0), name
        if mul == 64 and name != "generic":
            assert f32[1][2] % 4 == 0 and f32[1][0] == 0 and f32[1][4] == 500 * f32[1][2], name


def test_calls_refused_before_the_device_is_touched():
    from nequip_amd import _lib

    lib = _lib.load()
    plans = _refusal_plans()
    seen = []
    for name, call in _refusals(lib, plans):
        rc = call()
        assert rc in (-1, -2, -4) and (rc, lib.nqa_last_error().decode()) == REFUSED[name], name  # (-3 would be a launch)
        seen.append(name)
    assert sorted(seen) == sorted(REFUSED)


def test_empty_calls_are_accepted_without_a_launch():
    from nequip_amd import _lib

    lib = _lib.load()
    plans = _refusal_plans()
    for name, call in _empty(lib, plans):
        assert call() == _lib.NQA_OK, name


if __name__ == "__main__":  # print the tables from the library that is built in the tree
    import pprint

    sys.path.insert(0, os.path.join(HERE, ".."))
    from nequip_amd import _lib as _l

    _lib_ = _l.load()
    print("WORKSPACE = " + pprint.pformat({k: _queries(_lib_, v) for k, v in _structure_plans().items()}, width=120, compact=True))
    _plans = _refusal_plans()
    _out = {}
    for _name, _fn in _refusals(_lib_, _plans):
        _rc = _fn()
        _out[_name] = (_rc, _lib_.nqa_last_error().decode())
    print("REFUSED = " + pprint.pformat(_out, width=120))
    print("EMPTY = " + pprint.pformat({_name: _fn() for _name, _fn in _empty(_lib_, _plans)}, width=120))
