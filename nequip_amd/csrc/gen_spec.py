#!/usr/bin/env python3
"""Generate path-structure-specialised tensor-product/scatter kernels (one .hip per structure).

The generic kernels (``tp_generic.hip``) visit one instruction per wavefront, so the per-edge operands of a
node are fetched once *per path* and every iteration is a short dependent load chain (latency bound).  For the
uniform-multiplicity structures NequIP actually builds (``nequip/nn/interaction_block.py:89-109``: every
feature irrep has the same ``mul``) this generator emits "edge-outer" kernels instead: one wavefront owns 64
channels of one node, and per edge it issues *all* loads of that edge at once -- the full coalesced weight-row
segment of every path, the complete source-node row and the (scalar) spherical harmonics -- then evaluates every
path from registers with the unrolled Clebsch-Gordan code of ``cg_generated.h``.  All per-node outputs stay in
VGPRs across the neighbour loop and are stored once.

A structure is: the ``l`` of each in1 / in2 / out irrep and the instruction triples; ``mul`` is a runtime
argument (offsets scale with it), so one kernel serves 32/64/128... features.  ``STRUCTURES`` lists what is
prebuilt (the BASELINE model shapes); plans whose structure is not listed run on the generic kernels.
"""

from __future__ import annotations

import hashlib
import itertools
import os
import sys
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(HERE, "..", "..")))

import numpy as np  # noqa: E402

from nequip_amd.o3.irreps import Irreps  # noqa: E402
from nequip_amd.o3.wigner import wigner_3j  # noqa: E402


class Structure:
    def __init__(self, in1_ls: Sequence[int], in2_ls: Sequence[int], out_ls: Sequence[int],
                 instr: Sequence[Tuple[int, int, int]], name: str = ""):
        self.in1_ls = list(in1_ls)
        self.in2_ls = list(in2_ls)
        self.out_ls = list(out_ls)
        self.instr = [tuple(t) for t in instr]
        self.name = name

    def key(self) -> str:
        """Must match ``structure_key`` in plan.cpp."""
        s = "i1:" + ",".join(map(str, self.in1_ls))
        s += "|i2:" + ",".join(map(str, self.in2_ls))
        s += "|o:" + ",".join(map(str, self.out_ls))
        s += "|p:" + ",".join(f"{a}-{b}-{c}" for a, b, c in self.instr)
        return s

    def tag(self) -> str:
        return hashlib.sha1(self.key().encode()).hexdigest()[:12]


def nequip_structure(feature_irreps_in: str, lmax_sh: int, feature_irreps_out: str, name: str) -> Structure:
    """Replay InteractionBlock's instruction construction (interaction_block.py:89-109)."""
    f_in = Irreps(feature_irreps_in)
    e_at = Irreps.spherical_harmonics(lmax_sh)
    f_out = Irreps(feature_irreps_out)
    mid, ins = [], []
    for i, (mul, ir_in) in enumerate(f_in):
        for j, (_, ir_e) in enumerate(e_at):
            for ir_out in ir_in * ir_e:
                if ir_out in f_out:
                    k = len(mid)
                    mid.append((mul, ir_out))
                    ins.append((i, j, k))
    mid_sorted, p, _ = Irreps(mid).sort()
    ins = [(a, b, p[c]) for a, b, c in ins]
    return Structure([ir.l for _, ir in f_in], [ir.l for _, ir in e_at], [ir.l for _, ir in mid_sorted], ins, name)


def baseline_irreps() -> List[Tuple[str, str, int, str]]:
    """(name, feature_irreps_in, lmax_sh, feature_irreps_out) of every prebuilt structure, with ``1x`` multiplicities
    (the kernels take ``mul`` at run time; tests substitute 32 / 64 / 128)."""
    out = []
    for lmax in (1, 2, 3, 4):
        # l_max = 4 (the reference's XL preset, SO(3) irreps only): the full-parity l = 4 structures are not prebuilt
        for parity in ((False, True) if lmax <= 3 else (False,)):
            hidden = "+".join(
                f"1x{l}{'e' if p == 1 else 'o'}"
                for l in range(lmax + 1)
                for p in ((1, -1) if parity else ((1,) if l % 2 == 0 else (-1,)))
            )
            tag = f"l{lmax}{'p' if parity else 'n'}"
            # conv output irreps = scalars (+ gate scalars) + gated, simplified -> same set of (l,p) as hidden
            out.append((f"{tag}_first", "1x0e", lmax, hidden))
            if parity:
                # second layer of a parity model sees only what layer 0 could produce: 0e, 1o, 2e, ...
                reach = "+".join(f"1x{l}{'e' if l % 2 == 0 else 'o'}" for l in range(lmax + 1))
                out.append((f"{tag}_second", reach, lmax, hidden))
                # layer >= 2 input = what the second layer produced (every hidden irrep reachable from `reach`)
                out.append((f"{tag}_mid", hidden, lmax, hidden))
                out.append((f"{tag}_last", hidden, lmax, "1x0e"))
                out.append((f"{tag}_last2", reach, lmax, "1x0e"))
            else:
                out.append((f"{tag}_mid", hidden, lmax, hidden))
                out.append((f"{tag}_last", hidden, lmax, "1x0e"))
                # channel segments of non-uniform multiplicities (the reference's S / M / L presets: num_features
                # [128, 64], [128, 64, 32], [128, 64, 32, 32]; nn/_segmented.py): in the channel range where only the
                # first k input irreps are live the convolution is the uniform one over those k irreps
                hs = hidden.split("+")
                for k in range(1, lmax + 1):
                    out.append((f"{tag}_mid_k{k}", "+".join(hs[:k]), lmax, hidden))
                    out.append((f"{tag}_last_k{k}", "+".join(hs[:k]), lmax, "1x0e"))
    return out


def baseline_structures() -> List[Structure]:
    # de-duplicate by key
    seen, uniq = set(), []
    for name, f_in, lmax, f_out in baseline_irreps():
        s = nequip_structure(f_in, lmax, f_out, name)
        if s.key() not in seen and s.instr:
            seen.add(s.key())
            uniq.append(s)
    return uniq


# --------------------------------------------------------------------------------------------------------------
# Decisions.  Everything the emitters need to know about a structure is settled here, before any code is written.

PAIR_BUDGET = 110  # register estimate 2 OD + 3 XD + NP of the pair kernel (l2p_second at 144 spills 127 registers)
RING_BUDGET = 180  # register estimate of the LDS-ring pair kernel at two wavefronts per SIMD (see plan_structure)
RING_WAVE_BYTES = 20480  # one wavefront's LDS ring: the CU's 160 KB at two wavefronts per SIMD
RING_MAX_CHUNKS = 6
COPY_BYTES = 16  # bytes per lane of one LDS-DMA copy (dword-per-lane reads reach 4.0 TB/s on this part, 16-byte ones 6.7)
SPLIT_MERGE_BUDGET = 70  # merging l_1 = 0 and 1 into one part (budget 102) spilled 82 registers
SPLIT_NOHOIST = 64  # owner-side intermediates above which a split part keeps them per pair (l_1 = 3: 79 spilled registers)


def _cg(l1: int, l2: int, l3: int) -> np.ndarray:
    return np.array(wigner_3j(l1, l2, l3), dtype=np.float64)


def n_owner_terms(st: Structure, paths: Sequence[int]) -> int:
    """Owner-side intermediates T_ij = sum_k C_ijk g_k of the pair kernels: one per (path, i, j) with a non-zero 3j row."""
    n = 0
    for pth in paths:
        b, j, s = st.instr[pth]
        n += int((np.abs(_cg(st.in1_ls[b], st.in2_ls[j], st.out_ls[s])).sum(axis=2) != 0).sum())
    return n


def ring_plan(st: Structure, paths: Sequence[int]):
    """Chunks of one pair's ring image for `paths`: contiguous path ranges plus the chunk of every input block's x row (not
    later than its first use) with the smallest largest chunk, for the fewest chunks (at most RING_MAX_CHUNKS) whose ring of
    chunks + 1 slots fits RING_WAVE_BYTES.  Returns (chunks, slot bytes, path bounds, {block: chunk}), or None.  Sizes are in
    16-byte units: one component of 64 fp32 channels is 16 of them."""
    n = len(paths)
    blocks = sorted({st.instr[p_][0] for p_ in paths})
    units = [16 + 16 * (2 * st.out_ls[st.instr[p_][2]] + 1) for p_ in paths]  # weight + grad_out segments of each path
    xunits = {b_: 16 * (2 * st.in1_ls[b_] + 1) for b_ in blocks}
    yrow_units = (sum(2 * l + 1 for l in st.in2_ls) * 4 + COPY_BYTES - 1) // COPY_BYTES
    first_of = {}
    for k_, p_ in enumerate(paths):
        first_of.setdefault(st.instr[p_][0], k_)
    for C in range(1, min(n, RING_MAX_CHUNKS) + 1):
        best = None
        for cuts in itertools.combinations(range(1, n), C - 1):
            bounds = [0] + list(cuts) + [n]
            chunk_of = [0] * n
            for c_ in range(C):
                for k_ in range(bounds[c_], bounds[c_ + 1]):
                    chunk_of[k_] = c_
            base = [sum(units[bounds[c_]:bounds[c_ + 1]]) for c_ in range(C)]
            base[0] += 2 * yrow_units
            for place in itertools.product(*[range(chunk_of[first_of[b_]] + 1) for b_ in blocks]):
                tot = list(base)
                for b_, c_ in zip(blocks, place):
                    tot[c_] += xunits[b_]
                key = (max(tot), sum(place))
                if best is None or key < best[0]:
                    best = (key, bounds, dict(zip(blocks, place)))
        slot_bytes = best[0][0] * COPY_BYTES
        if RING_WAVE_BYTES // slot_bytes >= C + 1:
            return C, slot_bytes, best[1], best[2]
    return None


@dataclass
class Ring:
    """Layout of one LDS ring: chunk c of a pair holds the paths cpaths[c] (and the x rows of the blocks placed in it)."""
    chunks: int
    slot_bytes: int
    blocks: List[int]
    xplace: Dict[int, int]
    cpaths: List[List[int]]
    lds_off: List[dict]  # per chunk: (kind, id) -> byte offset inside the slot
    dma: List[list]  # per chunk: (kind, lds byte offset, lanes, [(lane_lo, lane_hi, id, unit of the segment at lane_lo)])
    Sgw: List[int]  # stores a chunk is certain to issue: grad_w per path,
    Sgx: List[int]  # the grad_x row components of the blocks that end in it (+ the unwritten components, in the last chunk)
    Sgx_atom: List[int]  # (ATOM: the components no path writes are not touched at all)

    @property
    def slots(self) -> int:
        return self.chunks + 1

    @property
    def copies(self) -> int:
        return sum(len(ins) for ins in self.dma)


def ring_layout(st: Structure, paths: Sequence[int], n_unused: int, last_path: Dict[int, int]) -> Optional[Ring]:
    """Chunk images [w segments][x segments][g segments][y_in][y_out] of the ring planned for `paths` (None: no plan)."""
    plan = ring_plan(st, paths)
    if plan is None:
        return None
    RC, RSLOT, bounds, xplace = plan
    S = sum(2 * l + 1 for l in st.in2_ls)
    yrow_units = (S * 4 + COPY_BYTES - 1) // COPY_BYTES
    blocks = sorted({st.instr[p_][0] for p_ in paths})
    cpaths = [[paths[k_] for k_ in range(bounds[c_], bounds[c_ + 1])] for c_ in range(RC)]
    lds_off, dma = [], []
    for c_ in range(RC):
        streams = {"w": [(p_, 16) for p_ in cpaths[c_]],
                   "x": [(b_, 16 * (2 * st.in1_ls[b_] + 1)) for b_ in blocks if xplace[b_] == c_],
                   "g": [(st.instr[p_][2], 16 * (2 * st.out_ls[st.instr[p_][2]] + 1)) for p_ in cpaths[c_]]}
        offs, ins, pos = {}, [], 0
        for kind in ("w", "x", "g"):
            segs, start = [], 0
            for ident, units in streams[kind]:
                offs[(kind, ident)] = (pos + start) * COPY_BYTES
                segs.append((ident, start, units))
                start += units
            for i0 in range(0, start, 64):
                nl = min(64, start - i0)
                pieces = []
                for ident, sstart, units in segs:
                    lo, hi = max(sstart, i0), min(sstart + units, i0 + nl)
                    if lo < hi:
                        pieces.append((lo - i0, hi - i0, ident, lo - sstart))
                ins.append((kind, (pos + i0) * COPY_BYTES, nl, pieces))
            pos += start
        if c_ == 0:
            offs[("y", "I")] = pos * COPY_BYTES
            ins.append(("yI", pos * COPY_BYTES, S, None))
            pos += yrow_units
            offs[("y", "X")] = pos * COPY_BYTES
            ins.append(("yX", pos * COPY_BYTES, S, None))
            pos += yrow_units
        assert pos * COPY_BYTES <= RSLOT, (st.name, c_, pos * COPY_BYTES, RSLOT)
        lds_off.append(offs)
        dma.append(ins)
    # (the two grad_y stores of the last chunk are not counted: an under-count only shortens the look-ahead by two operations)
    Sgw = [len(cpaths[c_]) for c_ in range(RC)]
    Sgx = [sum(2 * st.in1_ls[b_] + 1 for b_ in blocks if last_path[b_] in cpaths[c_]) for c_ in range(RC)]
    Sgx_atom = list(Sgx)
    Sgx[RC - 1] += n_unused
    ring = Ring(RC, RSLOT, blocks, xplace, cpaths, lds_off, dma, Sgw, Sgx, Sgx_atom)
    assert sum(Sgw) + sum(Sgx) + ring.copies < 64, "vmcnt range"
    return ring


@dataclass
class Plan:
    st: Structure
    NB: int
    NS: int
    NP: int
    XD: int  # dim_in1 / mul
    S: int
    OD: int  # dim_out / mul
    xpre: List[int]
    ypre: List[int]
    opre: List[int]
    coeff: List[float]  # path normalisation
    slot_coeff: List[Optional[float]]  # per output slot (None: no path writes it)
    used_blocks: List[int]
    used_y: List[int]
    used_slots: List[int]
    unused_comps: List[int]  # grad_x components of the input blocks no path reads
    first_path: Dict[int, int]  # input block -> its first / last path (paths are created input-block major)
    last_path: Dict[int, int]
    big: bool
    pair_ok: bool
    ring: Optional[Ring]  # bwd_pair_ring_kernel
    part_paths: List[List[int]]  # bwd_pair_split_kernel: the paths of each part
    pair_parts: int  # 0: no pair kernel, 1: bwd_pair_kernel, > 1: bwd_pair_split_kernel
    split_rings: List[Ring]  # bwd_pair_split_ring_kernel, per part
    ring_flag: int  # registered: 0 no ring kernel, 1 bwd_pair_ring_kernel, 2 bwd_pair_split_ring_kernel


def plan_structure(st: Structure) -> Plan:
    NB, NS, NP = len(st.in1_ls), len(st.out_ls), len(st.instr)
    xpre = [sum(2 * l + 1 for l in st.in1_ls[:b]) for b in range(NB)]
    ypre = [sum(2 * l + 1 for l in st.in2_ls[:j]) for j in range(len(st.in2_ls))]
    opre = [sum(2 * l + 1 for l in st.out_ls[:s]) for s in range(NS)]
    XD = sum(2 * l + 1 for l in st.in1_ls)
    S = sum(2 * l + 1 for l in st.in2_ls)
    OD = sum(2 * l + 1 for l in st.out_ls)
    n_into = [0] * NS
    for _, _, s in st.instr:
        n_into[s] += 1
    coeff = [((2 * st.out_ls[s] + 1) / n_into[s]) ** 0.5 for _, _, s in st.instr]
    # slots shared by several instructions have equal coeff per slot (same l3, same n_into)
    slot_coeff = [None] * NS
    for p, (_, _, s) in enumerate(st.instr):
        slot_coeff[s] = coeff[p]
    first_path, last_path = {}, {}
    for p, (b, _, _) in enumerate(st.instr):
        first_path.setdefault(b, p)
        last_path[b] = p
    blocks_in_order = [b for b, _, _ in st.instr]
    assert all(blocks_in_order[first_path[b]:last_path[b] + 1] == [b] * (last_path[b] - first_path[b] + 1) for b in first_path), \
        "paths are created input-block major (interaction_block.py:89-109)"
    unused_comps = [i for b in range(NB) if b not in first_path for i in range(xpre[b], xpre[b] + 2 * st.in1_ls[b] + 1)]
    # register-heavy structures (l_max = 3 middle layer): ask for two wavefronts per SIMD so that the compiler does not
    # spend the whole register file on load hoisting at occupancy 1
    big = (OD + 2 * (XD + NP + S)) > 160
    # pair kernel: two grad_out rows, three x rows, the weights in registers.  Measured on cu20k (l_max 3, 269): 298 spilled
    # registers, fused backward 10 -> 70 ms -- the big structures stay with the per-edge kernels or the split form
    pair_ok = (2 * OD + 3 * XD + NP) <= PAIR_BUDGET
    # ring kernel: the owner's grad_out row and the products of it the compiler hoists out of the pair loop, both y rows and
    # both grad_y accumulators, the owner's x row / its gradient / one block's row gradient (l2n_mid: 177 -> 247 registers;
    # l3n_mid_k2: 192 -> 27 spilled, whose scratch loads draw hipcc's own vmcnt waits into the loop --
    # scripts/check_ring_waits.py).  Structures beyond it keep bwd_pair_kernel.
    ring = None
    if pair_ok and OD + n_owner_terms(st, range(NP)) + 4 * S + 3 * XD <= RING_BUDGET:
        ring = ring_layout(st, list(range(NP)), len(unused_comps), last_path)
    # split form: greedy merge of consecutive input blocks while a (conservative) register budget holds -- the l_max = 3
    # parts carry 32 grad_y accumulators and up to 49 intermediates per path on top of what `budget` counts
    part_paths: List[List[int]] = []
    if not pair_ok:
        by_block = {}
        for pth, (b, _, _) in enumerate(st.instr):
            by_block.setdefault(b, []).append(pth)

        def budget(paths):
            od = sum(2 * st.out_ls[st.instr[p_][2]] + 1 for p_ in paths)
            xd = sum(2 * st.in1_ls[b_] + 1 for b_ in {st.instr[p_][0] for p_ in paths})
            return 2 * od + 3 * xd + len(paths)

        for b in sorted(by_block):
            if part_paths and budget(part_paths[-1] + by_block[b]) <= SPLIT_MERGE_BUDGET:
                part_paths[-1] = part_paths[-1] + by_block[b]
            else:
                part_paths.append(list(by_block[b]))
        if not (all(budget(pp) <= PAIR_BUDGET for pp in part_paths) and 1 < len(part_paths) <= 8):
            part_paths = []
    pair_parts = len(part_paths) if part_paths else (1 if pair_ok else 0)
    split_rings = []
    for part_i, paths in enumerate(part_paths):
        sr = ring_layout(st, paths, len(unused_comps) if part_i == 0 else 0, last_path)
        if sr is None:
            # (the host zeroes grad_y and asks for atomic adds for flag 2, which only the split ring kernel implements)
            raise ValueError(f"{st.name}: no LDS-ring plan for pair part {part_i} (paths {paths})")
        split_rings.append(sr)
    ring_flag = 2 if pair_parts > 1 else (1 if ring is not None else 0)
    return Plan(st, NB, NS, NP, XD, S, OD, xpre, ypre, opre, coeff, slot_coeff, sorted(first_path),
                sorted({j for _, j, _ in st.instr}), sorted({s for _, _, s in st.instr}), unused_comps, first_path, last_path,
                big, pair_ok, ring, part_paths, pair_parts, split_rings, ring_flag)


# --------------------------------------------------------------------------------------------------------------
# Shared pieces of the emitters.

def emit_store(ptr, val):
    # streamed per-edge / per-pair result rows (grad_w, grad_x rows) leave through nontemporal stores: they are read long after
    # the caches have turned over (same-box A/B: cfg-3 edge backward 0.24 -> 0.22 ms, cu20k step 22.2 -> 21.8 ms)
    return f"__builtin_nontemporal_store({val}, {ptr})"


def decl_x(p: Plan, indent, sfx=""):
    return [f"{indent}T xb{b}{sfx}[{2 * p.st.in1_ls[b] + 1}];" for b in p.used_blocks]


def decl_y(p: Plan, indent, sfx=""):
    return [f"{indent}T yb{j}{sfx}[{2 * p.st.in2_ls[j] + 1}];" for j in p.used_y]


# Addressing: every row base (x[src], w[e], y[e], g[dst]) is wave-uniform (scalar registers); the per-lane part is a
# loop-invariant 32-bit element offset computed once from the *clamped* channel uc = min(u, mul-1), so loads need
# no predication (lanes with u >= mul read channel mul-1 and never store).
def lane_offsets(p: Plan, indent, want_x=True, want_g=False):
    st = p.st
    out = [f"{indent}const unsigned ucb = (unsigned)(u < mul ? u : mul - 1) * (unsigned)sizeof(T);"]
    if want_x:
        for b in p.used_blocks:
            out.append(f"{indent}const unsigned xo{b} = (unsigned)(mul * {p.xpre[b]}) * (unsigned)sizeof(T) + ucb * {2 * st.in1_ls[b] + 1}u;")
    if want_g:
        for sl in p.used_slots:
            out.append(f"{indent}const unsigned go{sl} = (unsigned)(mul * {p.opre[sl]}) * (unsigned)sizeof(T) + ucb * {2 * st.out_ls[sl] + 1}u;")
    return out


def load_x(p: Plan, indent, row, sfx="", decl=True):
    out = decl_x(p, indent, sfx) if decl else []
    for b in p.used_blocks:
        for i in range(2 * p.st.in1_ls[b] + 1):
            out.append(f"{indent}xb{b}{sfx}[{i}] = spec_at({row}, xo{b})[{i}];")
    return out


def load_y(p: Plan, indent, row, sfx="", decl=True):
    out = decl_y(p, indent, sfx) if decl else []
    for j in p.used_y:
        for i in range(2 * p.st.in2_ls[j] + 1):
            out.append(f"{indent}yb{j}{sfx}[{i}] = {row}[{p.ypre[j] + i}];")
    return out


def load_w(p: Plan, indent, row, scale=False, sfx="", decl=True):
    # plain loads: nontemporal weight loads measured worse (cfg-3 tp_fwd 0.36 -> 0.39 ms, edge backward 0.21 -> 0.25)
    out = [f"{indent}T wv{sfx}[kNP];"] if decl else []
    for pth in range(p.NP):
        c = f"T({p.coeff[pth]!r}) * " if scale else ""
        out.append(f"{indent}wv{sfx}[{pth}] = {c}*spec_at({row} + (unsigned)(mul * {pth}), ucb);")
    return out


def load_g(p: Plan, indent, rowexpr, name):
    """A grad_out row, scaled by the path coefficients and zeroed on inactive lanes, into `name`."""
    out = [f"{indent}{{ const T* __restrict__ gb = {rowexpr};"]
    for s_ in range(p.NS):
        for k in range(2 * p.st.out_ls[s_] + 1):
            if p.slot_coeff[s_] is None:
                out.append(f"{indent}  {name}[{p.opre[s_] + k}] = T(0);")
            else:
                out.append(f"{indent}  {name}[{p.opre[s_] + k}] = spec_at(gb, go{s_})[{k}];")
    for s_ in range(p.NS):
        if p.slot_coeff[s_] is None:
            continue
        for k in range(2 * p.st.out_ls[s_] + 1):
            out.append(f"{indent}  {name}[{p.opre[s_] + k}] = act ? T({p.slot_coeff[s_]!r}) * {name}[{p.opre[s_] + k}] : T(0);")
    out.append(f"{indent}}}")
    return out


def path_terms(p: Plan, out, pth, xs, gname, ys, tag_, ind, dual):
    """One path of one directed edge of the pair kernels: B{tag}{jj} (-> grad_w, grad_y) into `out`; returns the live jj and
    the grad_x terms per input component.  dual: also the D{tag}{jj} of DUAL (B from the cotangent rows x2, D from x)."""
    b_, j, s_ = p.st.instr[pth]
    l1, l2, l3 = p.st.in1_ls[b_], p.st.in2_ls[j], p.st.out_ls[s_]
    d1, d2, d3 = 2 * l1 + 1, 2 * l2 + 1, 2 * l3 + 1
    C = _cg(l1, l2, l3)
    started = [False] * d2
    gx_terms = []
    for i in range(d1):
        a_terms = []
        for jj in range(d2):
            ks = [k for k in range(d3) if C[i, jj, k] != 0.0]
            if not ks:
                continue
            expr = " + ".join(f"T({float(C[i, jj, k])!r}) * {gname}[{p.opre[s_] + k}]" for k in ks)
            out.append(f"{ind}const T t{tag_}{i}_{jj} = {expr};")
            xa = f"(DUAL ? xb{b_}{xs}2[{i}] : xb{b_}{xs}[{i}])" if dual else f"xb{b_}{xs}[{i}]"
            if started[jj]:
                out.append(f"{ind}B{tag_}{jj} += {xa} * t{tag_}{i}_{jj};")
                if dual:
                    out.append(f"{ind}if (DUAL) D{tag_}{jj} += xb{b_}{xs}[{i}] * t{tag_}{i}_{jj};")
            else:
                out.append(f"{ind}T B{tag_}{jj} = {xa} * t{tag_}{i}_{jj};")
                if dual:
                    out.append(f"{ind}T D{tag_}{jj} = DUAL ? xb{b_}{xs}[{i}] * t{tag_}{i}_{jj} : T(0);")
                started[jj] = True
            a_terms.append(f"yb{j}{ys}[{jj}] * t{tag_}{i}_{jj}")
        gx_terms.append((p.xpre[b_] + i, " + ".join(a_terms) if a_terms else None))
    return [jj for jj in range(d2) if started[jj]], gx_terms


def src_base(p: Plan, kind, ident):
    """Byte offset of a ring copy's segment from its row base (weight column / x block / grad_out slot of this chunk)."""
    if kind == "w":
        return f"(unsigned)(mul * {ident} + chunk * 64) * 4u"
    if kind == "x":
        return f"(unsigned)(mul * {p.xpre[ident]} + chunk * {64 * (2 * p.st.in1_ls[ident] + 1)}) * 4u"
    return f"(unsigned)(mul * {p.opre[ident]} + chunk * {64 * (2 * p.st.out_ls[ident] + 1)}) * 4u"


def ring_lane_offsets(p: Plan, r: Ring, ind, ro):
    """Per-lane source offsets of the copies that span several segments (one segment: its uniform offset goes into the
    scalar base, the lanes share l16)."""
    out = []
    for c_ in range(r.chunks):
        for i_, (kind, loff, nl, pieces) in enumerate(r.dma[c_]):
            if pieces is None or len(pieces) == 1:
                continue
            expr = None
            for lo, hi, ident, seg_unit in reversed(pieces):
                e_ = f"{src_base(p, kind, ident)} + (unsigned)({(seg_unit - lo) * COPY_BYTES})"
                expr = e_ if expr is None else f"(lane < {hi} ? {e_} : {expr})"
            out.append(f"{ind}const unsigned {ro}{c_}_{i_} = ({expr}) + l16;")
    return out


def ring_copies(p: Plan, r: Ring, ind, c_, sfx, slotexpr, slot_bytes, ro, lgkm_note, lgkm=True):
    """Copies of chunk c_ of the pair whose indices are in jn{sfx} / pr{sfx} / ei{sfx} / eo{sfx} into LDS slot `slotexpr`.
    Only the weight rows are copied nontemporally: they are read once (lab: 545 -> 533 us; x / g too: slower)."""
    out = [f"{ind}{{ const unsigned sb_ = wbase + (unsigned)({slotexpr}) * {slot_bytes};"]
    if lgkm:
        out.append(f"{ind}  spec_wait_lgkm();{lgkm_note}")
    kinds = {k_ for k_, _, _, _ in r.dma[c_]}
    if "w" in kinds:
        out.append(f"{ind}  const T* __restrict__ wr_ = a.w + (int64_t)pr{sfx} * a.wn;")
    if "x" in kinds:
        out.append(f"{ind}  const T* __restrict__ xr_ = a.x + (int64_t)jn{sfx} * a.din;")
    if "g" in kinds:
        out.append(f"{ind}  const T* __restrict__ gr_ = a.g + (int64_t)jn{sfx} * a.dout;")
    for i_, (kind, loff, nl, pieces) in enumerate(r.dma[c_]):
        if kind == "yI":
            out.append(f"{ind}  spec_glds4<{nl}>(sb_ + {loff}u, a.y + (int64_t)ei{sfx} * kS, l4);")
        elif kind == "yX":
            out.append(f"{ind}  spec_glds4<{nl}>(sb_ + {loff}u, a.y + (int64_t)eo{sfx} * kS, l4);")
        else:
            nt_ = ", true" if kind == "w" else ""
            if len(pieces) == 1:
                lo_, _, ident_, seg_unit_ = pieces[0]
                uoff = f"{src_base(p, kind, ident_)} + (unsigned)({(seg_unit_ - lo_) * COPY_BYTES})"
                out.append(f"{ind}  spec_glds16<{nl}{nt_}>(sb_ + {loff}u, reinterpret_cast<const char*>({kind}r_) + ({uoff}), l16);")
            else:
                out.append(f"{ind}  spec_glds16<{nl}{nt_}>(sb_ + {loff}u, {kind}r_, {ro}{c_}_{i_});")
    out.append(f"{ind}}}")
    return out


def ring_waits(r: Ring, c_, ind):
    """Counted wait before chunk c_ is read: the copies and stores issued since its own copies (tp_spec.h spec_wait_vm)."""
    nfirst = r.copies + sum(r.Sgw[:c_])
    nfirst_gx = f"(ATOM ? {nfirst + sum(r.Sgx_atom[:c_])} : {nfirst + sum(r.Sgx[:c_])})"
    nsteady = r.copies + sum(r.Sgw)
    nsteady_gx = f"(ATOM ? {nsteady + sum(r.Sgx_atom)} : {nsteady + sum(r.Sgx)})"
    return [f"{ind}if (!hasB) spec_wait_vm<0>();",
            f"{ind}else if (first) spec_wait_vm<GX ? {nfirst_gx} : {nfirst}>();",
            f"{ind}else spec_wait_vm<GX ? {nsteady_gx} : {nsteady}>();"]


def ring_operand_reads(p: Plan, r: Ring, c_, ys, ind):
    """The y rows (chunk 0) and the x blocks placed in chunk c_, from its LDS image into registers."""
    lo, out = r.lds_off[c_], []
    if c_ == 0:
        for j in ys:
            for i in range(2 * p.st.in2_ls[j] + 1):
                out.append(f"{ind}yb{j}I[{i}] = *reinterpret_cast<const T*>(cb + {lo[('y', 'I')] + 4 * (p.ypre[j] + i)});")
                out.append(f"{ind}yb{j}X[{i}] = *reinterpret_cast<const T*>(cb + {lo[('y', 'X')] + 4 * (p.ypre[j] + i)});")
    for b_ in r.blocks:
        if r.xplace[b_] == c_:
            d1 = 2 * p.st.in1_ls[b_] + 1
            for i in range(d1):
                out.append(f"{ind}xb{b_}J[{i}] = *reinterpret_cast<const T*>(cb + {lo[('x', b_)]} + l4 * {d1}u + {4 * i});")
    return out


def wave_reduce_lines(n, acc):
    """WPN > 1: the wavefronts of a node add their `n` accumulators through the LDS into wavefront 0's."""
    return ["  if (WPN > 1) {",
            "    extern __shared__ __align__(16) unsigned char nqa_smem[];",
            "    T* red = reinterpret_cast<T*>(nqa_smem);",
            "    if (wsub > 0) {",
            "#pragma unroll",
            f"      for (int k = 0; k < {n}; ++k) red[((wsub - 1) * {n} + k) * 64 + lane] = {acc}[k];",
            "    }",
            "    __syncthreads();",
            "    if (wsub > 0) return;",
            "#pragma unroll",
            f"    for (int k = 0; k < {n}; ++k) {{",
            "#pragma unroll",
            f"      for (int w2 = 0; w2 < WPN - 1; ++w2) {acc}[k] += red[(w2 * {n} + k) * 64 + lane];",
            "    }",
            "  }"]


def store_x_rows(p: Plan, ind, blocks, uvar, val):
    """One node's grad_x row in the irreps layout; val(component) gives the value."""
    out = []
    for b in blocks:
        d = 2 * p.st.in1_ls[b] + 1
        for i in range(d):
            out.append(f"{ind}ob[(int64_t)mul * {p.xpre[b]} + (int64_t){uvar} * {d} + {i}] = {val(p.xpre[b] + i)};")
    return out


# --------------------------------------------------------------------------------------------------------------
# Emitters: one per kernel family, each returns its lines.

def emit_header(p: Plan) -> List[str]:
    st = p.st
    return [f"// GENERATED by gen_spec.py for structure '{st.name}': {st.key()}",
            "// Edge-outer specialised TensorProductScatter kernels (see gen_spec.py docstring).",
            '#include <hip/hip_runtime.h>',
            '#include <cstdint>',
            '#include "../generated/cg_generated.h"',
            '#include "../tp_spec.h"',
            "namespace nqa {",
            "namespace {",
            f"constexpr int kXD = {p.XD}, kS = {p.S}, kOD = {p.OD}, kNP = {p.NP};",
            "typedef float f2 __attribute__((ext_vector_type(2)));  // one v_pk_*_f32 operand: two fp32 values in a register pair"]


def _node_kernel_prologue(L):
    """Item / node / chunk of fwd_kernel and bwd_x_kernel (WPN == 1: four nodes per workgroup, else one)."""
    L += ["  const int lane = threadIdx.x & 63;",
          "  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));",
          "  const int mul = a.mul;",
          "  const int nchunk = (mul + 63) >> 6;",
          "  int64_t item; int wsub;",
          "  const unsigned bid = spec_xcd_remap(blockIdx.x, gridDim.x);",
          "  if (WPN == 1) { item = (int64_t)bid * 4 + wid; wsub = 0; } else { item = bid; wsub = wid; }",
          "  const bool valid = item < (int64_t)a.N * nchunk;",
          "  if (WPN == 1 && !valid) return;",
          "  const int node = spec_uniform(valid ? (int)(item / nchunk) : 0);",
          "  const int chunk = (int)(item - (int64_t)node * nchunk);",
          "  const int u = chunk * 64 + lane;",
          "  const bool act = valid && (u < mul);"]


def _edge_kernel_prologue(L):
    """Item / node / chunk of the kernels that spread WPN wavefronts over a node (four wavefronts per workgroup)."""
    L += ["  const int lane = threadIdx.x & 63;",
          "  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));",
          "  const int mul = a.mul;",
          "  const int nchunk = (mul + 63) >> 6;",
          "  const int64_t witem = (int64_t)spec_xcd_remap(blockIdx.x, gridDim.x) * 4 + wid;",
          "  const int64_t item = witem / WPN;",
          "  const int wsub = (int)(witem - item * WPN);"]


def emit_fwd(p: Plan) -> List[str]:
    st = p.st
    lb = "__launch_bounds__(256, 2)" if p.big else "__launch_bounds__(256)"
    L = []
    A = L.append
    A("// JVP (second-order backward of training: the gradient w.r.t. grad_out): out = F(x2, y, w) + F(x, y2, w) + F(x, y, w2) in")
    A("// one pass over the edges; a term whose cotangent pointer (a.x2 / a.y2 / a.w2) is NULL is skipped (wave-uniform).")
    A("template <typename T, int WPN, bool JVP = false>")
    # (four wavefronts per SIMD would need 128 registers: 19-48 spills in the pipelined loop, measured 2.2x slower)
    A(f"__global__ {lb} void fwd_kernel(const SpecArgs<T> a) {{")
    _node_kernel_prologue(L)
    L.extend(lane_offsets(p, "  "))
    A(f"  T acc[kOD];")
    A("#pragma unroll")
    A("  for (int k = 0; k < kOD; ++k) acc[k] = T(0);")
    A("  const int beg = a.rowptr[node], end = valid ? a.rowptr[node + 1] : beg;")
    # register budget: accumulators + two operand sets; big structures (l_max = 3 middle layer: 99 accumulators, 23
    # paths) would hit the 256-VGPR wall at one wavefront per SIMD, so they run the plain loop at twice the occupancy
    pipelined = not p.big
    if pipelined:
        A("  // Two register sets (A/B): the operands of edge i+1 are requested before edge i is evaluated, the indices of")
        A("  // edge i+2 before that -- every HBM/L2 round trip of an edge hides behind the arithmetic of the previous one.")
        L.extend(["  T wvA[kNP], wvB[kNP];"] + decl_x(p, "  ", "A") + decl_x(p, "  ", "B") + decl_y(p, "  ", "A") + decl_y(p, "  ", "B"))
        L.extend(["  T wv2A[kNP], wv2B[kNP];"] + decl_x(p, "  ", "A2") + decl_x(p, "  ", "B2") + decl_y(p, "  ", "A2") + decl_y(p, "  ", "B2"))
    else:
        L.extend(["  T wvA[kNP];"] + decl_x(p, "  ", "A") + decl_y(p, "  ", "A"))
        L.extend(["  T wv2A[kNP];"] + decl_x(p, "  ", "A2") + decl_y(p, "  ", "A2"))

    def fwd_loads(sfx, e, sv, r):
        out = [f"    {{ const T* __restrict__ xr = a.x + (int64_t){sv} * a.din;",
               f"      const T* __restrict__ wr = a.w + (int64_t){r} * a.wn;",
               f"      const T* __restrict__ yr = a.y + (int64_t){e} * kS;"]
        out += load_w(p, "      ", "wr", sfx=sfx, decl=False)
        out += load_x(p, "      ", "xr", sfx=sfx, decl=False)
        out += load_y(p, "      ", "yr", sfx=sfx, decl=False)
        out.append("      if (JVP) {")
        out.append("        if (a.x2 != nullptr) {")
        out += load_x(p, "          ", f"(a.x2 + (int64_t){sv} * a.din)", sfx=sfx + "2", decl=False)
        out.append("        }")
        out.append("        if (a.y2 != nullptr) {")
        out += load_y(p, "          ", f"(a.y2 + (int64_t){e} * kS)", sfx=sfx + "2", decl=False)
        out.append("        }")
        out.append("        if (a.w2 != nullptr) {")
        out += load_w(p, "          ", f"(a.w2 + (int64_t){r} * a.wn)", sfx="2" + sfx, decl=False)
        out.append("        }")
        out.append("      }")
        out.append("    }")
        return out

    def fwd_compute(sfx):
        out = []
        for pth, (b, j, sl) in enumerate(st.instr):
            l1, l2, l3 = st.in1_ls[b], st.in2_ls[j], st.out_ls[sl]
            d3 = 2 * l3 + 1
            out.append("    if (!JVP) {")
            out.append(f"      T t[{d3}]; CGT<{l1},{l2},{l3}>::template ab_c<T>(xb{b}{sfx}, yb{j}{sfx}, t);")
            for k in range(d3):
                out.append(f"      acc[{p.opre[sl] + k}] += wv{sfx}[{pth}] * t[{k}];")
            out.append("    } else {")
            for cond, xa, ya, wa in ((f"a.w2 != nullptr", f"xb{b}{sfx}", f"yb{j}{sfx}", f"wv2{sfx}[{pth}]"),
                                     (f"a.x2 != nullptr", f"xb{b}{sfx}2", f"yb{j}{sfx}", f"wv{sfx}[{pth}]"),
                                     (f"a.y2 != nullptr", f"xb{b}{sfx}", f"yb{j}{sfx}2", f"wv{sfx}[{pth}]")):
                out.append(f"      if ({cond}) {{ T t[{d3}]; CGT<{l1},{l2},{l3}>::template ab_c<T>({xa}, {ya}, t);")
                for k in range(d3):
                    out.append(f"        acc[{p.opre[sl] + k}] += {wa} * t[{k}];")
                out.append("      }")
            out.append("    }")
        return out

    if pipelined:
        A("  int idx = beg + wsub;")
        A("  int nidx = idx + WPN;")
        A("  int e0 = 0, s0 = 0, e1 = 0, s1 = 0, r0 = 0, r1 = 0;  // r: row of the edge's weights (tp_spec.h spec_wrow)")
        A("  if (idx < end) { e0 = spec_uniform(a.eid[idx]); s0 = spec_uniform(a.nbr[idx]); r0 = spec_wrow(a, idx); }")
        A("  if (idx < end) {")
        L.extend(fwd_loads("A", "e0", "s0", "r0"))
        A("  }")
        A("  if (nidx < end) { e1 = spec_uniform(a.eid[nidx]); s1 = spec_uniform(a.nbr[nidx]); r1 = spec_wrow(a, nidx); }")
        A("  while (idx < end) {")
        A("    if (nidx < end) {")
        L.extend(fwd_loads("B", "e1", "s1", "r1"))
        A("    }")
        A("    int nn = nidx + WPN;")
        A("    if (nn < end) { e0 = spec_uniform(a.eid[nn]); s0 = spec_uniform(a.nbr[nn]); r0 = spec_wrow(a, nn); }")
        L.extend(fwd_compute("A"))
        A("    idx = nidx; nidx = nn;")
        A("    if (idx >= end) break;")
        A("    if (nidx < end) {")
        L.extend(fwd_loads("A", "e0", "s0", "r0"))
        A("    }")
        A("    nn = nidx + WPN;")
        A("    if (nn < end) { e1 = spec_uniform(a.eid[nn]); s1 = spec_uniform(a.nbr[nn]); r1 = spec_wrow(a, nn); }")
        L.extend(fwd_compute("B"))
        A("    idx = nidx; nidx = nn;")
        A("  }")
    else:
        A("  int idx = beg + wsub;")
        A("  int e0 = 0, s0 = 0, r0 = 0;")
        A("  if (idx < end) { e0 = spec_uniform(a.eid[idx]); s0 = spec_uniform(a.nbr[idx]); r0 = spec_wrow(a, idx); }")
        A("  while (idx < end) {")
        A("    const int nidx = idx + WPN;")
        A("    int e_n = 0, s_n = 0, r_n = 0;")
        A("    if (nidx < end) { e_n = spec_uniform(a.eid[nidx]); s_n = spec_uniform(a.nbr[nidx]); r_n = spec_wrow(a, nidx); }")
        L.extend(fwd_loads("A", "e0", "s0", "r0"))
        L.extend(fwd_compute("A"))
        A("    idx = nidx; e0 = e_n; s0 = s_n; r0 = r_n;")
        A("  }")
    L.extend(wave_reduce_lines("kOD", "acc"))
    A("  if (act) {")
    A("    T* __restrict__ ob = a.out + (int64_t)node * a.dout;")
    for s in range(p.NS):
        d3 = 2 * st.out_ls[s] + 1
        for k in range(d3):
            val = "T(0)" if p.slot_coeff[s] is None else f"T({p.slot_coeff[s]!r}) * acc[{p.opre[s] + k}]"
            A(f"    ob[(int64_t)mul * {p.opre[s]} + (int64_t)u * {d3} + {k}] = {val};")
    A("  }")
    A("}")
    return L


def emit_bwd_edge(p: Plan) -> List[str]:
    # One contraction serves both edge gradients:  B^p_j = sum_ik C^p_ijk x_i g_k  gives  gw_p = sum_j y_j B^p_j  and
    # gy_j += w_p B^p_j.  FUSED additionally forms A^p_i = sum_jk C^p_ijk y_j g_k and emits the edge's contribution
    # w_p A^p_i to grad_x[src] (grad_out[dst] is already in registers), summed per source node afterwards.
    # FULL: mul is a multiple of 64, every lane owns a channel -- `act` is a compile-time true, so the per-path stores
    # inside the edge loop are plain stores instead of one exec-mask branch region each (16 of them split the loop body
    # of the l_max = 2 middle layer into as many scheduling regions)
    st = p.st
    L = []
    A = L.append
    A("template <typename T, int WPN, bool FUSED, bool GW, bool GY, bool FULL>")
    # two operand sets at three wavefronts per SIMD (same-box cfg-3: fused backward 0.80 ms vs 0.86 for a plain loop at four
    # wavefronts and 0.91 for a plain loop at three).  Big structures (l_max = 3 middle layer: 99 accumulators, 23 paths)
    # run the plain loop at one wavefront per SIMD: forcing two costs 28 spilled registers and 20 % of the kernel; two
    # operand sets out of a lone wavefront's 512 registers gained nothing on cu20k (9.98 vs 9.36 ms)
    # (the emitted text is pinned by generated_spec.manifest.json: the redundant `FUSED ? 3 : 3`, the never-read `rr` and
    # `probe_sink` stay until a change that re-pins the manifest)
    pipelined = not p.big
    be_lb = "__launch_bounds__(256)" if p.big else "__launch_bounds__(256, FUSED ? 3 : 3)"
    A(f"__global__ {be_lb} void bwd_edge_kernel(const SpecArgs<T> a) {{")
    _edge_kernel_prologue(L)
    A("  if (item >= (int64_t)a.N * nchunk) return;")
    A("  const int node = spec_uniform((int)(item / nchunk));")
    A("  const int chunk = (int)(item - (int64_t)node * nchunk);")
    A("  const int u = chunk * 64 + lane;")
    A("  const bool act = FULL || (u < mul);")
    A("  const int beg = a.rowptr[node], end = a.rowptr[node + 1];")
    A("  if (beg + wsub >= end) return;")
    L.extend(lane_offsets(p, "  ", want_x=True, want_g=True))
    A("  T gv[kOD];")
    A("  {")
    A("    // unpredicated loads from the clamped channel (all requests in flight at once, contiguous components merge into")
    A("    // wide loads), masked afterwards: `act ? load : 0` per element compiles into one branch + load + wait per value,")
    A("    // i.e. kOD serial memory round trips before the first edge")
    A("    const T* __restrict__ gb = a.g + (int64_t)node * a.dout;")
    for s_ in range(p.NS):
        for k in range(2 * st.out_ls[s_] + 1):
            A(f"    gv[{p.opre[s_] + k}] = T(0);" if p.slot_coeff[s_] is None else f"    gv[{p.opre[s_] + k}] = spec_at(gb, go{s_})[{k}];")
    for s_ in range(p.NS):
        if p.slot_coeff[s_] is None:
            continue
        for k in range(2 * st.out_ls[s_] + 1):
            A(f"    gv[{p.opre[s_] + k}] = act ? T({p.slot_coeff[s_]!r}) * gv[{p.opre[s_] + k}] : T(0);")
    A("  }")

    def be_loads(sfx, e, sv, rg):
        out = [f"    {{ const T* __restrict__ xr = a.x + (int64_t){sv} * a.din;",
               f"      const T* __restrict__ yr = a.y + (int64_t){e} * kS;",
               f"      const T* __restrict__ wr = a.w + (int64_t)spec_wrow_of(a, {rg}) * a.wn;"]
        out += load_x(p, "      ", "xr", sfx=sfx, decl=False)
        out.append("      if (GY || FUSED) {")
        out += load_w(p, "        ", "wr", sfx=sfx, decl=False)
        out.append("      }")
        out.append("      if (GW || FUSED) {")
        out += load_y(p, "        ", "yr", sfx=sfx, decl=False)
        out.append("      }")
        out.append("    }")
        return out

    def be_compute(sfx, e, rg):
        # every path's weight gradient is stored as soon as it is formed, and an input block's grad_x components as soon
        # as its last path is done: keeps up to kNP + kXD values out of the live set (the fused form has to fit 168
        # registers for three wavefronts per SIMD; 28 spilled registers doubled its time)
        out = ["    {", "    T rr[kNP];", "    T q[kS];", "#pragma unroll", "    for (int j = 0; j < kS; ++j) q[j] = T(0);"]
        out.append(f"    T* __restrict__ gwr_e = (GW || FUSED) ? a.gw + (int64_t){rg} * a.wn : nullptr;")

        def emit_gw(pth, expr, ind):
            return [f"{ind}{{ const T r_ = {expr}; if (act) {emit_store(f'spec_at(gwr_e + (unsigned)(mul * {pth}), ucb)', 'r_')}; }}"]

        # ---- fused form (all three gradients): one intermediate serves both contractions.  Per path and input component i,
        #   T_ij = sum_k C_ijk g_k   (nnz(C) fused multiply-adds with literal coefficients)
        #   B_j += x_i T_ij          (-> grad_w = sum_j y_j B_j,  grad_y_j += w B_j)
        #   A_i  = sum_j y_j T_ij    (-> grad_x_i += w A_i)
        # i.e. nnz + 2 |{(i,j)}| operations per path instead of 2 nnz + |{(i,k)}| + |{(j,k)}| for two separate
        # contractions of C with (x, g) and (y, g): 346 instead of 429 per edge for the l_max = 2 middle layer, 1272
        # instead of 1625 for l_max = 3 -- the kernel is bound by its vector-ALU work.
        out.append("    if (FUSED) {")
        out.append(f"      T* __restrict__ gxr = a.gxe + (int64_t){e} * a.din;")
        out.append("      T gxa[kXD];")
        for pth, (b_, j, s_) in enumerate(st.instr):
            l1, l2, l3 = st.in1_ls[b_], st.in2_ls[j], st.out_ls[s_]
            d1, d2, d3 = 2 * l1 + 1, 2 * l2 + 1, 2 * l3 + 1
            C = _cg(l1, l2, l3)
            if p.first_path[b_] == pth:
                for i in range(d1):
                    out.append(f"      gxa[{p.xpre[b_] + i}] = T(0);")
            out.append(f"      {{  // path {pth}: {l1} x {l2} -> {l3}")
            bj_started = [False] * d2
            for i in range(d1):
                a_terms = []
                for jj in range(d2):
                    ks = [k for k in range(d3) if C[i, jj, k] != 0.0]
                    if not ks:
                        continue
                    expr = " + ".join(f"T({float(C[i, jj, k])!r}) * gv[{p.opre[s_] + k}]" for k in ks)
                    out.append(f"        const T t{i}_{jj} = {expr};")
                    if bj_started[jj]:
                        out.append(f"        B{jj} += xb{b_}{sfx}[{i}] * t{i}_{jj};")
                    else:
                        out.append(f"        T B{jj} = xb{b_}{sfx}[{i}] * t{i}_{jj};")
                        bj_started[jj] = True
                    a_terms.append(f"yb{j}{sfx}[{jj}] * t{i}_{jj}")
                if a_terms:
                    out.append(f"        gxa[{p.xpre[b_] + i}] += wv{sfx}[{pth}] * ({' + '.join(a_terms)});")
            live = [jj for jj in range(d2) if bj_started[jj]]
            gw_expr = " + ".join(f"yb{j}{sfx}[{jj}] * B{jj}" for jj in live) if live else "T(0)"
            out.extend(emit_gw(pth, gw_expr, "        "))
            for jj in live:
                out.append(f"        q[{p.ypre[j] + jj}] += wv{sfx}[{pth}] * B{jj};")
            out.append("      }")
            if p.last_path[b_] == pth:
                out.append("      if (act) {")
                for i in range(d1):
                    out.append(f"        {emit_store(f'spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb)', f'gxa[{p.xpre[b_] + i}]')};")
                out.append("      }")
        if p.unused_comps:
            out.append("      if (act) {")
            for i in p.unused_comps:
                out.append(f"        *spec_at(gxr + (unsigned)(mul * {i}), ucb) = T(0);")
            out.append("      }")
        out.append("    } else {")
        # ---- edge operands only: B^p_j = sum_ik C^p_ijk x_i g_k through the shared pair products of cg_generated.h
        for pth, (b_, j, s_) in enumerate(st.instr):
            l1, l2, l3 = st.in1_ls[b_], st.in2_ls[j], st.out_ls[s_]
            d2 = 2 * l2 + 1
            out.append(f"    {{ T t[{d2}]; CGT<{l1},{l2},{l3}>::template ac_b<T>(xb{b_}{sfx}, gv + {p.opre[s_]}, t);")
            terms = " + ".join(f"t[{i}] * yb{j}{sfx}[{i}]" for i in range(d2))
            out.append("      if (GW) {")
            out.extend(emit_gw(pth, terms, "        "))
            out.append("      }")
            out.append("      if (GY) {")
            for i in range(d2):
                out.append(f"        q[{p.ypre[j] + i}] += wv{sfx}[{pth}] * t[{i}];")
            out.append("      }")
            out.append("    }")
        out.append("    }")
        out.append("    if (GY || FUSED) {")
        out.append(f"      T* __restrict__ gyr = a.gy + (int64_t){e} * a.gy_stride + chunk * kS;")
        out.append("      spec_mask_dup<T, kS>(q, u < mul);")
        out.append("      spec_wave_reduce_store<T, kS>(q, gyr, lane);")
        out.append("    }")
        out.append("    }")
        return out

    A("  T probe_sink = T(0);")
    A("  int idx = beg + wsub;")
    if pipelined:
        A("  // Two operand sets (A/B) as in the forward kernel: the rows of edge i+1 are requested before edge i is")
        A("  // evaluated and its gradients stored, so every wavefront keeps two edges' worth of loads in flight.")
        L.extend(["  T wvA[kNP], wvB[kNP];"] + decl_x(p, "  ", "A") + decl_x(p, "  ", "B") + decl_y(p, "  ", "A") + decl_y(p, "  ", "B"))
        A("  int e0 = spec_uniform(a.eid[idx]), s0 = spec_uniform(a.nbr[idx]), r0 = spec_gwrow(a, idx);")
        A("  int e1 = 0, s1 = 0, r1 = 0;")
        L.extend(be_loads("A", "e0", "s0", "r0"))
        A("  while (idx < end) {")
        A("    int nidx = idx + WPN;")
        A("    if (nidx < end) {")
        A("      e1 = spec_uniform(a.eid[nidx]); s1 = spec_uniform(a.nbr[nidx]); r1 = spec_gwrow(a, nidx);")
        L.extend(be_loads("B", "e1", "s1", "r1"))
        A("    }")
        L.extend(be_compute("A", "e0", "r0"))
        A("    idx = nidx;")
        A("    if (idx >= end) break;")
        A("    nidx = idx + WPN;")
        A("    if (nidx < end) {")
        A("      e0 = spec_uniform(a.eid[nidx]); s0 = spec_uniform(a.nbr[nidx]); r0 = spec_gwrow(a, nidx);")
        L.extend(be_loads("A", "e0", "s0", "r0"))
        A("    }")
        L.extend(be_compute("B", "e1", "r1"))
        A("    idx = nidx;")
        A("  }")
    else:
        L.extend(["  T wvA[kNP];"] + decl_x(p, "  ", "A") + decl_y(p, "  ", "A"))
        A("  int e = spec_uniform(a.eid[idx]), s = spec_uniform(a.nbr[idx]);")
        A("  int rg = spec_gwrow(a, idx);  // row of grad_w written by this edge; its weights are row spec_wrow_of(a, rg)")
        A("  while (idx < end) {")
        A("    const int nidx = idx + WPN;")
        A("    int e_n = 0, s_n = 0, rg_n = 0;")
        A("    if (nidx < end) { e_n = spec_uniform(a.eid[nidx]); s_n = spec_uniform(a.nbr[nidx]); rg_n = spec_gwrow(a, nidx); }")
        L.extend(be_loads("A", "e", "s", "rg"))
        L.extend(be_compute("A", "e", "rg"))
        A("    idx = nidx; e = e_n; s = s_n; rg = rg_n;")
        A("  }")
    A("}")
    return L


def emit_bwd_x(p: Plan) -> List[str]:
    st = p.st
    lb = "__launch_bounds__(256, 2)" if p.big else "__launch_bounds__(256)"
    L = []
    A = L.append
    A("// DUAL (second-order backward of training): out = Bx(y2, w, g) + Bx(y, w2, g) in one pass (a.y2 / a.w2 = the cotangents)")
    A("template <typename T, int WPN, bool DUAL = false>")
    A(f"__global__ {lb} void bwd_x_kernel(const SpecArgs<T> a) {{")
    _node_kernel_prologue(L)
    L.extend(lane_offsets(p, "  ", want_x=False, want_g=True))
    A("  T acc[kXD];")
    A("#pragma unroll")
    A("  for (int i = 0; i < kXD; ++i) acc[i] = T(0);")
    A("  const int beg = a.rowptr[node], end = valid ? a.rowptr[node + 1] : beg;")
    A("  int idx = beg + wsub;")
    A("  int e = 0, d = 0, r = 0;")
    A("  if (idx < end) { e = spec_uniform(a.eid[idx]); d = spec_uniform(a.nbr[idx]); r = spec_wrow(a, idx); }")
    A("  while (idx < end) {")
    A("    const int nidx = idx + WPN;")
    A("    int e_n = 0, d_n = 0, r_n = 0;")
    A("    if (nidx < end) { e_n = spec_uniform(a.eid[nidx]); d_n = spec_uniform(a.nbr[nidx]); r_n = spec_wrow(a, nidx); }")
    A("    const T* __restrict__ gr = a.g + (int64_t)d * a.dout;")
    A("    const T* __restrict__ wr = a.w + (int64_t)r * a.wn;")
    A("    const T* __restrict__ yr = a.y + (int64_t)e * kS;")
    L.extend(load_w(p, "    ", "wr", scale=True))
    A("    T wv2[kNP];")
    L.extend(decl_y(p, "    ", "2"))
    A("    if (DUAL) {")
    L.extend(load_w(p, "      ", "(a.w2 + (int64_t)r * a.wn)", scale=True, sfx="2", decl=False))
    L.extend(load_y(p, "      ", "(a.y2 + (int64_t)e * kS)", sfx="2", decl=False))
    A("    }")
    for s in p.used_slots:
        d3 = 2 * st.out_ls[s] + 1
        A(f"    T gs{s}[{d3}];")
        for k in range(d3):
            A(f"    gs{s}[{k}] = spec_at(gr, go{s})[{k}];")
    L.extend(load_y(p, "    ", "yr"))
    for pth, (b, j, s) in enumerate(st.instr):
        l1, l2, l3 = st.in1_ls[b], st.in2_ls[j], st.out_ls[s]
        d1 = 2 * l1 + 1
        A("    if (!DUAL) {")
        A(f"      T t[{d1}]; CGT<{l1},{l2},{l3}>::template bc_a<T>(yb{j}, gs{s}, t);")
        for i in range(d1):
            A(f"      acc[{p.xpre[b] + i}] += wv[{pth}] * t[{i}];")
        A("    } else {")
        A(f"      T t[{d1}], t2[{d1}]; CGT<{l1},{l2},{l3}>::template bc_a<T>(yb{j}2, gs{s}, t); CGT<{l1},{l2},{l3}>::template bc_a<T>(yb{j}, gs{s}, t2);")
        for i in range(d1):
            A(f"      acc[{p.xpre[b] + i}] += wv[{pth}] * t[{i}] + wv2[{pth}] * t2[{i}];")
        A("    }")
    A("    idx = nidx; e = e_n; d = d_n; r = r_n;")
    A("  }")
    L.extend(wave_reduce_lines("kXD", "acc"))
    A("  if (act) {")
    A("    T* __restrict__ ob = a.out + (int64_t)node * a.din;")
    L.extend(store_x_rows(p, "    ", range(p.NB), "u", lambda c: f"acc[{c}]"))
    A("  }")
    A("}")
    return L


# ------------------------------------------------------------------ backward, pair-centric (paired radial weights)
# A reverse-edge pair p = {j -> o, o -> j} shares one weight row.  Walking the edges by destination, the two directed
# edges of a pair are evaluated by different wavefronts at different times: the weight row is read twice, the two
# halves of its gradient are written to separate rows (summed later by the radial backward), and every directed edge
# writes a per-edge row of grad_x contributions for its source.  Here every pair has an OWNER node o (half of each
# node's pairs, see EdgePairing.owner_csr); the wavefront of o holds x[o], grad_out[o] and the grad_x[o] accumulators
# in registers and, per owned pair, gathers x[j] and grad_out[j] and evaluates BOTH directed edges:
#   in  = j -> o  (x = x[j], g = grad_out[o]):  grad_w half, grad_y[in],  grad_x[j] contribution -> row of the pair
#   out = o -> j  (x = x[o], g = grad_out[j]):  grad_w half, grad_y[out], grad_x[o] contribution -> registers
# so the weight row is read once, grad_w leaves already summed ([P, W] instead of [2P, W]) and only one grad_x row per
# pair is written: per pair 2 W + dim_in1 floats of HBM traffic instead of 2 (2 W + dim_in1), in exchange for a second
# gathered node row (grad_out[j]) that comes out of the cache hierarchy.  Same arithmetic per directed edge as the
# fused kernel above (shared intermediate T_ij).
def emit_pair(p: Plan) -> List[str]:
    st = p.st
    pair_lb = "__launch_bounds__(256)" if p.big else "__launch_bounds__(256, 2)"
    L = []
    A = L.append
    A("// GX = false: grad_w (summed over the pair) and grad_y only -- layers whose grad_x is not needed or comes from bwd_x")
    A("// DUAL (with GX = false; second-order backward of training): two operand sets in one pass,")
    A("//   grad_w = Bw(x2, y, g) + Bw(x, y2, g),  grad_y = By(x2, w, g)   (x2 = a.x2, y2 = a.y2: the cotangents of grad_x /")
    A("//   grad_y of the first-order backward) -- the intermediate T_ij = sum_k C_ijk g_k serves both products")
    A("template <typename T, int WPN, bool FULL, bool GX, bool DUAL = false>")
    A(f"__global__ {pair_lb} void bwd_pair_kernel(const SpecArgs<T> a) {{")
    _edge_kernel_prologue(L)
    A("  if (item >= (int64_t)a.N * nchunk) return;  // (WPN == 4: the whole workgroup)")
    A("  const int node = spec_uniform((int)(item / nchunk));")
    A("  const int chunk = (int)(item - (int64_t)node * nchunk);")
    A("  const int u = chunk * 64 + lane;")
    A("  const bool act = FULL || (u < mul);")
    A("  const int beg = a.rowptr[node], end = a.rowptr[node + 1];")
    L.extend(lane_offsets(p, "  ", want_x=True, want_g=True))
    A("  T gvO[kOD], gxO[kXD];")
    L.extend(load_g(p, "  ", "a.g + (int64_t)node * a.dout", "gvO"))
    L.extend(load_x(p, "  ", "(a.x + (int64_t)node * a.din)", sfx="O"))
    L.extend(decl_x(p, "  ", "O2"))
    A("  if (DUAL) {")
    L.extend(load_x(p, "    ", "(a.x2 + (int64_t)node * a.din)", sfx="O2", decl=False))
    A("  }")
    A("#pragma unroll")
    A("  for (int i = 0; i < kXD; ++i) gxO[i] = T(0);")
    A("  int idx = beg + wsub;")
    A("  T gvJ[kOD];")
    L += (["  T wvA[kNP], wv2A[kNP];", "  int jnA = 0, prA = 0, eiA = 0, eoA = 0;"]
          + decl_x(p, "  ", "JA") + decl_y(p, "  ", "IA") + decl_y(p, "  ", "XA")
          + decl_x(p, "  ", "JA2") + decl_y(p, "  ", "IA2") + decl_y(p, "  ", "XA2"))
    # the next pair's weight row (the one stream that comes from HBM) is touched while this pair is evaluated -- plain loads
    # into a sink value, so that the row is in the L2 when the real loads ask for it (same-box cfg-3: 2.930 -> 2.912 ms)
    A("  T pf_sink = T(0);")
    A("  for (; idx < end; idx += WPN) {")
    # operands of the pair in owner slot idx (the indices are wave-uniform)
    A("    {")
    A("      jnA = spec_uniform(a.nbr[idx]); prA = spec_uniform(a.wid[idx]);")
    A("      eiA = spec_uniform(a.eid[idx]); eoA = spec_uniform(a.eid2[idx]);")
    A("      const T* __restrict__ xr = a.x + (int64_t)jnA * a.din;")
    A("      const T* __restrict__ wr = a.w + (int64_t)prA * a.wn;")
    A("      const T* __restrict__ yi = a.y + (int64_t)eiA * kS;")
    A("      const T* __restrict__ yo = a.y + (int64_t)eoA * kS;")
    L.extend(load_w(p, "      ", "wr", sfx="A", decl=False))
    L.extend(load_x(p, "      ", "xr", sfx="JA", decl=False))
    L.extend(load_g(p, "      ", "a.g + (int64_t)jnA * a.dout", "gvJ"))
    L.extend(load_y(p, "      ", "yi", sfx="IA", decl=False))
    L.extend(load_y(p, "      ", "yo", sfx="XA", decl=False))
    A("      if (DUAL && a.w2 != nullptr) {")
    L.extend(load_w(p, "        ", "(a.w2 + (int64_t)prA * a.wn)", sfx="2A", decl=False))
    A("      }")
    A("      if (DUAL) {")
    L.extend(load_x(p, "        ", "(a.x2 + (int64_t)jnA * a.din)", sfx="JA2", decl=False))
    L.extend(load_y(p, "        ", "(a.y2 + (int64_t)eiA * kS)", sfx="IA2", decl=False))
    L.extend(load_y(p, "        ", "(a.y2 + (int64_t)eoA * kS)", sfx="XA2", decl=False))
    A("      }")
    A("    }")
    A("    T pf[kNP];")
    A("    {")
    A("      const int nidx_ = idx + WPN < end ? idx + WPN : idx;")
    A("      const int prn_ = spec_uniform(a.wid[nidx_]);")
    A("      const T* __restrict__ wn_ = a.w + (int64_t)prn_ * a.wn;")
    for pth in range(p.NP):
        A(f"      pf[{pth}] = *spec_at(wn_ + (unsigned)(mul * {pth}), ucb);")
    A("    }")
    # both directed edges of the pair
    A("    {")
    A("    T qI[kS], qX[kS], gxa[kXD];")
    A("#pragma unroll")
    A("    for (int j = 0; j < kS; ++j) { qI[j] = T(0); qX[j] = T(0); }")
    A("    T* __restrict__ gwr_e = a.gw + (int64_t)prA * a.wn;")
    A("    T* __restrict__ gxr = a.gxe + (int64_t)(idx) * a.din;")
    for pth, (b_, j, s_) in enumerate(st.instr):
        d1 = 2 * st.in1_ls[b_] + 1
        if p.first_path[b_] == pth:
            for i in range(d1):
                A(f"      gxa[{p.xpre[b_] + i}] = T(0);")
        A(f"      {{  // path {pth}")
        live_i, gx_i = path_terms(p, L, pth, "JA", "gvO", "IA", "i", "        ", dual=True)
        for comp, expr in gx_i:
            if expr:
                A(f"        if (GX) gxa[{comp}] += wvA[{pth}] * ({expr});")
        live_x, gx_x = path_terms(p, L, pth, "O", "gvJ", "XA", "x", "        ", dual=True)
        for comp, expr in gx_x:
            if expr:
                A(f"        if (GX) gxO[{comp}] += wvA[{pth}] * ({expr});")
        terms = [f"yb{j}IA[{jj}] * Bi{jj}" for jj in live_i] + [f"yb{j}XA[{jj}] * Bx{jj}" for jj in live_x]
        gw_expr = " + ".join(terms) if terms else "T(0)"
        dterms = [f"yb{j}IA2[{jj}] * Di{jj}" for jj in live_i] + [f"yb{j}XA2[{jj}] * Dx{jj}" for jj in live_x]
        dual_expr = " + ".join(dterms) if dterms else "T(0)"
        A(f"        {{ T r_ = {gw_expr}; if (DUAL) r_ += {dual_expr}; if (act) {emit_store(f'spec_at(gwr_e + (unsigned)(mul * {pth}), ucb)', 'r_')}; }}")
        for jj in live_i:
            A(f"        qI[{p.ypre[j] + jj}] += wvA[{pth}] * Bi{jj};")
        for jj in live_x:
            A(f"        qX[{p.ypre[j] + jj}] += wvA[{pth}] * Bx{jj};")
        # DUAL with a weight cotangent (a.w2): grad_y += By(x, w2, g) rides on the D intermediates
        A("        if (DUAL && a.w2 != nullptr) {")
        for jj in live_i:
            A(f"          qI[{p.ypre[j] + jj}] += wv2A[{pth}] * Di{jj};")
        for jj in live_x:
            A(f"          qX[{p.ypre[j] + jj}] += wv2A[{pth}] * Dx{jj};")
        A("        }")
        A("      }")
        if p.last_path[b_] == pth:
            A("      if (GX && act) {")
            for i in range(d1):
                A(f"        {emit_store(f'spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb)', f'gxa[{p.xpre[b_] + i}]')};")
            A("      }")
    if p.unused_comps:
        A("      if (GX && act) {")
        for i in p.unused_comps:
            A(f"        *spec_at(gxr + (unsigned)(mul * {i}), ucb) = T(0);")
        A("      }")
    A("      spec_mask_dup<T, kS>(qI, u < mul);")
    A("      spec_mask_dup<T, kS>(qX, u < mul);")
    A("      spec_wave_reduce_store<T, kS>(qI, a.gy + (int64_t)eiA * a.gy_stride + chunk * kS, lane);")
    A("      spec_wave_reduce_store<T, kS>(qX, a.gy + (int64_t)eoA * a.gy_stride + chunk * kS, lane);")
    A("    }")
    A("#pragma unroll")
    A("    for (int p_ = 0; p_ < kNP; ++p_) pf_sink += pf[p_];")
    A("  }")
    A("  if (pf_sink == T(12345.678)) a.gy[0] = pf_sink;")
    A("  // grad_x[owner]: the owner-side contributions of all its pairs (the other side arrives through the rows)")
    A("  if (!GX) return;")
    L.extend(wave_reduce_lines("kXD", "gxO"))
    A("  if (act) {")
    A("    const int uc = u < mul ? u : mul - 1;")
    A("    T* __restrict__ ob = a.out + (int64_t)node * a.din;")
    L.extend(store_x_rows(p, "    ", range(p.NB), "uc", lambda c: f"gxO[{c}]"))
    A("  }")
    A("}")
    return L


# ------------------------------------------------------------------ pair-centric backward, LDS ring
# What held bwd_pair_kernel at half of the HBM roof (profiles/r6_pair_*.txt, r6_lab_call4.txt ... call7.txt; index: profiles/README_r6.md): one pair in flight per
# wavefront at two wavefronts per SIMD.  The same loop WITHOUT its arithmetic takes 85 % of the kernel's time, with every
# stream pointed at cache-hot rows still 42 % -- it is the serial chain indices -> row loads -> arithmetic -> stores of
# each pair, 8 of them per CU, not bandwidth and not the vector ALU; a second operand set in registers spills (254 used).
# (A packed-fp32 form that evaluated both directed edges of a pair as v_pk_* pairs measured 561 vs 575 us: a v_pk_fma_f32
# takes twice the passes of a v_fma_f32, profiles/r6_pk_rate_and_packed_pair_call2.txt.)
# Here the rows of the NEXT pair travel global -> LDS by LDS-DMA (no registers) while the current pair is evaluated out
# of the LDS: every wavefront owns a ring of kRingSlots slots in the CU's 160 KB (20 KB per wavefront at two per SIMD);
# a pair's rows (w, x[other], grad_out[other], the two y rows: 14 KB for the l_max = 2 middle layer) are cut into
# kRingChunks = kRingSlots - 1 chunks in the order the paths consume them, so that one whole pair is always in flight
# behind the one being evaluated.  After chunk q is evaluated its slot is refilled with chunk q + kRingSlots.  The copies
# are 16 bytes per lane (dword-per-lane reads reach 4.0 TB/s on this part, 16-byte ones 6.7: scripts/micro/store_bw.hip);
# lane l of an instruction lands at slot + 16 l, the LDS image of a segment is the 64 channels' values in row order, and
# the evaluation reads its operands with ds_read (4 u + component) right where it uses them -- no operand arrays in
# registers.  Ordering: the issuing wavefront's counted s_waitcnt vmcnt(N), N = the copies and stores issued since
# (static: one pair's worth of each in the steady state, tp_spec.h spec_wait_vm); the first pair of a wavefront counts
# its own shorter history, the last one waits for everything.  scripts/check_ring_waits.py re-counts N in the ISA.
def emit_pair_ring(p: Plan) -> List[str]:
    st, r = p.st, p.ring
    RC, RN, RSLOT = r.chunks, r.slots, r.slot_bytes
    L = []
    A = L.append

    def copies(ind, c_, sfx, slotexpr, lgkm=True):
        return ring_copies(p, r, ind, c_, sfx, slotexpr, "(unsigned)kRingSlotBytes", "ro", "  // the slot's last reads have returned", lgkm)

    A(f"constexpr int kRingChunks = {RC}, kRingSlots = {RN}, kRingSlotBytes = {RSLOT}, kRingWaveBytes = {RN * RSLOT};")
    A("// ring chunks: " + "; ".join(
        f"{c_}: paths {r.cpaths[c_][0]}-{r.cpaths[c_][-1]}" + "".join(f" +x{b_}" for b_ in r.blocks if r.xplace[b_] == c_)
        + f", {len(r.dma[c_])} copies, {r.Sgw[c_]}+{r.Sgx[c_]} stores" for c_ in range(RC)))
    A("// ATOM: the other node's grad_x contribution goes into a zeroed [N, dim_in1] accumulator (a.gxe, component rows of 64")
    A("// channels as the per-pair rows) by floating-point atomics instead of one row per pair: no [P, dim_in1] round trip")
    A("// through HBM and no row sum -- gx_acc_finish_kernel folds the accumulator into a.out.  (Sums in arrival order: the")
    A("// low bits of grad_x differ from run to run; ATOM = false keeps the fixed-order rows.)")
    A("template <int WPN, bool GX, bool ATOM>")
    A("__global__ __launch_bounds__(256, 2) void bwd_pair_ring_kernel(const SpecArgs<float> a) {")
    A("  typedef float T;")
    A("  extern __shared__ __align__(16) unsigned char nqa_smem[];")
    A("  const int lane = threadIdx.x & 63;")
    A("  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));")
    A("  const int mul = a.mul;  // a multiple of 64 (the launcher sends other multiplicities to bwd_pair_kernel)")
    A("  const int nchunk = mul >> 6;")
    A("  const int64_t witem = (int64_t)spec_xcd_remap(blockIdx.x, gridDim.x) * 4 + wid;")
    A("  const int64_t item = witem / WPN;")
    A("  const int wsub = (int)(witem - item * WPN);")
    A("  const bool valid = item < (int64_t)a.N * nchunk;  // (WPN < 4: the last workgroup may hold idle wavefronts)")
    A("  const int node = spec_uniform(valid ? (int)(item / nchunk) : 0);")
    A("  const int chunk = valid ? (int)(item - (int64_t)node * nchunk) : 0;")
    A("  const int u = chunk * 64 + lane;")
    A("  constexpr bool act = true, DUAL = false;")
    A("  const int beg = a.rowptr[node], end = valid ? a.rowptr[node + 1] : beg;")
    L.extend(lane_offsets(p, "  ", want_x=True, want_g=True))
    A("  const unsigned wbase = (unsigned)wid * (unsigned)kRingWaveBytes;  // this wavefront's ring (LDS byte address)")
    A("  const unsigned l4 = (unsigned)lane * 4u, l16 = (unsigned)lane * 16u;")
    A("  // per-lane source offsets of the copies (bytes from the row base; lane l moves 16 bytes)")
    L.extend(ring_lane_offsets(p, r, "  ", "ro"))
    A("  T gvO[kOD], gxO[kXD];")
    L.extend(load_g(p, "  ", "a.g + (int64_t)node * a.dout", "gvO"))
    L.extend(load_x(p, "  ", "(a.x + (int64_t)node * a.din)", sfx="O"))
    A("#pragma unroll")
    A("  for (int i = 0; i < kXD; ++i) gxO[i] = T(0);")

    # The pair indices (other node, weight row, the two edges) of up to 64 of this wavefront's pairs sit in four vector
    # registers, lane l = the wavefront's l-th pair, fetched by ONE vector load per list before the loop; a pair's
    # indices are then a v_readlane away.  (Per-pair scalar loads, as bwd_pair_kernel has them, are not available here:
    # behind the "memory" clobbers of the copy / wait statements hipcc turns them into vector loads followed by vmcnt(0).)
    def block_load(ind, first_pair):
        return [f"{ind}{{ const int i_ = beg + wsub + (({first_pair}) + lane) * WPN; const int ic_ = i_ < end ? i_ : end - 1;",
                f"{ind}  jnV = a.nbr[ic_]; prV = a.wid[ic_]; eiV = a.eid[ic_]; eoV = a.eid2[ic_]; }}"]

    A("  int idx = beg + wsub;")
    A("  int kk = 0;  // this wavefront's pair counter: pair kk sits in owner slot beg + wsub + kk * WPN")
    A("  int jnA = 0, prA = 0, eiA = 0, eoA = 0, jnB = 0, prB = 0, eiB = 0, eoB = 0, jnC = 0, prC = 0, eiC = 0, eoC = 0;")
    A("  int jnV = 0, prV = 0, eiV = 0, eoV = 0;")
    A("  bool hasA = idx < end, hasB = idx + WPN < end, hasC = false;")
    A("  if (hasA) {")
    L.extend(block_load("    ", "0"))
    L.extend(_ring_index_get("A", "0", "    "))
    L.extend(_ring_index_get("B", "1", "    "))
    A("  }")
    A("  // prologue: the whole first pair and the first chunk of the second fill the ring")
    A("  if (hasA) {")
    for c_ in range(RC):
        L.extend(copies("    ", c_, "A", str(c_), lgkm=False))
    A("  }")
    A("  if (hasB) {")
    L.extend(copies("    ", 0, "B", str(RC), lgkm=False))
    A("  }")
    A("  // the owner's rows are in their registers before the loop starts: hipcc, which does not see the copies, would")
    A("  // otherwise wait for them inside the loop with a small vmcnt(n) of ITS count -- every iteration, draining the ring")
    A("#pragma unroll")
    A("  for (int k = 0; k < kOD; ++k) asm volatile(\"\" : \"+v\"(gvO[k]));")
    for b in p.used_blocks:
        for i in range(2 * st.in1_ls[b] + 1):
            A(f"  asm volatile(\"\" : \"+v\"(xb{b}O[{i}]));")
    A("  int rot = 0;       // slot of chunk 0 of pair A")
    A("  bool first = true;")
    A("  T qI[kS], qX[kS], gxa[kXD], gvJ[kOD];")
    L.extend(decl_y(p, "  ", "I") + decl_y(p, "  ", "X") + decl_x(p, "  ", "J"))
    L.extend(decl_x(p, "  ", "J2") + decl_x(p, "  ", "O2"))  # (names the shared path emitter mentions under DUAL, never read)
    A("  while (hasA) {")
    A("    hasC = idx + 2 * WPN < end;")
    A("    if (hasC) {")
    A("      if (((kk + 2) & 63) == 0) {  // (a wavefront with more than 64 pairs: the next block of indices)")
    L.extend(block_load("        ", "kk + 2"))
    A("      }")
    L.extend(_ring_index_get("C", "kk + 2", "      "))
    A("    }")
    A("    T* __restrict__ gwr_e = a.gw + (int64_t)prA * a.wn;")
    A("    T* __restrict__ gxr = a.gxe + (int64_t)(ATOM ? jnA : idx) * a.din;")
    A("#pragma unroll")
    A("    for (int j = 0; j < kS; ++j) { qI[j] = T(0); qX[j] = T(0); }")
    for c_ in range(RC):
        lo = r.lds_off[c_]
        A(f"    {{  // ---- chunk {c_}: paths {r.cpaths[c_][0]}..{r.cpaths[c_][-1]}")
        A(f"      int s_ = rot + {c_}; s_ = s_ >= kRingSlots ? s_ - kRingSlots : s_;")
        A("      const unsigned sb = wbase + (unsigned)s_ * (unsigned)kRingSlotBytes;")
        A("      const unsigned char* __restrict__ cb = nqa_smem + sb;")
        L.extend(ring_waits(r, c_, "      "))
        L.extend(ring_operand_reads(p, r, c_, p.used_y, "      "))
        for pth in r.cpaths[c_]:
            b_, j, s_ = st.instr[pth]
            d1, d3 = 2 * st.in1_ls[b_] + 1, 2 * st.out_ls[s_] + 1
            if p.first_path[b_] == pth:
                for i in range(d1):
                    A(f"      gxa[{p.xpre[b_] + i}] = T(0);")
            A(f"      {{  // path {pth}")
            A(f"        const T wv_ = *reinterpret_cast<const T*>(cb + {lo[('w', pth)]} + l4);")
            for k in range(d3):
                A(f"        gvJ[{p.opre[s_] + k}] = T({p.slot_coeff[s_]!r}) * *reinterpret_cast<const T*>(cb + {lo[('g', s_)]} + l4 * {d3}u + {4 * k});")
            live_i, gx_i = path_terms(p, L, pth, "J", "gvO", "I", "i", "        ", dual=True)
            for comp, expr in gx_i:
                if expr:
                    A(f"        if (GX) gxa[{comp}] += wv_ * ({expr});")
            live_x, gx_x = path_terms(p, L, pth, "O", "gvJ", "X", "x", "        ", dual=True)
            for comp, expr in gx_x:
                if expr:
                    A(f"        if (GX) gxO[{comp}] += wv_ * ({expr});")
            terms = [f"yb{j}I[{jj}] * Bi{jj}" for jj in live_i] + [f"yb{j}X[{jj}] * Bx{jj}" for jj in live_x]
            gw_expr = " + ".join(terms) if terms else "T(0)"
            A(f"        {{ const T r_ = {gw_expr}; {emit_store(f'spec_at(gwr_e + (unsigned)(mul * {pth}), ucb)', 'r_')}; }}")
            for jj in live_i:
                A(f"        qI[{p.ypre[j] + jj}] += wv_ * Bi{jj};")
            for jj in live_x:
                A(f"        qX[{p.ypre[j] + jj}] += wv_ * Bx{jj};")
            A("      }")
            if p.last_path[b_] == pth:
                A("      if (GX) {")
                for i in range(d1):
                    st_ = emit_store(f'spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb)', f'gxa[{p.xpre[b_] + i}]')
                    A(f"        if (ATOM) unsafeAtomicAdd(spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb), gxa[{p.xpre[b_] + i}]); else {st_};")
                A("      }")
        if c_ == RC - 1:
            if p.unused_comps:
                A("      if (GX && !ATOM) {")
                for i in p.unused_comps:
                    A(f"        *spec_at(gxr + (unsigned)(mul * {i}), ucb) = T(0);")
                A("      }")
            A("      // refill this slot with chunk 0 of the pair after next")
            A("      if (hasC) {")
            L.extend(copies("        ", 0, "C", "s_"))
            A("      }")
            A("      // (a.gy_atomic: more than one channel chunk per edge -- the chunks add into grad_y itself instead of partial rows)")
            A("      spec_wave_reduce_store<T, kS>(qI, a.gy + (int64_t)eiA * a.gy_stride + (a.gy_atomic ? 0 : chunk * kS), lane, a.gy_atomic != 0);")
            A("      spec_wave_reduce_store<T, kS>(qX, a.gy + (int64_t)eoA * a.gy_stride + (a.gy_atomic ? 0 : chunk * kS), lane, a.gy_atomic != 0);")
        else:
            A(f"      // refill this slot with chunk {c_ + 1} of the next pair")
            A("      if (hasB) {")
            L.extend(copies("        ", c_ + 1, "B", "s_"))
            A("      }")
        A("    }")
    A("    jnA = jnB; prA = prB; eiA = eiB; eoA = eoB; jnB = jnC; prB = prC; eiB = eiC; eoB = eoC;")
    A("    hasA = hasB; hasB = hasC; idx += WPN; ++kk; first = false;")
    A(f"    rot += {RC}; rot = rot >= kRingSlots ? rot - kRingSlots : rot;")
    A("  }")
    A("  if (!GX) return;")
    A("  // grad_x[owner]: the owner-side contributions of all its pairs (the other side arrives through the rows)")
    A("  if (WPN > 1) {")
    A("    T* red = reinterpret_cast<T*>(nqa_smem);  // (the rings are idle: every copy was waited for)")
    A("    __syncthreads();")
    A("    if (wsub > 0) {")
    A("#pragma unroll")
    A("      for (int k = 0; k < kXD; ++k) red[(((wid / WPN) * (WPN - 1) + wsub - 1) * kXD + k) * 64 + lane] = gxO[k];")
    A("    }")
    A("    __syncthreads();")
    A("    if (wsub > 0) return;")
    A("#pragma unroll")
    A("    for (int k = 0; k < kXD; ++k) {")
    A("#pragma unroll")
    A("      for (int w2 = 0; w2 < WPN - 1; ++w2) gxO[k] += red[(((wid / WPN) * (WPN - 1) + w2) * kXD + k) * 64 + lane];")
    A("    }")
    A("  }")
    A("  if (valid) {")
    A("    T* __restrict__ ob = a.out + (int64_t)node * a.din;")
    L.extend(store_x_rows(p, "    ", range(p.NB), "u", lambda c: f"gxO[{c}]"))
    A("  }")
    A("}")
    return L


def _ring_index_get(sfx, k, ind):
    return [f"{ind}jn{sfx} = __builtin_amdgcn_readlane(jnV, ({k}) & 63); pr{sfx} = __builtin_amdgcn_readlane(prV, ({k}) & 63);",
            f"{ind}ei{sfx} = __builtin_amdgcn_readlane(eiV, ({k}) & 63); eo{sfx} = __builtin_amdgcn_readlane(eoV, ({k}) & 63);"]


def _split_part_sets(st: Structure, paths):
    return (sorted({st.instr[p_][0] for p_ in paths}), sorted({st.instr[p_][2] for p_ in paths}),
            sorted({st.instr[p_][1] for p_ in paths}))


def _split_load_g(p: Plan, ind, rowexpr, name, slots):
    out = [f"{ind}{{ const T* __restrict__ gb = {rowexpr};"]
    for s_ in slots:
        for k in range(2 * p.st.out_ls[s_] + 1):
            out.append(f"{ind}  {name}[{p.opre[s_] + k}] = spec_at(gb, go{s_})[{k}];")
    for s_ in slots:
        for k in range(2 * p.st.out_ls[s_] + 1):
            out.append(f"{ind}  {name}[{p.opre[s_] + k}] = act ? T({p.slot_coeff[s_]!r}) * {name}[{p.opre[s_] + k}] : T(0);")
    out.append(f"{ind}}}")
    return out


def _split_load_x(p: Plan, ind, rowexpr, sfx, blocks):
    return [f"{ind}xb{b}{sfx}[{i}] = spec_at({rowexpr}, xo{b})[{i}];" for b in blocks for i in range(2 * p.st.in1_ls[b] + 1)]


def _split_part_registers(p: Plan, blocks, ys):
    return ([f"      T xb{b}O[{2 * p.st.in1_ls[b] + 1}], xb{b}J[{2 * p.st.in1_ls[b] + 1}];" for b in blocks]
            + [f"      T yb{j}I[{2 * p.st.in2_ls[j] + 1}], yb{j}X[{2 * p.st.in2_ls[j] + 1}];" for j in ys])


def _split_item(L):
    L += ["  const int64_t item = (int64_t)spec_xcd_remap(blockIdx.x, gridDim.x) * 4 + wid;",
          "  if (item >= (int64_t)a.N * nchunk * kPairParts) return;",
          "  const int node = spec_uniform((int)(item / (nchunk * kPairParts)));",
          "  const int rem = (int)(item - (int64_t)node * (nchunk * kPairParts));",
          "  const int chunk = spec_uniform(rem / kPairParts);",
          "  const int part = spec_uniform(rem - chunk * kPairParts);",
          "  const int u = chunk * 64 + lane;"]


def _nohoist(p: Plan, slots, ind):
    # the owner-side intermediates T_ij = sum_k C_ijk grad_out[owner]_k are the same for all pairs; hoisted out of the pair
    # loop they are ~150 live values for the l_1 = 3 block (79 spilled registers).  An empty asm that "modifies" the
    # owner's slots makes them per-pair values.
    return [f"{ind}asm volatile(\"\" : \"+v\"(gvO[{p.opre[s_] + k}]));" for s_ in slots for k in range(2 * p.st.out_ls[s_] + 1)]


# ------------------------------------------------------------------ pair-centric backward, split by input block
# Structures whose two grad_out rows do not fit one wavefront's registers (l_max = 3: 99 values each): every input
# block l_1 owns its paths, its output slots, its weight columns and its grad_x components, so the pair kernel splits
# over PS wavefronts per (node, channel chunk) with no exchange -- wavefront `part` holds only its blocks' slice of
# grad_out[owner] / grad_out[other] / x / w.  Shared by the parts: the two y rows and the pair indices (scalar loads).
# grad_y: every part reduces its own partial sums into a [chunk, part] slot of the partial buffer (summed by
# spec_gy_reduce_kernel, as the chunk partials are).
def emit_pair_split(p: Plan) -> List[str]:
    st = p.st
    L = []
    A = L.append
    A(f"constexpr int kPairParts = {p.pair_parts};")
    A("// ATOM (multiples of 64 channels): the other node's grad_x by atomics into the zeroed [N, dim_in1] accumulator a.gxe")
    A("// (see bwd_pair_ring_kernel) instead of one row per pair")
    A("template <typename T, bool FULL, bool GX, bool ATOM = false>")
    A("__global__ __launch_bounds__(256, 2) void bwd_pair_split_kernel(const SpecArgs<T> a) {")
    A("  const int lane = threadIdx.x & 63;")
    A("  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));")
    A("  const int mul = a.mul;")
    A("  const int nchunk = (mul + 63) >> 6;")
    _split_item(L)
    A("  const bool act = FULL || (u < mul);")
    A("  const int beg = a.rowptr[node], end = a.rowptr[node + 1];")
    L.extend(lane_offsets(p, "  ", want_x=True, want_g=True))
    A("  switch (part) {")
    for part_i, paths in enumerate(p.part_paths):
        blocks, slots, ys = _split_part_sets(st, paths)
        A(f"    case {part_i}: {{  // input blocks {blocks}: paths {paths}")
        A("      T gvO[kOD], gvJ[kOD], gxO[kXD], wv[kNP];")
        L.extend(_split_part_registers(p, blocks, ys))
        L.extend(_split_load_g(p, "      ", "a.g + (int64_t)node * a.dout", "gvO", slots))
        L.extend(_split_load_x(p, "      ", "(a.x + (int64_t)node * a.din)", "O", blocks))
        for b in blocks:
            for i in range(2 * st.in1_ls[b] + 1):
                A(f"      gxO[{p.xpre[b] + i}] = T(0);")
        A("      for (int idx = beg; idx < end; ++idx) {")
        A("        const int j_ = spec_uniform(a.nbr[idx]), pr = spec_uniform(a.wid[idx]);")
        A("        const int ei = spec_uniform(a.eid[idx]), eo = spec_uniform(a.eid2[idx]);")
        A("        const T* __restrict__ xr = a.x + (int64_t)j_ * a.din;")
        A("        const T* __restrict__ wr = a.w + (int64_t)pr * a.wn;")
        A("        const T* __restrict__ yi = a.y + (int64_t)ei * kS;")
        A("        const T* __restrict__ yo = a.y + (int64_t)eo * kS;")
        for pth in paths:
            A(f"        wv[{pth}] = *spec_at(wr + (unsigned)(mul * {pth}), ucb);")
        L.extend(_split_load_x(p, "        ", "xr", "J", blocks))
        L.extend(_split_load_g(p, "        ", "a.g + (int64_t)j_ * a.dout", "gvJ", slots))
        for j in ys:
            for i in range(2 * st.in2_ls[j] + 1):
                A(f"        yb{j}I[{i}] = yi[{p.ypre[j] + i}]; yb{j}X[{i}] = yo[{p.ypre[j] + i}];")
        if n_owner_terms(st, paths) > SPLIT_NOHOIST:
            L.extend(_nohoist(p, slots, "        "))
        A("        T qI[kS], qX[kS], gxa[kXD];")
        A("#pragma unroll")
        A("        for (int j = 0; j < kS; ++j) { qI[j] = T(0); qX[j] = T(0); }")
        A("        T* __restrict__ gwr_e = a.gw + (int64_t)pr * a.wn;")
        A("        T* __restrict__ gxr = a.gxe + (int64_t)(ATOM ? j_ : idx) * a.din;")
        for pth in paths:
            b_, j, s_ = st.instr[pth]
            d1 = 2 * st.in1_ls[b_] + 1
            if p.first_path[b_] == pth:
                for i in range(d1):
                    A(f"        gxa[{p.xpre[b_] + i}] = T(0);")
            A(f"        {{  // path {pth}")
            live_i, gx_i = path_terms(p, L, pth, "J", "gvO", "I", "i", "          ", dual=False)
            for comp, expr in gx_i:
                if expr:
                    A(f"          if (GX) gxa[{comp}] += wv[{pth}] * ({expr});")
            live_x, gx_x = path_terms(p, L, pth, "O", "gvJ", "X", "x", "          ", dual=False)
            for comp, expr in gx_x:
                if expr:
                    A(f"          if (GX) gxO[{comp}] += wv[{pth}] * ({expr});")
            terms = [f"yb{j}I[{jj}] * Bi{jj}" for jj in live_i] + [f"yb{j}X[{jj}] * Bx{jj}" for jj in live_x]
            gw_expr = " + ".join(terms) if terms else "T(0)"
            A(f"          {{ const T r_ = {gw_expr}; if (act) {emit_store(f'spec_at(gwr_e + (unsigned)(mul * {pth}), ucb)', 'r_')}; }}")
            for jj in live_i:
                A(f"          qI[{p.ypre[j] + jj}] += wv[{pth}] * Bi{jj};")
            for jj in live_x:
                A(f"          qX[{p.ypre[j] + jj}] += wv[{pth}] * Bx{jj};")
            A("        }")
            if p.last_path[b_] == pth:
                A("        if (GX && act) {")
                for i in range(d1):
                    st_ = emit_store(f'spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb)', f'gxa[{p.xpre[b_] + i}]')
                    A(f"          if (ATOM) unsafeAtomicAdd(spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb), gxa[{p.xpre[b_] + i}]); else {st_};")
                A("        }")
        if part_i == 0 and p.unused_comps:
            A("        if (GX && act && !ATOM) {")
            for i in p.unused_comps:
                A(f"          *spec_at(gxr + (unsigned)(mul * {i}), ucb) = T(0);")
            A("        }")
        A("        spec_mask_dup<T, kS>(qI, u < mul);")
        A("        spec_mask_dup<T, kS>(qX, u < mul);")
        A(f"        spec_wave_reduce_store<T, kS>(qI, a.gy + (int64_t)ei * a.gy_stride + (chunk * kPairParts + {part_i}) * kS, lane);")
        A(f"        spec_wave_reduce_store<T, kS>(qX, a.gy + (int64_t)eo * a.gy_stride + (chunk * kPairParts + {part_i}) * kS, lane);")
        A("      }")
        A("      if (GX && act) {")
        A("        const int uc = u < mul ? u : mul - 1;")
        A("        T* __restrict__ ob = a.out + (int64_t)node * a.din;")
        L.extend(_split_part_x_rows(p, part_i, blocks, "uc"))
        A("      }")
        A("    } break;")
    A("    default: break;")
    A("  }")
    A("}")
    return L


def _split_part_x_rows(p: Plan, part_i, blocks, uvar):
    """A part's grad_x[owner] components; part 0 also zeroes the components of the blocks no path reads."""
    out = store_x_rows(p, "        ", blocks, uvar, lambda c: f"gxO[{c}]")
    if part_i == 0:
        out += store_x_rows(p, "        ", [b for b in range(p.NB) if b not in p.first_path], uvar, lambda c: "T(0)")
    return out


# ------------------------------------------------------------------ split pair kernel on the LDS ring
# The l_max = 3 structures' pair kernel (one wavefront per (node, chunk, input block)) walked its pairs with a plain loop:
# indices -> rows -> arithmetic -> stores, nothing of the next pair requested (the registers hold two grad_out slices).
# The same ring as bwd_pair_ring_kernel, per part: the part's slice of w / x[other] / grad_out[other] and the two y rows
# of the NEXT pair travel by LDS-DMA while this pair is evaluated out of the LDS.
def emit_split_ring(p: Plan) -> List[str]:
    st = p.st
    L = []
    A = L.append
    A("// (see bwd_pair_ring_kernel for the ring, the counted waits and ATOM; parts as in bwd_pair_split_kernel)")
    A("template <bool GX, bool ATOM>")
    A("__global__ __launch_bounds__(256, 2) void bwd_pair_split_ring_kernel(const SpecArgs<float> a) {")
    A("  typedef float T;")
    A("  extern __shared__ __align__(16) unsigned char nqa_smem[];")
    A("  const int lane = threadIdx.x & 63;")
    A("  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));")
    A("  const int mul = a.mul;  // a multiple of 64")
    A("  const int nchunk = mul >> 6;")
    _split_item(L)
    A("  constexpr bool act = true;")
    A("  const int beg = a.rowptr[node], end = a.rowptr[node + 1];")
    L.extend(lane_offsets(p, "  ", want_x=True, want_g=True))
    A(f"  const unsigned wbase = (unsigned)wid * {RING_WAVE_BYTES}u;  // this wavefront's ring (LDS byte address)")
    A("  const unsigned l4 = (unsigned)lane * 4u, l16 = (unsigned)lane * 16u;")
    A("  switch (part) {")
    for part_i, paths in enumerate(p.part_paths):
        blocks, slots, ys = _split_part_sets(st, paths)
        r = p.split_rings[part_i]
        RC, RN, RSLOT = r.chunks, r.slots, r.slot_bytes
        pfx = f"p{part_i}"

        def copies(ind, c_, sfx, slotexpr, lgkm=True):
            return ring_copies(p, r, ind, c_, sfx, slotexpr, f"{RSLOT}u", f"{pfx}ro", "", lgkm)

        def blk_load(ind, first_pair):
            return [f"{ind}{{ const int i_ = beg + ({first_pair}) + lane; const int ic_ = i_ < end ? i_ : end - 1;",
                    f"{ind}  jnV = a.nbr[ic_]; prV = a.wid[ic_]; eiV = a.eid[ic_]; eoV = a.eid2[ic_]; }}"]

        A(f"    case {part_i}: {{  // input blocks {blocks}: paths {paths}; ring of {RN} slots of {RSLOT} bytes, {RC} chunk(s) per pair, {r.copies} copies")
        L.extend(ring_lane_offsets(p, r, "      ", f"{pfx}ro"))
        A("      T gvO[kOD], gvJ[kOD], gxO[kXD], qI[kS], qX[kS], gxa[kXD];")
        L.extend(_split_part_registers(p, blocks, ys))
        L.extend(_split_load_g(p, "      ", "a.g + (int64_t)node * a.dout", "gvO", slots))
        L.extend(_split_load_x(p, "      ", "(a.x + (int64_t)node * a.din)", "O", blocks))
        for b in blocks:
            for i in range(2 * st.in1_ls[b] + 1):
                A(f"      gxO[{p.xpre[b] + i}] = T(0);")
        A("      int idx = beg, kk = 0;")
        A("      int jnA = 0, prA = 0, eiA = 0, eoA = 0, jnB = 0, prB = 0, eiB = 0, eoB = 0, jnC = 0, prC = 0, eiC = 0, eoC = 0;")
        A("      int jnV = 0, prV = 0, eiV = 0, eoV = 0;")
        A("      bool hasA = idx < end, hasB = idx + 1 < end, hasC = false;")
        A("      if (hasA) {")
        L.extend(blk_load("        ", "0"))
        L.extend(_ring_index_get("A", "0", "        "))
        L.extend(_ring_index_get("B", "1", "        "))
        for c_ in range(RC):
            L.extend(copies("        ", c_, "A", str(c_), lgkm=False))
        A("      }")
        A("      if (hasB) {")
        L.extend(copies("        ", 0, "B", str(RC), lgkm=False))
        A("      }")
        A("      // (the owner's rows are in their registers before the loop starts: see bwd_pair_ring_kernel)")
        L.extend(_nohoist(p, slots, "      "))
        for b in blocks:
            for i in range(2 * st.in1_ls[b] + 1):
                A(f"      asm volatile(\"\" : \"+v\"(xb{b}O[{i}]));")
        A("      int rot = 0;")
        A("      bool first = true;")
        A("      while (hasA) {")
        A("        hasC = idx + 2 < end;")
        A("        if (hasC) {")
        A("          if (((kk + 2) & 63) == 0) {")
        L.extend(blk_load("            ", "kk + 2"))
        A("          }")
        L.extend(_ring_index_get("C", "kk + 2", "          "))
        A("        }")
        A("        T* __restrict__ gwr_e = a.gw + (int64_t)prA * a.wn;")
        A("        T* __restrict__ gxr = a.gxe + (int64_t)(ATOM ? jnA : idx) * a.din;")
        A("#pragma unroll")
        A("        for (int j = 0; j < kS; ++j) { qI[j] = T(0); qX[j] = T(0); }")
        if n_owner_terms(st, paths) > SPLIT_NOHOIST:
            L.extend(_nohoist(p, slots, "        "))
        for c_ in range(RC):
            lo = r.lds_off[c_]
            A(f"        {{  // ---- chunk {c_}: paths {r.cpaths[c_]}")
            A(f"          int s_ = rot + {c_}; s_ = s_ >= {RN} ? s_ - {RN} : s_;")
            A(f"          const unsigned char* __restrict__ cb = nqa_smem + (wbase + (unsigned)s_ * {RSLOT}u);")
            L.extend(ring_waits(r, c_, "          "))
            L.extend(ring_operand_reads(p, r, c_, ys, "          "))
            for pth in r.cpaths[c_]:
                b_, j, s_ = st.instr[pth]
                d1, d3 = 2 * st.in1_ls[b_] + 1, 2 * st.out_ls[s_] + 1
                if p.first_path[b_] == pth:
                    for i in range(d1):
                        A(f"          gxa[{p.xpre[b_] + i}] = T(0);")
                A(f"        {{  // path {pth}")
                A(f"          const T wv_ = *reinterpret_cast<const T*>(cb + {lo[('w', pth)]} + l4);")
                for k in range(d3):
                    A(f"          gvJ[{p.opre[s_] + k}] = T({p.slot_coeff[s_]!r}) * *reinterpret_cast<const T*>(cb + {lo[('g', s_)]} + l4 * {d3}u + {4 * k});")
                live_i, gx_i = path_terms(p, L, pth, "J", "gvO", "I", "i", "          ", dual=False)
                for comp, expr in gx_i:
                    if expr:
                        A(f"          if (GX) gxa[{comp}] += wv_ * ({expr});")
                live_x, gx_x = path_terms(p, L, pth, "O", "gvJ", "X", "x", "          ", dual=False)
                for comp, expr in gx_x:
                    if expr:
                        A(f"          if (GX) gxO[{comp}] += wv_ * ({expr});")
                terms = [f"yb{j}I[{jj}] * Bi{jj}" for jj in live_i] + [f"yb{j}X[{jj}] * Bx{jj}" for jj in live_x]
                gw_expr = " + ".join(terms) if terms else "T(0)"
                A(f"          {{ const T r_ = {gw_expr}; {emit_store(f'spec_at(gwr_e + (unsigned)(mul * {pth}), ucb)', 'r_')}; }}")
                for jj in live_i:
                    A(f"          qI[{p.ypre[j] + jj}] += wv_ * Bi{jj};")
                for jj in live_x:
                    A(f"          qX[{p.ypre[j] + jj}] += wv_ * Bx{jj};")
                A("        }")
                if p.last_path[b_] == pth:
                    A("          if (GX) {")
                    for i in range(d1):
                        st_ = emit_store(f'spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb)', f'gxa[{p.xpre[b_] + i}]')
                        A(f"            if (ATOM) unsafeAtomicAdd(spec_at(gxr + (unsigned)(mul * {p.xpre[b_] + i}), ucb), gxa[{p.xpre[b_] + i}]); else {st_};")
                    A("          }")
            if c_ == RC - 1:
                if part_i == 0 and p.unused_comps:
                    A("          if (GX && !ATOM) {")
                    for i in p.unused_comps:
                        A(f"            *spec_at(gxr + (unsigned)(mul * {i}), ucb) = T(0);")
                    A("          }")
                A("          if (hasC) {")
                L.extend(copies("            ", 0, "C", "s_"))
                A("          }")
                A(f"          spec_wave_reduce_store<T, kS>(qI, a.gy + (int64_t)eiA * a.gy_stride + (a.gy_atomic ? 0 : (chunk * kPairParts + {part_i}) * kS), lane, a.gy_atomic != 0);")
                A(f"          spec_wave_reduce_store<T, kS>(qX, a.gy + (int64_t)eoA * a.gy_stride + (a.gy_atomic ? 0 : (chunk * kPairParts + {part_i}) * kS), lane, a.gy_atomic != 0);")
            else:
                A("          if (hasB) {")
                L.extend(copies("            ", c_ + 1, "B", "s_"))
                A("          }")
            A("        }")
        A("        jnA = jnB; prA = prB; eiA = eiB; eoA = eoB; jnB = jnC; prB = prC; eiB = eiC; eoB = eoC;")
        A("        hasA = hasB; hasB = hasC; ++idx; ++kk; first = false;")
        A(f"        rot += {RC}; rot = rot >= {RN} ? rot - {RN} : rot;")
        A("      }")
        A("      if (GX) {")
        A("        T* __restrict__ ob = a.out + (int64_t)node * a.din;")
        L.extend(_split_part_x_rows(p, part_i, blocks, "u"))
        A("      }")
        A("    } break;")
    A("    default: break;")
    A("  }")
    A("}")
    return L


def emit_gx_kernels(p: Plan) -> List[str]:
    """The last steps of grad_x: the accumulator form of the pair kernels (ATOM) and the per-source-node sum of the rows."""
    st = p.st
    L = []
    A = L.append
    if p.pair_parts:
        A("// a.out[n] += the accumulator row of n (ATOM forms of the pair kernels), re-ordered from component rows to the irreps layout")
        A("__global__ __launch_bounds__(256) void gx_acc_finish_kernel(const SpecArgs<float> a) {")
        A("  const int mul = a.mul;")
        A("  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;  // one thread per (node, channel)")
        A("  if (t >= (int64_t)a.N * mul) return;")
        A("  const int64_t node = t / mul;")
        A("  const int u = (int)(t - node * mul);")
        A("  const float* __restrict__ acc = a.gxe + node * a.din + u;")
        A("  float* __restrict__ ob = a.out + node * a.din;")
        for b in p.used_blocks:
            d = 2 * st.in1_ls[b] + 1
            for i in range(d):
                A(f"  ob[(int64_t)mul * {p.xpre[b]} + (int64_t)u * {d} + {i}] += acc[(int64_t)mul * {p.xpre[b] + i}];")
        A("}")
    A("// ACC: add the rows to what a.out already holds (pair-centric backward: the owner-side sums) instead of overwriting")
    A("template <typename T, bool ACC>")
    A("__global__ __launch_bounds__(256) void gx_rows_sum_kernel(const SpecArgs<T> a) {")
    A("  const int lane = threadIdx.x & 63;")
    A("  const int wid = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));")
    A("  const int mul = a.mul;")
    A("  const int nchunk = (mul + 63) >> 6;")
    A("  const int64_t item = (int64_t)spec_xcd_remap(blockIdx.x, gridDim.x) * 4 + wid;")
    A("  if (item >= (int64_t)a.N * nchunk) return;")
    A("  const int node = spec_uniform((int)(item / nchunk));")
    A("  const int chunk = (int)(item - (int64_t)node * nchunk);")
    A("  const int u = chunk * 64 + lane;")
    A("  const bool act = u < mul;")
    A("  T acc[kXD];")
    A("#pragma unroll")
    A("  for (int i = 0; i < kXD; ++i) acc[i] = T(0);")
    A("  const int beg = a.rowptr[node], end = a.rowptr[node + 1];")
    A("  const T* __restrict__ base = a.gxe + (act ? u : 0);")
    A("  int idx = beg;")
    A("  for (; idx + 4 <= end; idx += 4) {")
    A("    const int e0 = a.eid[idx], e1 = a.eid[idx + 1], e2 = a.eid[idx + 2], e3 = a.eid[idx + 3];")
    A("    T r0[kXD], r1[kXD], r2[kXD], r3[kXD];")
    A("#pragma unroll")
    A("    for (int i = 0; i < kXD; ++i) {")
    A("      r0[i] = base[(int64_t)e0 * a.din + (int64_t)mul * i];")
    A("      r1[i] = base[(int64_t)e1 * a.din + (int64_t)mul * i];")
    A("      r2[i] = base[(int64_t)e2 * a.din + (int64_t)mul * i];")
    A("      r3[i] = base[(int64_t)e3 * a.din + (int64_t)mul * i];")
    A("    }")
    A("#pragma unroll")
    A("    for (int i = 0; i < kXD; ++i) acc[i] += (r0[i] + r1[i]) + (r2[i] + r3[i]);")
    A("  }")
    A("  for (; idx < end; ++idx) {")
    A("    const int e0 = a.eid[idx];")
    A("#pragma unroll")
    A("    for (int i = 0; i < kXD; ++i) acc[i] += base[(int64_t)e0 * a.din + (int64_t)mul * i];")
    A("  }")
    A("  if (act) {")
    A("    T* __restrict__ ob = a.out + (int64_t)node * a.din;")
    for b in range(p.NB):
        d = 2 * st.in1_ls[b] + 1
        for i in range(d):
            A(f"    {{ T* o_ = ob + ((int64_t)mul * {p.xpre[b]} + (int64_t)u * {d} + {i}); *o_ = ACC ? *o_ + acc[{p.xpre[b] + i}] : acc[{p.xpre[b] + i}]; }}")
    A("  }")
    A("}")
    return L


def emit_launcher(p: Plan) -> List[str]:
    """launch<WPN>(SpecKernel, ...) for every member of tp_spec.h's SpecKernel, and the structure's registration (closes the
    namespaces).  The launcher reads no environment: what the dispatcher decided arrives in SpecLaunchOpts."""
    st = p.st
    L = []
    A = L.append
    pair_operands = "a.gw == nullptr || a.gy == nullptr || a.eid2 == nullptr"
    # (NQA_LAB: scripts/micro/pair_lab.hip includes a generated file and launches single instantiations itself)
    A("#ifndef NQA_LAB")
    A("template <int WPN>")
    A("static int launch(SpecKernel which, const SpecLaunchOpts& o, const SpecArgs<float>& a, hipStream_t stream) {")
    A("  const int nchunk = (a.mul + 63) / 64;")
    A("  const int64_t items = (int64_t)a.N * nchunk;")
    # FULL for EVERY multiplicity: a lane beyond the last channel works on the clamped channel -- same loads, same
    # arithmetic, and it rewrites its twin's stores with identical values; only the wave reductions (grad_y) mask it out
    # (spec_mask_dup) and the owner-side stores use the clamped channel.  The FULL = false instantiations (one exec-mask
    # branch region per store: 155 spilled registers in the l_max = 3 split pair kernel that the 32-channel segments of the
    # L preset ran) remain behind NQA_SPEC_MASKED=1 (SpecLaunchOpts::masked).
    A("  const bool full = (a.mul & 63) == 0 || !o.masked;")
    A("  if (items == 0) return 0;")
    A("  const dim3 blk(256);")
    A("  const dim3 node_grid((unsigned)(WPN == 1 ? (items + 3) / 4 : items));  // fwd / bwd_x: a block per item when split")
    A("  const dim3 edge_grid((unsigned)((items * WPN + 3) / 4));")
    A("  const dim3 rows_grid((unsigned)((items + 3) / 4));")
    A("  const size_t smem_out = WPN > 1 ? (size_t)(WPN - 1) * kOD * 64 * sizeof(float) : 0;")
    A("  const size_t smem_x = WPN > 1 ? (size_t)(WPN - 1) * kXD * 64 * sizeof(float) : 0;")
    A("  switch (which) {")
    A("    case SpecKernel::Fwd:")
    A("      hipLaunchKernelGGL((fwd_kernel<float, WPN, false>), node_grid, blk, smem_out, stream, a);")
    A("      return 0;")
    A("    case SpecKernel::FwdJvp:  // out = F(x2, y, w) + F(x, y2, w) + F(x, y, w2)")
    A("      hipLaunchKernelGGL((fwd_kernel<float, WPN, true>), node_grid, blk, smem_out, stream, a);")
    A("      return 0;")
    A("    case SpecKernel::BwdX:")
    A("      hipLaunchKernelGGL((bwd_x_kernel<float, WPN, false>), node_grid, blk, smem_x, stream, a);")
    A("      return 0;")
    A("    case SpecKernel::BwdXDual:  // out = Bx(y2, w, g) + Bx(y, w2, g)")
    A("      if (a.y2 == nullptr || a.w2 == nullptr) return 1;")
    A("      hipLaunchKernelGGL((bwd_x_kernel<float, WPN, true>), node_grid, blk, smem_x, stream, a);")
    A("      return 0;")
    A("    case SpecKernel::BwdEdge:")
    A("      if (a.gxe != nullptr) {")
    A("        if (a.gw == nullptr || a.gy == nullptr) return 1;")
    for cond, flags in ((None, "true, true, true"), ("a.gw != nullptr && a.gy != nullptr", "false, true, true"),
                        ("a.gw != nullptr", "false, true, false"), ("a.gy != nullptr", "false, false, true")):
        if cond is not None:
            A(f"      }} else if ({cond}) {{")
        A(f"        if (full) hipLaunchKernelGGL((bwd_edge_kernel<float, WPN, {flags}, true>), edge_grid, blk, 0, stream, a); "
          f"else hipLaunchKernelGGL((bwd_edge_kernel<float, WPN, {flags}, false>), edge_grid, blk, 0, stream, a);")
    A("      }")
    A("      return 0;")
    A("    case SpecKernel::RowsSumSrc:")
    A("      hipLaunchKernelGGL((gx_rows_sum_kernel<float, false>), rows_grid, blk, 0, stream, a);")
    A("      return 0;")
    A("    case SpecKernel::RowsSumPairs:  // grad_x += rows of the pairs in which the node is not the owner")
    A("      hipLaunchKernelGGL((gx_rows_sum_kernel<float, true>), rows_grid, blk, 0, stream, a);")
    A("      return 0;")
    A("    case SpecKernel::AccFinish:  // grad_x += the accumulator rows of the atomic form of the pair kernels")
    if p.pair_parts:
        A("      hipLaunchKernelGGL(gx_acc_finish_kernel, dim3((unsigned)(((int64_t)a.N * a.mul + 255) / 256)), blk, 0, stream, a);")
        A("      return 0;")
    else:
        A("      return 1;")
    A("    case SpecKernel::BwdPairsDual:  // see bwd_pair_kernel<DUAL>")
    if p.pair_ok:
        A(f"      if ({pair_operands} || a.x2 == nullptr || a.y2 == nullptr) return 1;")
        A("      if (full) hipLaunchKernelGGL((bwd_pair_kernel<float, WPN, true, false, true>), edge_grid, blk, 0, stream, a);")
        A("      else hipLaunchKernelGGL((bwd_pair_kernel<float, WPN, false, false, true>), edge_grid, blk, 0, stream, a);")
        A("      return 0;")
    else:
        A("      return 1;")
    A("    case SpecKernel::BwdPairs: {  // owner CSR in rowptr / nbr / wid / eid / eid2")
    if p.pair_ok:
        A(f"      if ({pair_operands} || (a.out != nullptr && a.gxe == nullptr)) return 1;")
        if p.ring is not None:
            A("      // LDS-ring kernel: multiples of 64 channels; one wavefront per (node, chunk) when that fills the chip")
            A("      if (o.ring && (a.mul & 63) == 0) {")
            A("        const int rw = items >= 6144 ? 1 : (items >= 3072 ? 2 : 4);")
            A("        const size_t rsmem = (size_t)4 * kRingWaveBytes;")
            A("        const dim3 rgrid((unsigned)((items * rw + 3) / 4));")
            A("#define NQA_RING_LAUNCH(W, GX_, AT_) do { \\")
            A("          static bool lds_ok_[64] = {}; \\")
            A("          if (!spec_allow_lds((const void*)bwd_pair_ring_kernel<W, GX_, AT_>, 4 * kRingWaveBytes, lds_ok_)) return 1; \\")
            A("          hipLaunchKernelGGL((bwd_pair_ring_kernel<W, GX_, AT_>), rgrid, blk, rsmem, stream, a); } while (0)")
            A("#define NQA_RING_WPN(GX_, AT_) do { if (rw == 1) NQA_RING_LAUNCH(1, GX_, AT_); else if (rw == 2) NQA_RING_LAUNCH(2, GX_, AT_); else NQA_RING_LAUNCH(4, GX_, AT_); } while (0)")
            A("        if (a.out == nullptr) NQA_RING_WPN(false, false);")
            A("        else if (a.gx_atomic) NQA_RING_WPN(true, true);")
            A("        else NQA_RING_WPN(true, false);")
            A("#undef NQA_RING_WPN")
            A("#undef NQA_RING_LAUNCH")
            A("        return 0;")
            A("      }")
        A("      if (a.gx_atomic || a.gy_atomic) return 1;  // (the accumulator forms, which only the ring kernel has)")
        A("      if (a.out != nullptr) {")
        A("        if (full) hipLaunchKernelGGL((bwd_pair_kernel<float, WPN, true, true>), edge_grid, blk, smem_x, stream, a);")
        A("        else hipLaunchKernelGGL((bwd_pair_kernel<float, WPN, false, true>), edge_grid, blk, smem_x, stream, a);")
        A("      } else {")
        A("        if (full) hipLaunchKernelGGL((bwd_pair_kernel<float, WPN, true, false>), edge_grid, blk, 0, stream, a);")
        A("        else hipLaunchKernelGGL((bwd_pair_kernel<float, WPN, false, false>), edge_grid, blk, 0, stream, a);")
        A("      }")
        A("      return 0;")
    elif p.pair_parts > 1:
        A(f"      if ({pair_operands} || (a.out != nullptr && a.gxe == nullptr)) return 1;")
        A("      const dim3 grid((unsigned)((items * kPairParts + 3) / 4));  // one wavefront per (node, chunk, part)")
        A("      // LDS-ring form: multiples of 64 channels, with grad_x; otherwise the plain loop")
        A("      if (a.out != nullptr && o.ring && (a.mul & 63) == 0) {")
        A(f"        const size_t rsmem = (size_t)4 * {RING_WAVE_BYTES};")
        A("#define NQA_SRING_LAUNCH(GX_, AT_) do { \\")
        A("          static bool lds_ok_[64] = {}; \\")
        A(f"          if (!spec_allow_lds((const void*)bwd_pair_split_ring_kernel<GX_, AT_>, 4 * {RING_WAVE_BYTES}, lds_ok_)) return 1; \\")
        A("          hipLaunchKernelGGL((bwd_pair_split_ring_kernel<GX_, AT_>), grid, blk, rsmem, stream, a); } while (0)")
        A("        if (a.gx_atomic) NQA_SRING_LAUNCH(true, true); else NQA_SRING_LAUNCH(true, false);")
        A("#undef NQA_SRING_LAUNCH")
        A("        return 0;")
        A("      }")
        A("      if (a.gy_atomic) return 1;  // (only the ring kernel adds into grad_y)")
        A("      if (a.out != nullptr) {")
        A("        if (a.gx_atomic && (a.mul & 63) != 0) return 1;")
        A("        if (a.gx_atomic) hipLaunchKernelGGL((bwd_pair_split_kernel<float, true, true, true>), grid, blk, 0, stream, a);")
        A("        else if (full) hipLaunchKernelGGL((bwd_pair_split_kernel<float, true, true>), grid, blk, 0, stream, a);")
        A("        else hipLaunchKernelGGL((bwd_pair_split_kernel<float, false, true>), grid, blk, 0, stream, a);")
        A("      } else {")
        A("        if (full) hipLaunchKernelGGL((bwd_pair_split_kernel<float, true, false>), grid, blk, 0, stream, a);")
        A("        else hipLaunchKernelGGL((bwd_pair_split_kernel<float, false, false>), grid, blk, 0, stream, a);")
        A("      }")
        A("      return 0;")
    else:
        A("      return 1;  // not generated for this structure (register budget)")
    A("    }")
    A("  }")
    A("  return 1;")
    A("}")
    A("static int launch_any(SpecKernel which, const SpecLaunchOpts& o, const SpecArgs<float>& a, hipStream_t stream) {")
    A("  // LDS budget of the 4-way split: (WPN-1) * accumulators * 256 B per block")
    A("  if (o.wpn >= 4 && kOD <= 64) return launch<4>(which, o, a, stream);")
    A("  return launch<1>(which, o, a, stream);")
    A("}")
    A(f'static SpecRegistrar reg_{st.tag()}("{st.key()}", &launch_any, kXD, kS, kOD, kNP, {p.pair_parts}, {p.ring_flag});')
    A("#endif  // NQA_LAB")
    A("}  // namespace")
    A("}  // namespace nqa")
    return L


def emit_structure(st: Structure) -> str:
    """The generated .hip source of one structure."""
    p = plan_structure(st)
    parts = [emit_header(p), emit_fwd(p), emit_bwd_edge(p), emit_bwd_x(p)]
    if p.pair_ok:
        parts.append(emit_pair(p))
    if p.ring is not None:
        parts.append(emit_pair_ring(p))
    if p.pair_parts > 1:
        parts += [emit_pair_split(p), emit_split_ring(p)]
    parts += [emit_gx_kernels(p), emit_launcher(p)]
    return "\n".join(line for part in parts for line in part) + "\n"


def generate(out_dir: str) -> List[str]:
    os.makedirs(out_dir, exist_ok=True)
    files = []
    for st in baseline_structures():
        path = os.path.join(out_dir, f"tp_spec_{st.name}_{st.tag()}.hip")
        src = emit_structure(st)
        if not os.path.exists(path) or open(path).read() != src:
            with open(path, "w") as f:
                f.write(src)
        files.append(path)
    # drop stale files
    keep = {os.path.basename(p) for p in files}
    for fn in os.listdir(out_dir):
        if fn.startswith("tp_spec_") and fn.endswith(".hip") and fn not in keep:
            os.remove(os.path.join(out_dir, fn))
    return files


MANIFEST = os.path.join(HERE, "generated_spec.manifest.json")


def manifest() -> dict:
    """file name -> {sha256, lines, key} of what the generator emits NOW (the generated sources are not tracked in git;
    tests/test_bench_contract.py pins them to the committed manifest)."""
    out = {}
    for st in baseline_structures():
        src = emit_structure(st)
        out[f"tp_spec_{st.name}_{st.tag()}.hip"] = {"sha256": hashlib.sha256(src.encode()).hexdigest(),
                                                     "lines": src.count("\n") + 1, "key": st.key()}
    return out


if __name__ == "__main__":
    if "--write-manifest" in sys.argv:
        import json

        old = json.load(open(MANIFEST)) if os.path.exists(MANIFEST) else {"note": ""}
        json.dump({"note": old.get("note", ""), "files": manifest()}, open(MANIFEST, "w"), indent=1)
        print("wrote", MANIFEST)
        sys.exit(0)
    fs = generate(os.path.join(HERE, "generated_spec"))
    for st in baseline_structures():
        print(st.name, st.tag(), "paths", len(st.instr), "kOD", sum(2 * l + 1 for l in st.out_ls))
    print(len(fs), "files")
