#!/usr/bin/env python3
"""Read, in the ISA of the built `node_ops.o`, what the stage loops of the per-wavefront node kernels promise
(`node_linear_wave_bf16_unit` in csrc/node_ops.hip, `node_fused_unit` in csrc/node_fused.h).

A stage of these kernels requests the next stage's x slab (and gate scalars) and the next weight fragments while it
multiplies the current ones.  Vector loads return in order, so that only works while no wait in front of a K block's matrix
instructions asks for an empty queue: hipcc writes the waits, and one load inside a wave-uniform branch is enough to turn all
of them into `vmcnt(0)` -- a whole memory latency in front of every block, with nothing in the source to show it.

Checked for `node_linear_wave_bf16_kernel<true>`, `<false>` and `node_fused_kernel`:

  * at most 168 VGPRs (three wavefronts per SIMD), no VGPR spill, no scratch;
  * every stage loop (an innermost loop that holds matrix instructions; one per irrep dimension and template variant)
    requests vector loads and waits for them with counted waits only: no `s_waitcnt vmcnt(0)` inside the loop.

    python scripts/check_node_waits.py [-v] [node_ops.o]      # default: the object of the last build; exit code 1 on a violation

-v prints one line per stage loop: static instructions, matrix instructions, vector loads and the vmcnt waits in order."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_ring_waits as crw  # noqa: E402  (disassemble)
import kernel_resources as kr  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNELS = ("node_linear_wave_bf16_kernelILb1E", "node_linear_wave_bf16_kernelILb0E", "node_fused_kernel")
RES_NAMES = ("node_linear_wave_bf16_kernel<true>", "node_linear_wave_bf16_kernel<false>", "node_fused_kernel(")
MAX_VGPR = 168  # 512 / 3, allocation granularity 8


def kernel_instructions(text):
    """{kernel symbol: [(address, instruction text, branch target address or None)]}"""
    out, cur = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        if cur is None or not line.startswith("\t") or "//" not in line:
            continue
        ins, rest = line.split("//", 1)
        am = re.match(r"\s*([0-9A-Fa-f]+):", rest)
        if not am:
            continue
        addr = int(am.group(1), 16)
        ins = ins.strip()
        target = None
        if ins.startswith(("s_cbranch", "s_branch")):
            off = int(ins.split()[-1])
            off = off - 65536 if off >= 32768 else off
            target = addr + 4 + 4 * off
        cur.append((addr, ins, target))
    return out


def stage_loops(ins):
    """Innermost loops (address ranges closed by a backward branch) that hold matrix instructions."""
    addrs = [a for a, _, _ in ins]
    index = {a: i for i, a in enumerate(addrs)}
    loops = []
    for i, (a, s, t) in enumerate(ins):
        if t is not None and t <= a and t in index:
            lo = index[t]
            if any(x[1].startswith("v_mfma") for x in ins[lo:i + 1]):
                loops.append((lo, i))
    # (block placement can put a unit's prologue loop around the head of its stage loop: ranges overlap without nesting)
    inner = [l for l in loops if not any(o != l and l[0] <= o[0] <= l[1] and (o[0] > l[0] or o[1] < l[1]) for o in loops)]
    return sorted(set(inner))


def check_kernel(ins, verbose, label):
    problems = []
    loops = stage_loops(ins)
    if not loops:
        return 0, ["no stage loop (a loop with matrix instructions) found"]
    for lo, hi in loops:
        body = [s for _, s, _ in ins[lo:hi + 1]]
        waits = [int(m.group(1)) for s in body for m in [re.search(r"vmcnt\((\d+)\)", s)] if m and s.startswith("s_waitcnt")]
        loads = sum(1 for s in body if s.startswith(("global_load", "buffer_load", "flat_load")))
        mfma = sum(1 for s in body if s.startswith("v_mfma"))
        where = f"{label} loop at {ins[lo][0]:#x}"
        if verbose:
            lanes = sum(1 for s in body if s.startswith(("v_readlane", "v_writelane")))  # SGPR spills and reloads
            print(f"  {where}: {len(body)} instructions, {mfma} matrix instructions, {loads} vector loads, "
                  f"{lanes} v_readlane/v_writelane, vmcnt waits {waits}")
        if loads == 0 or not waits:
            problems.append(f"{where}: requests no vector loads / waits for none: not the stage loop this check knows")
        if any(w == 0 for w in waits):
            problems.append(f"{where}: s_waitcnt vmcnt(0) inside the stage loop (waits {waits}): the next stage's loads are drained")
    return len(loops), problems


def main():
    args = [a for a in sys.argv[1:] if a != "-v"]
    verbose = "-v" in sys.argv[1:]
    obj = args[0] if args else os.path.join(ROOT, "nequip_amd", "csrc", "build", "node_ops.o")
    bad = 0
    res = kr.kernels_of(obj)
    for want in RES_NAMES:
        r = [v for k, v in res.items() if want in k]
        if len(r) != 1:
            print(f"{want}: kernel not found in {obj}")
            bad += 1
            continue
        r = r[0]
        print(f"{want.rstrip('(')}: {r['vgpr']} VGPRs, {r['vgpr_spill']} VGPR spills, {r['sgpr_spill']} SGPR spills, scratch {r['scratch']}")
        if r["vgpr"] > MAX_VGPR or r["vgpr_spill"] != 0 or r["scratch"] != 0:
            print(f"{want}: more than {MAX_VGPR} VGPRs, a VGPR spill or scratch")
            bad += 1
    n = 0
    for name, ins in kernel_instructions(crw.disassemble(obj)).items():
        if not any(k in name for k in KERNELS):
            continue
        label = next(r for k, r in zip(KERNELS, RES_NAMES) if k in name).rstrip("(")
        cnt, problems = check_kernel(ins, verbose, label)
        n += cnt
        for p in problems:
            bad += 1
            print(p)
    print(f"{n} stage loops checked, {bad} problem(s)")
    return 1 if bad or not n else 0


if __name__ == "__main__":
    sys.exit(main())
