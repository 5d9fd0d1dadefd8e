"""The stage loops of the per-wavefront node kernels in the ISA of the last build (scripts/check_node_waits.py).

hipcc writes the `s_waitcnt` of these loops.  One vector load inside a wave-uniform branch turns every wait of the loop into
`vmcnt(0)`: the next stage's slab, requested a few instructions earlier, is then waited for in front of every K block, and
nothing in the source shows it.  No GPU needed: `build/node_ops.o` of `python -m nequip_amd.csrc.build` is disassembled and
checked for <= 168 VGPRs, no VGPR spill, no scratch, and counted waits only inside every stage loop of
`node_linear_wave_bf16_kernel<true>`, `<false>` and `node_fused_kernel`."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OBJ = os.path.join(ROOT, "nequip_amd", "csrc", "build", "node_ops.o")
OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"


@pytest.mark.skipif(not os.path.exists(OBJ) or not os.path.exists(OBJDUMP), reason="no build objects / no llvm-objdump here")
def test_node_stage_loops_wait_with_counted_waits_only():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "check_node_waits.py"), "-v"], capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    m = re.search(r"(\d+) stage loops checked, 0 problem\(s\)", r.stdout)
    # five irrep dimensions x (one | two column tiles) x (aligned | element-wise slab loads), the fused kernel's d >= 3 units
    # with and without gate scalars on top: at least 20 loops per kernel
    assert m and int(m.group(1)) >= 60, r.stdout[-3000:]
    for kernel in ("node_linear_wave_bf16_kernel<true>", "node_linear_wave_bf16_kernel<false>", "node_fused_kernel"):
        v = re.search(re.escape(kernel) + r": (\d+) VGPRs, 0 VGPR spills, \d+ SGPR spills, scratch 0", r.stdout)
        assert v and int(v.group(1)) <= 168, r.stdout[:600]
