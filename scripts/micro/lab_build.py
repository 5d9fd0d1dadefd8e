"""Build one pair_lab binary per generated structure (cross-compiles here, runs on the GPU box).

    python scripts/micro/lab_build.py name[:struct][:hipcc-flag,...] ...

e.g.  base  ring::-DLAB_RING  cu:l3n_mid  cusr:l3n_mid:-DLAB_SRING
A structure with a split pair kernel gets -DLAB_SPLIT by itself.  Generated sources go to
nequip_amd/csrc/generated_lab/<name>.hip (next to generated_spec/, so the relative includes hold), binaries to
scripts/micro/lab/<name>.out (both git-ignored; the binaries travel with the GPU job's copy of the tree)."""
import concurrent.futures
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "nequip_amd", "csrc")
LAB_SRC = os.path.join(CSRC, "generated_lab")
LAB_BIN = os.path.join(ROOT, "scripts", "micro", "lab")
sys.path.insert(0, CSRC)

import gen_spec  # noqa: E402


def emit(name, struct):
    st = [s for s in gen_spec.baseline_structures() if s.name == struct][0]
    src = gen_spec.emit_structure(st)
    path = os.path.join(LAB_SRC, name + ".hip")
    if not os.path.exists(path) or open(path).read() != src:
        open(path, "w").write(src)
    return path, "bwd_pair_split_kernel" in src


def compile_one(job):
    name, path, split, flags = job
    out = os.path.join(LAB_BIN, name + ".out")
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", f"-I{CSRC}",
           f"-I{os.path.join(ROOT, 'include')}", f'-DSPEC_FILE="{path}"', "-Wno-unused-value", "-Wno-unused-function"]
    cmd += (["-DLAB_SPLIT"] if split and "-DLAB_SPLIT" not in flags else []) + flags
    cmd += [os.path.join(ROOT, "scripts", "micro", "pair_lab.hip"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    return name, r.returncode, (r.stderr or "")[-3000:]


if __name__ == "__main__":
    os.makedirs(LAB_SRC, exist_ok=True)
    os.makedirs(LAB_BIN, exist_ok=True)
    jobs = []
    for spec in sys.argv[1:]:
        parts = spec.split(":")
        name = parts[0]
        struct = parts[1] if len(parts) > 1 and parts[1] else "l2n_mid"
        flags = [f_ for f_ in parts[2].split(",") if f_] if len(parts) > 2 else []
        path, split = emit(name, struct)
        jobs.append((name, path, split, flags))
    with concurrent.futures.ThreadPoolExecutor(max_workers=6) as ex:
        for name, rc, err in ex.map(compile_one, jobs):
            print(name, "ok" if rc == 0 else f"FAILED\n{err}")
