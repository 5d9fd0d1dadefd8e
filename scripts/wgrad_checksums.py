"""sha256 of every ``nqa_wgrad`` result on the case lists of ``tests/wgrad_cases.py`` (``EXACT_CASES``: every kernel choice at
tile and row edges, typed and untyped, forced split counts; ``ACCURACY_CASES``: real data), to compare two builds bit for bit:

    python scripts/wgrad_checksums.py <tree with a built nequip_amd> <out file> [label]

The kernel choice follows the process's ``NQA_WGRAD_EXACT_FP32`` (read once per process): run it once per build and setting
in separate processes and compare the lines that do not start with ``#``.  The case lists and their inputs come from this
checkout's ``tests/wgrad_cases.py`` (a function of the case names), the library and its Python host layer from ``<tree>``."""
import hashlib, os, sys
tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
sys.path.insert(0, tree)
import torch
import nequip_amd  # (before wgrad_cases, which puts its own checkout in front of sys.path)
from nequip_amd import _lib
from nequip_amd.utils import wgrad as _wg  # noqa: F401
assert os.path.dirname(os.path.abspath(nequip_amd.__file__)) == os.path.join(tree, "nequip_amd"), nequip_amd.__file__
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import wgrad_cases as wc
dev = torch.device("cuda:0")
exact_fp32 = os.environ.get("NQA_WGRAD_EXACT_FP32", "")
exact_fp32 = exact_fp32 != "" and exact_fp32[0] != "0"
lines = []
for case in wc.EXACT_CASES + wc.ACCURACY_CASES:
    a, b, types = wc.make_inputs(case)
    got, fails = wc.launch(case, a, b, types, dev)  # float64 [T, out_stride]; forced-S cases: the partials summed in float64
    assert not fails, fails
    S = case.S if case.S is not None else wc.library_splits(case.records, case.T, case.Z)
    h = hashlib.sha256(got.contiguous().numpy().tobytes()).hexdigest()
    lines.append(f"{case.name} T={case.T} Z={case.Z} S={S} {tuple(got.shape)} {h}")
open(out_path, "w").write(f"# {label}: NQA_WGRAD_EXACT_FP32={int(exact_fp32)} python scripts/wgrad_checksums.py <tree> <out> on "
                          f"{torch.cuda.get_device_name(0)}\n" + "\n".join(lines) + "\n")
print("wrote", len(lines), "checksums to", out_path, "from", _lib.LIB_PATH)
