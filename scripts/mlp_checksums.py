"""sha256 of every output of the radial-MLP launchers (``nequip_amd/nn/mlp.py::_launch_*``) on fixed seeds, to compare two
builds bit for bit:

    python scripts/mlp_checksums.py <tree with a built nequip_amd> <out file> [label]

One line per output tensor: mode, shape (E, H, W), launcher, ``#0`` = first call (the prepass fills the weight image) /
``#1`` = second call on the cached image (``workspace_ready``), output index, tensor shape, sha256 of its bytes.  Run it
once per build in separate processes and compare the lines that do not start with ``#``."""
import hashlib, os, sys
tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
sys.path.insert(0, tree)
import torch
import nequip_amd
from nequip_amd import _lib
from nequip_amd.nn import mlp as M
assert os.path.dirname(os.path.abspath(nequip_amd.__file__)) == os.path.join(tree, "nequip_amd"), nequip_amd.__file__
dev = torch.device("cuda:0")
MODES = {"f16x3": {}, "bf16x6": {"NQA_MLP_FWD_F16": "0", "NQA_MLP_BWD_F16": "0"}, "fp32": {"NQA_MLP_EXACT_FP32": "1"}}
SHAPES = [(200279, 128, 704), (200279, 128, 192), (70001, 64, 192), (513, 128, 64)]
lines = []
def rec(tag, *ts):
    torch.cuda.synchronize()
    for i, t in enumerate(ts):
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        lines.append(f"{tag}[{i}] {tuple(t.shape)} {h}")
for mname, env in MODES.items():
    for k in ("NQA_MLP_FWD_F16", "NQA_MLP_BWD_F16", "NQA_MLP_EXACT_FP32"):
        os.environ.pop(k, None)
    os.environ.update(env)
    mode = M.radial_mlp_mode()
    for (E, H, W) in SHAPES:
        g = torch.Generator().manual_seed(1234 + E + H + W)
        r = lambda *s: torch.randn(*s, generator=g)
        emb, cot = (r(E, 8) * 0.5).to(dev), (r(E, 8) * 0.5).to(dev)
        w0, w1 = (r(8, H) * 1.7).to(dev), (r(H, W) * 1.7).to(dev)
        gw, gw2 = r(E, W).to(dev), r(E, W).to(dev)
        pre = r(E, H).to(dev)
        a0, a1 = 8 ** -0.5, (2.0 / H) ** 0.5
        tag = f"{mname} E={E} H={H} W={W} "
        for rep in range(2):  # second pass: the cached weight image (workspace_ready)
            c = M._WeightImages() if rep == 0 else c
            rec(tag + f"fwd#{rep}", M._launch_fwd(emb, w0, w1, a0, a1, mode, c))
            rec(tag + f"bwd#{rep}", M._launch_bwd(emb, w0, w1, a0, a1, gw, mode, c))
            if mname != "fp32":
                rec(tag + f"bwd_paired#{rep}", M._launch_bwd_paired(emb, w0, w1, a0, a1, gw, gw2, mode, c))
                rec(tag + f"bwd_train1#{rep}", *M._launch_bwd_train(emb, w0, w1, a0, a1, gw, None, mode, c))
                rec(tag + f"bwd_train2#{rep}", *M._launch_bwd_train(emb, w0, w1, a0, a1, gw, cot, mode, c))
                rec(tag + f"tangent#{rep}", M._launch_fwd_tangent(emb, cot, w0, w1, a0, a1, mode, c))
            if mname == "f16x3":
                cl = M._WeightImages() if rep == 0 else cl
                rec(tag + f"last_fwd#{rep}", M._launch_last(pre, w1, a1, cl))
                rec(tag + f"last_bwd#{rep}", M._launch_last(pre, w1, a1, cl, g=gw))
open(out_path, "w").write(f"# {label}: python scripts/mlp_checksums.py <tree> <out> on {torch.cuda.get_device_name(0)}\n" + "\n".join(lines) + "\n")
print("wrote", len(lines), "checksums to", out_path, "from", _lib.LIB_PATH)
