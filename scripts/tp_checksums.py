"""sha256 of every output of every tensor-product launcher (``nequip_amd/nn/_tp_scatter_base.py::_Kernels``) on fixed
seeds, to compare two builds bit for bit:

    python scripts/tp_checksums.py <tree with a built nequip_amd> <out file> [label] [default-form tensors .pt]
    python scripts/tp_checksums.py --compare <parent .pt> <child .pt>

One line per output tensor: structure, ``NQA_SPEC_WPN``, per-edge (``edge``) or paired (``pair``) weights, method, output
index, tensor shape, sha256 of its bytes.  The pair-centric backward is run in its two forms that add in a fixed order:
``ring_rows`` (LDS-ring kernel, grad_x rows) and ``registers`` (register kernel, grad_x rows).  Run the script once per
build in separate processes; every line that does not start with ``#`` must be equal in the two files.

The default form adds into its accumulators in arrival order and is not reproducible to the bit.  For it a ``#`` line per
structure gives the largest difference of one run from the ``registers`` result and between two runs of this build, and the
first run's tensors go to the ``.pt`` file; ``--compare`` then prints, per structure, the largest difference between the
two builds next to the first build's own run-to-run difference."""
import hashlib, os, sys
import torch
if sys.argv[1] == "--compare":
    pa, ch = torch.load(sys.argv[2]), torch.load(sys.argv[3])
    for name in pa:
        d = max(float((s - t).abs().max()) for s, t in zip(pa[name]["first"], ch[name]["first"]))
        print(f"{name} bwd_pairs default form: max|d| between the builds {d:.3e}, between two runs of the first build "
              f"{pa[name]['run_to_run']:.3e}, of the second {ch[name]['run_to_run']:.3e} (max|gx| {pa[name]['max_gx']:.3e})")
    sys.exit(0)
tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
pt_path = sys.argv[4] if len(sys.argv) > 4 else None
sys.path.insert(0, tree)
import nequip_amd
from nequip_amd import _lib
from nequip_amd.nn import TensorProductScatter
from nequip_amd.nn._topology import EdgeTopology
from nequip_amd.o3 import Irreps
from nequip_amd.utils import synthetic as syn
from oracle import tp as otp, irreps as oir
assert os.path.dirname(os.path.abspath(nequip_amd.__file__)) == os.path.join(tree, "nequip_amd"), nequip_amd.__file__
dev = torch.device("cuda:0")
# the three cfg-3 layer shapes of scripts/bench_tp.py and one l_max = 3 structure whose pair kernel is split by input block
SHAPES = [("mid", "64x0e+64x1o+64x2e", 2, "192x0e+64x1o+64x2e"), ("first", "64x0e", 2, "64x0e+64x1o+64x2e"),
          ("last", "64x0e+64x1o+64x2e", 2, "64x0e"), ("l3_mid", "64x0e+64x1o+64x2e+64x3o", 3, "64x0e+64x1o+64x2e+64x3o")]
FORMS = {"ring_rows": {"NQA_PAIR_RING": "1", "NQA_PAIR_GX_ATOMIC": "0"},
         "registers": {"NQA_PAIR_RING": "0", "NQA_PAIR_GX_ATOMIC": "0"}}
pos, types, cell, names = syn.water_box(9, seed=0)
data = syn.make_data(pos, types, 4.5, cell)
ei = data["edge_index"].to(dev)
N, E = len(pos), ei.shape[1]
lines, default_form = [], {}
def rec(tag, *ts):
    torch.cuda.synchronize()
    for i, t in enumerate(ts):
        if t is not None:
            h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
            lines.append(f"{tag}[{i}] {tuple(t.shape)} {h}")
def maxdiff(a, b):
    return max(float((s - t).abs().max()) for s, t in zip(a, b))
for name, f_in, lmax, f_out in SHAPES:
    e_at = Irreps.spherical_harmonics(lmax)
    mid, instr = otp.build_instructions(f_in, str(e_at), f_out)
    tps = TensorProductScatter(Irreps(f_in), e_at, Irreps(oir.to_str(mid)), instr).to(dev)
    k, topo = tps._get_kernels(), EdgeTopology(ei[0], ei[1], N)
    pr = topo.pairing(data["edge_cell_shift"].to(dev))
    assert k.has_spec(torch.float32) and pr is not None
    g_ = torch.Generator().manual_seed(4321 + k.weight_numel)
    r = lambda *s: torch.randn(*s, generator=g_).to(dev)
    x, y, g, cx, cy = r(N, k.dim_in1), r(E, k.dim_in2), r(N, k.dim_out), r(N, k.dim_in1), r(E, k.dim_in2)
    ws = {"edge": (r(E, k.weight_numel), r(E, k.weight_numel), None), "pair": (r(pr.num_pairs, k.weight_numel), r(pr.num_pairs, k.weight_numel), pr)}
    for wpn in ("1", "4"):
        os.environ["NQA_SPEC_WPN"] = wpn
        for kind, (w, cw, p) in ws.items():
            tag = f"{name} wpn={wpn} {kind} "
            rec(tag + "fwd", k.fwd(x, y, w, topo, p))
            rec(tag + "bwd_x", k.bwd_x(y, w, g, topo, p))
            rec(tag + "bwd_edge", *k.bwd_edge(x, y, w, g, topo, True, True, p))
            rec(tag + "bwd_edge_gw", *k.bwd_edge(x, y, w, g, topo, True, False, p))
            rec(tag + "bwd_edge_gy", *k.bwd_edge(x, y, w, g, topo, False, True, p))
            if k.fused_rows_ok:
                rec(tag + "bwd_fused", *k.bwd_fused(x, y, w, g, topo, True, True, p))
            rec(tag + "fwd_jvp", k.fwd_jvp(x, y, w, cx, cy, cw, topo, p))
            rec(tag + "bwd_x_dual", k.bwd_x_dual(y, w, cy, cw, g, topo, p))
        w, cw, _ = ws["pair"]
        tag = f"{name} wpn={wpn} pair "
        if k.has_dual_pairs_kernel(torch.float32):
            rec(tag + "edge_grads_dual", *k.edge_grads_dual(x, cx, y, cy, w, g, topo, pr, w_cot=cw))
        if k.has_pairs_kernel(torch.float32):
            for form, env in FORMS.items():
                os.environ.update(env)
                rows = k.bwd_pairs(x, y, w, g, topo, pr)
                rec(tag + f"bwd_pairs {form}", *rows)
                rec(tag + f"bwd_pairs {form} no_gx", *k.bwd_pairs(x, y, w, g, topo, pr, need_gx=False))
            for key in ("NQA_PAIR_RING", "NQA_PAIR_GX_ATOMIC"):
                os.environ.pop(key)
    os.environ.pop("NQA_SPEC_WPN")  # the default form, at the launch shape the library picks itself
    if k.has_pairs_kernel(torch.float32):
        w = ws["pair"][0]
        a, b = k.bwd_pairs(x, y, w, g, topo, pr), k.bwd_pairs(x, y, w, g, topo, pr)
        torch.cuda.synchronize()
        default_form[name] = {"first": [t.cpu() for t in a], "run_to_run": maxdiff(a, b), "max_gx": float(a[0].abs().max())}
        lines.append(f"# {name} bwd_pairs default form: max|d| from registers {maxdiff(a, rows):.3e}, between two runs "
                     f"{maxdiff(a, b):.3e} (max|gx| {float(a[0].abs().max()):.3e})")
if pt_path:
    torch.save(default_form, pt_path)
open(out_path, "w").write(f"# {label}: python scripts/tp_checksums.py <tree> <out> on {torch.cuda.get_device_name(0)}, N={N} E={E}\n"
                          + "\n".join(lines) + "\n")
print("wrote", len(lines), "lines to", out_path, "from", _lib.LIB_PATH)
