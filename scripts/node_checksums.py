"""sha256 of every output of the node launchers (``nequip_amd/o3/_node_kernels.py``: ``_launch_linear`` forward and transposed,
``_launch_gate`` modes 0-3, ``launch_fused`` forward and backward with an output gate) on fixed seeds, to compare two builds
bit for bit:

    python scripts/node_checksums.py <tree with a built nequip_amd> <out file> [label]

Modes: two-plane fp16 split, three-plane bf16 split, exact fp32, float64 (linear maps and gate; the fused stage exists in the
fp16 split only).  Every map runs untyped and typed with one atom type that no atom has.  Typed linear maps and all fused
launches run three times: in the caller's own atom order, grouped by type, and in a fixed random permutation -- the three
must give the same bits, and so must the two builds.  Shapes: the layer shapes of ``tests/test_node_fused.py`` (the last one
has more merged chunks than one fused launch holds) and the 43-chunk map of ``tests/test_node_kernels.py`` (more chunks than one
linear launch holds), and the stage-loop edge shapes of ``tests/test_node_stage_loop.py`` (units of 1 to 5 stages, partial K
slabs, one and two column tiles, d = 1 .. 9, 1 / 31 / 33 / 37 atoms, with an addend, unaligned slabs).  Run it once per build in separate processes and compare the lines that do not start with ``#``."""
import hashlib, os, sys
tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
sys.path.insert(0, tree)
import torch
import nequip_amd
from nequip_amd import _lib
from nequip_amd.o3 import _node_kernels as nk
from nequip_amd.o3.irreps import Irreps
from nequip_amd.o3.modules import FullyConnectedTensorProduct, Gate, Linear
assert os.path.dirname(os.path.abspath(nequip_amd.__file__)) == os.path.join(tree, "nequip_amd"), nequip_amd.__file__
dev = torch.device("cuda:0")
MODES = {"f16": {"NQA_NODE_F16": "1", "NQA_NODE_EXACT_FP32": "0"}, "bf16": {"NQA_NODE_F16": "0", "NQA_NODE_EXACT_FP32": "0"},
         "fp32": {"NQA_NODE_F16": "1", "NQA_NODE_EXACT_FP32": "1"}, "f64": {"NQA_NODE_F16": "1", "NQA_NODE_EXACT_FP32": "0"}}
LAYERS = [("64x0e+64x1o+64x2e", 2, 1003), ("32x0e+32x0o+32x1e+32x1o", 4, 105), ("128x0e+128x1o+128x2e+128x3o", 1, 257),
          ("64x0e+64x1o+64x2e+64x3o+64x4e", 5, 70), ("128x0e+128x1o+128x2e+128x3o+128x4e", 3, 70)]
SILU = torch.nn.functional.silu
lines = []
real_type_order = nk.type_order


def rec(tag, *ts):
    torch.cuda.synchronize()
    for i, t in enumerate(ts):
        h = hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()
        lines.append(f"{tag}[{i}] {tuple(t.shape)} {h}")


def layer(hidden):  # as tests/test_node_fused.py::_layer
    hid = Irreps(hidden)
    scalars = Irreps([(m, ir) for m, ir in hid if ir.l == 0])
    gated = Irreps([(m, ir) for m, ir in hid if ir.l > 0])
    gates = Irreps([(m, (0, 1)) for m, _ in gated])
    gate = Gate(scalars, [{1: SILU, -1: torch.tanh}[ir.p] for _, ir in scalars], gates, [SILU for _ in gates], gated)
    x_ir = gate.irreps_out
    return gate._kernel_meta, Linear(x_ir, x_ir)._meta, FullyConnectedTensorProduct(x_ir, Irreps([(8, (0, 1))]), gate.irreps_in)._meta


def orders(N, g):
    perm = torch.randperm(N, generator=g).to(torch.int32).to(dev)
    return (("own", None), ("by_type", "by_type"), ("perm", perm))


def linear(tag, meta, N, T, absent, g, dtype):
    """forward and transposed map; T > 1: types 0 .. T-1 without `absent`"""
    r = lambda *s: torch.randn(*s, generator=g)
    x, xt, wp = r(N, meta.din).to(dev, dtype), r(N, meta.dout).to(dev, dtype), r(T, meta.wstride).to(dev, dtype)
    types = None
    if T > 1:
        present = torch.tensor([t for t in range(T) if t != absent])
        types = present[torch.randint(0, len(present), (N,), generator=g)].to(dev)
    for oname, order in (orders(N, g) if T > 1 else (("own", None),)):
        os.environ["NQA_NODE_TYPE_ORDER"] = "0" if order is None else "1"
        nk.type_order = real_type_order if not torch.is_tensor(order) else (lambda types, order=order: order)
        rec(f"{tag} T={T} {oname} fwd", nk._launch_linear(x, wp, None, types, meta, "fwd", 0.37))
        rec(f"{tag} T={T} {oname} transposed",
            nk._launch_linear(xt, nk.meta_transposed_weights(meta, wp).contiguous(), None, types, nk._transposed(meta), "fwd", 0.37))
    nk.type_order = real_type_order
    os.environ.pop("NQA_NODE_TYPE_ORDER", None)


def fused(tag, gm, m1, ms, N, T, absent, g):
    r = lambda *s: torch.randn(*s, generator=g)
    h = r(N, gm.din)
    h[::7] *= 30.0
    h = h.to(dev)
    wp1, wps = r(1, m1.wstride).to(dev), r(T, ms.wstride).to(dev)
    g1, gs = r(N, m1.dout).to(dev), r(N, ms.dout).to(dev)
    types = None
    if T > 1:
        present = torch.tensor([t for t in range(T) if t != absent])
        types = present[torch.randint(0, len(present), (N,), generator=g)].to(dev)
    for oname, order in orders(N, g):
        if isinstance(order, str):
            if types is None:
                continue
            order = real_type_order(types)
        parts = [nk.FusedPart(h, wp1, m1, 0.1617, in_gate=gm), nk.FusedPart(h, wps, ms, 1.0, in_gate=gm)]
        rec(f"{tag} T={T} {oname} fused_fwd", *nk.launch_fused(parts, types, order=order))
        parts = [nk.FusedPart(g1, nk._scaled(nk.meta_transposed_weights(m1, wp1), 0.1617), nk._transposed(m1)),
                 nk.FusedPart(gs, nk.meta_transposed_weights(ms, wps), nk._transposed(ms), accumulate=True)]
        rec(f"{tag} T={T} {oname} fused_bwd", *nk.launch_fused(parts, types, out_gate=gm, gate_h=h, order=order))


for hidden, n_types, N in LAYERS:
    gm, m1, ms = layer(hidden)
    g = torch.Generator().manual_seed(4321 + N + gm.din)
    for dtype, dname in ((torch.float32, "f32"), (torch.float64, "f64")):
        r = lambda *s: torch.randn(*s, generator=g).to(dev, dtype)
        x, gout, cot = r(N, gm.din), r(N, gm.dout), r(N, gm.din)
        tag = f"gate {dname} {hidden} N={N} "
        rec(tag + "mode0", nk._launch_gate(x, None, gm, 0))
        rec(tag + "mode1", nk._launch_gate(x, gout, gm, 1))
        rec(tag + "mode2", nk._launch_gate(x, None, gm, 2, cot=cot))
        rec(tag + "mode3", nk._launch_gate(x, gout, gm, 3, cot=cot))
    for mname, env in MODES.items():
        os.environ.update(env)
        dtype = torch.float64 if mname == "f64" else torch.float32
        for lname, meta in (("linear_1", m1), ("sc", ms)):
            for T, absent in ((1, None), (n_types + 1, n_types // 2)):
                linear(f"{mname} {lname} {hidden} N={N}", meta, N, T, absent, g, dtype)
        if mname == "f16":
            for T, absent in ((1, None), (n_types + 1, n_types // 2)):
                fused(f"{mname} {hidden} N={N}", gm, m1, ms, N, T, absent, g)

# more chunks than one linear launch holds: 43 (tests/test_node_kernels.py)
meta = nk.NodeLinearMeta(Irreps("16x0e+8x0e+8x1o"), Irreps("+".join(["64x0e"] * 41 + ["70x1o"])),
                         [(0, b) for b in range(41)] + [(1, b) for b in range(10)] + [(2, 41)])
g = torch.Generator().manual_seed(43)
for mname, env in MODES.items():
    os.environ.update(env)
    for T, absent in ((1, None), (3, 2)):
        linear(f"{mname} 43chunks N=37", meta, 37, T, absent, g, torch.float64 if mname == "f64" else torch.float32)

# the shapes of tests/test_node_stage_loop.py: units of 1, 2, 3 and 5 stages, last K slabs of 8 and 16 channels, one and two
# column tiles, d = 1 .. 9, slabs that are not 16-byte aligned; atom groups with one row, one short of and one past a full
# d = 1 group; with an addend (forward, untyped); typed with three weight sets of which no atom has the middle one
EDGE_LINEAR = [("32x0e+64x1o+72x2e+144x3o+40x4e", "32x0e+64x1o+32x2e+64x3o+32x4e"), ("144x0e+32x1o+64x2e", "64x0e+32x1o+64x2e"),
               ("72x0e+16x0e+72x1o+16x2e", "32x0e+64x1o+32x2e"), ("7x0e+13x1o+5x2e", "7x0e+13x1o+5x2e")]
EDGE_FUSED = ["32x0e+32x1o+32x2e", "40x0e+72x1o+48x2e"]
EDGE_ATOMS = (1, 31, 33, 37)
g = torch.Generator().manual_seed(97)
for mname in ("f16", "bf16"):
    os.environ.update(MODES[mname])
    for ir_in, ir_out in EDGE_LINEAR:
        meta = Linear(Irreps(ir_in), Irreps(ir_out))._meta
        for N in EDGE_ATOMS:
            tag = f"{mname} edge {ir_in}->{ir_out} N={N}"
            for T, absent in ((1, None), (3, 1)):
                linear(tag, meta, N, T, absent, g, torch.float32)
            x, wp, add = (torch.randn(*s, generator=g).to(dev) for s in ((N, meta.din), (1, meta.wstride), (N, meta.dout)))
            rec(tag + " addend fwd", nk._launch_linear(x, wp, add, None, meta, "fwd", 0.37))
os.environ.update(MODES["f16"])
for hidden in EDGE_FUSED:
    gm, m1, ms = layer(hidden)
    for N in EDGE_ATOMS:
        for T, absent in ((1, None), (3, 1)):
            fused(f"f16 edge {hidden} N={N}", gm, m1, ms, N, T, absent, g)

open(out_path, "w").write(f"# {label}: python scripts/node_checksums.py <tree> <out> on {torch.cuda.get_device_name(0)}\n" + "\n".join(lines) + "\n")
print("wrote", len(lines), "checksums to", out_path, "from", _lib.LIB_PATH)
