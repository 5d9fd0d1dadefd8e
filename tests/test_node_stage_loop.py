"""The stage loop of the per-wavefront node kernels (csrc/node_ops.hip: node_linear_wave_bf16_unit, csrc/node_fused.h:
node_fused_unit) at the shapes where its pipeline can go wrong.

The loop keeps the next stage's x slab (and gate scalars) and the next two weight-fragment sets in flight while it multiplies
the current ones; the stage behind a unit's last one is the last one again.  So: units of exactly 1, 2, 3 and more stages
(prologue only, a loop that never reaches its steady state, the drain), a last K slab of 8 and of 16 channels next to full
ones, one and two column tiles, every irrep dimension, atom groups that are empty but for one row / one short of full / one
past full, with and without an addend, slabs that are not 16-byte aligned (element-wise loads), typed launches whose units
lack a type, hold one type only, or walk the atoms in an arbitrary order.

References: the oracle's float64 restatements of e3nn's Linear, FullyConnectedTensorProduct and Gate (oracle/nn.py); bounds:
those of tests/test_node_kernels.py (linear maps: 2e-5 untyped, 3e-5 typed, relative to the largest reference value) and of
tests/test_node_fused.py (fused stage: 2e-6 relative to max(1, largest reference value))."""
import pytest
import torch

from nequip_amd.o3 import _node_kernels as nk
from nequip_amd.o3.irreps import Irreps
from nequip_amd.o3.modules import FullyConnectedTensorProduct, Gate, Linear
from oracle import nn as onn

SILU = torch.nn.functional.silu

# (input irreps, output irreps): stages of a unit = 32-channel slabs of the input blocks of its irrep; column tiles = 32-column
# tiles of its output block
LINEAR = {
    # d = 1: 1 stage, 1 tile | d = 3: 2 stages, 2 tiles | d = 5: 3 stages (last slab 8), 1 tile | d = 7: 5 stages (last slab 16),
    # 2 tiles | d = 9: 2 stages (last slab 8), 1 tile
    "all_d": ("32x0e+64x1o+72x2e+144x3o+40x4e", "32x0e+64x1o+32x2e+64x3o+32x4e"),
    # d = 1: 5 stages (last slab 16), 2 tiles | d = 3: 1 stage, 1 tile | d = 5: 2 stages, 2 tiles
    "long_scalars": ("144x0e+32x1o+64x2e", "64x0e+32x1o+64x2e"),
    # d = 1: 3 stages (last slab 8) from one block + 1 stage (slab 16) from a second block | d = 3: 3 stages (last slab 8), 2 tiles
    # | d = 5: 1 stage (slab 16), 1 tile
    "two_blocks": ("72x0e+16x0e+72x1o+16x2e", "32x0e+64x1o+32x2e"),
    # nothing a multiple of 4: element-wise slab loads, masked stores; 1 stage per unit, partial tiles
    "unaligned": ("7x0e+13x1o+5x2e", "7x0e+13x1o+5x2e"),
}
ATOMS = [1, 31, 33, 37]  # d = 1 holds 32 atoms per group (d = 3: 10, d = 5: 6, d = 7: 4, d = 9: 3)


def _close(out, ref, tol, what):
    scale = float(ref.abs().max())
    err = float((out.double().cpu() - ref).abs().max())
    print(f"{what}: max error {err:.3e}, largest reference value {scale:.3e}, bound {tol * scale:.3e}")
    torch.testing.assert_close(out.double().cpu(), ref, atol=tol * scale, rtol=tol, msg=lambda m: f"{what}: {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("n_atoms", ATOMS)
@pytest.mark.parametrize("case", sorted(LINEAR))
def test_linear_map_forward_and_transposed(device, case, n_atoms):
    """Constant (packed) weights: forward with a scale and -- for every second atom count -- an addend, and the gradient
    w.r.t. the rows (the transposed map through the same kernel), against oracle.nn.o3_linear in float64."""
    ir_in, ir_out = LINEAR[case]
    g = torch.Generator().manual_seed(100 + n_atoms)
    lin = Linear(ir_in, ir_out).eval()
    x = torch.randn(n_atoms, lin.irreps_in.dim, generator=g, dtype=torch.float64)
    add = torch.randn(n_atoms, lin.irreps_out.dim, generator=g, dtype=torch.float64) if n_atoms in (1, 33) else None
    go = torch.randn(n_atoms, lin.irreps_out.dim, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    ref = onn.o3_linear(xr, lin.weight.detach().double(), str(lin.irreps_in), str(lin.irreps_out)) * 0.37
    if add is not None:
        ref = ref + add
    (gx_ref,) = torch.autograd.grad(ref, xr, go)

    lin = lin.to(device)
    wp = lin.eval_weights(device, torch.float32)
    assert not wp.requires_grad  # (the packed kernels; weights of a training step take the exact fp32 kernel)
    xd = x.float().to(device).requires_grad_(True)
    out = nk.node_linear(xd, wp, None, lin._meta, addend=None if add is None else add.float().to(device), scale=0.37)
    (gx,) = torch.autograd.grad(out, xd, go.float().to(device))
    _close(out.detach(), ref.detach(), 2e-5, f"{case} N={n_atoms} forward")
    _close(gx, gx_ref, 2e-5, f"{case} N={n_atoms} transposed")


TYPED = {
    "mixed": lambda n, g: torch.randint(0, 3, (n,), generator=g),             # every group holds what it holds
    "type_1_absent": lambda n, g: 2 * torch.randint(0, 2, (n,), generator=g),  # no unit holds type 1: its stages are skipped
    "one_type": lambda n, g: torch.full((n,), 2),                              # every unit runs one type's stages only
}


@pytest.mark.gpu
@pytest.mark.parametrize("order", ["by_type", "own", "permuted"])
@pytest.mark.parametrize("types_of", sorted(TYPED))
def test_typed_map_with_absent_types_and_atom_orders(device, monkeypatch, types_of, order):
    """Three weight sets, N = 37: d = 1 units of 3 x 3 stages (last slab 8, two tiles), d = 3 of 3 x 1, d = 5 of 3 x 2 (one tile)
    when no type is skipped; atom order grouped by type (default), the caller's own, and a fixed random permutation."""
    ir_in, ir_attr, ir_out = "72x0e+32x1o+48x2e", "8x0e", "64x0e+64x1o+32x2e"
    n_atoms, n_types = 37, 3
    g = torch.Generator().manual_seed(7)
    sc = FullyConnectedTensorProduct(ir_in, ir_attr, ir_out).eval()
    x = torch.randn(n_atoms, sc.irreps_in1.dim, generator=g, dtype=torch.float64)
    table = torch.randn(n_types, 8, generator=g, dtype=torch.float64)
    types = TYPED[types_of](n_atoms, g)
    go = torch.randn(n_atoms, sc.irreps_out.dim, generator=g, dtype=torch.float64)
    xr = x.clone().requires_grad_(True)
    ref = onn.fully_connected_tp(xr, table[types], sc.weight.detach().double(), ir_in, ir_attr, ir_out)
    (gx_ref,) = torch.autograd.grad(ref, xr, go)

    if order == "own":
        monkeypatch.setenv("NQA_NODE_TYPE_ORDER", "0")
    elif order == "permuted":
        perm = torch.randperm(n_atoms, generator=g).to(torch.int32).to(device)
        monkeypatch.setattr(nk, "type_order", lambda t: perm)
    sc = sc.to(device)
    wps = sc.eval_weights_typed(table.float().to(device), torch.float32)
    xd = x.float().to(device).requires_grad_(True)
    out = nk.node_linear(xd, wps, types.to(device), sc._meta)
    (gx,) = torch.autograd.grad(out, xd, go.float().to(device))
    _close(out.detach(), ref.detach(), 3e-5, f"typed {types_of} {order} forward")
    _close(gx, gx_ref, 3e-5, f"typed {types_of} {order} transposed")


def _layer(hidden):
    hid = Irreps(hidden)
    scalars = Irreps([(m, ir) for m, ir in hid if ir.l == 0])
    gated = Irreps([(m, ir) for m, ir in hid if ir.l > 0])
    gates = Irreps([(m, (0, 1)) for m, _ in gated])
    gate = Gate(scalars, [SILU for _ in scalars], gates, [SILU for _ in gates], gated)
    x_ir = gate.irreps_out
    return gate, Linear(x_ir, x_ir), FullyConnectedTensorProduct(x_ir, Irreps([(8, (0, 1))]), gate.irreps_in)


def _fused_reference(h, types, table, gate, lin1, sc, scale1):
    x = onn.gate(h, str(gate.irreps_scalars), ["silu" for _ in gate.act_scalars], str(gate.irreps_gates),
                 ["silu" for _ in gate.act_gates], str(gate.irreps_gated))
    y1 = onn.o3_linear(x, lin1.weight.detach().double(), str(lin1.irreps_in), str(lin1.irreps_out)) * scale1
    if sc is None:
        return y1, None
    return y1, onn.fully_connected_tp(x, table[types], sc.weight.detach().double(), str(sc.irreps_in1), str(sc.irreps_in2),
                                      str(sc.irreps_out))


# linear_1 units: ceil(mul / 32) stages; self-connection units: 3 types x ceil(mul / 32) stages of the types they hold
FUSED = [
    "32x0e+32x1o+32x2e",   # 1 stage, one tile (the scalar part of the self-connection: 96 columns, two chunks)
    "40x0e+72x1o+48x2e",   # 2 / 3 / 2 stages, last slabs of 8 / 8 / 16 channels, two tiles
]


@pytest.mark.gpu
@pytest.mark.parametrize("with_sc", [True, False])
@pytest.mark.parametrize("n_atoms", ATOMS)
@pytest.mark.parametrize("hidden", FUSED)
def test_fused_stage_forward_and_backward(device, hidden, n_atoms, with_sc):
    g = torch.Generator().manual_seed(11 * n_atoms + len(hidden))
    gate, lin1, sc = (m.eval() for m in _layer(hidden))
    gm = gate._kernel_meta
    n_types = 3
    table = torch.randn(n_types, 8, generator=g, dtype=torch.float64)
    types = torch.randint(0, n_types, (n_atoms,), generator=g)
    h = torch.randn(n_atoms, gm.din, generator=g, dtype=torch.float64)
    h[::7] *= 30.0  # rows far out in the activations' tails
    scale1 = 0.1617
    hr = h.clone().requires_grad_(True)
    r1, rs = _fused_reference(hr, types, table, gate, lin1, sc if with_sc else None, scale1)
    c1 = torch.randn(r1.shape, generator=g, dtype=torch.float64)
    cs = torch.randn(rs.shape, generator=g, dtype=torch.float64) if with_sc else None
    (g_ref,) = torch.autograd.grad((r1 * c1).sum() + ((rs * cs).sum() if with_sc else 0.0), hr)

    lin1, sc = lin1.to(device), sc.to(device)
    wp1 = lin1.eval_weights(device, torch.float32)
    hd = h.float().to(device).requires_grad_(True)
    if with_sc:
        wps = sc.eval_weights_typed(table.float().to(device), torch.float32)
        x1, s = nk.fused_node_stage(hd, types.to(device), gm, wp1, lin1._meta, scale1, wps, sc._meta)
        loss = (x1 * c1.float().to(device)).sum() + (s * cs.float().to(device)).sum()
    else:
        x1, s = nk.fused_node_stage(hd, None, gm, wp1, lin1._meta, scale1)
        assert s is None
        loss = (x1 * c1.float().to(device)).sum()
    (gh,) = torch.autograd.grad(loss, hd)

    def close(a, b, what):
        scale = float(b.abs().max())
        err = float((a.double().cpu() - b).abs().max())
        print(f"{hidden} N={n_atoms} sc={with_sc} {what}: max error {err:.3e}, bound {2e-6 * max(1.0, scale):.3e}")
        assert err <= 2e-6 * max(1.0, scale), f"{what}: {err:.3e} (scale {scale:.3e})"

    close(x1.detach(), r1.detach(), "linear_1(Gate(h)) * scale")
    if with_sc:
        close(s.detach(), rs.detach(), "sc(Gate(h))")
    close(gh, g_ref, "gradient w.r.t. the pre-gate rows")
