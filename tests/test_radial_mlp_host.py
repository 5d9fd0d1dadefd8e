"""Host side of the fused radial MLP (``nequip_amd/csrc/radial_mlp.hip``), no GPU: the workspace size of every (mode,
direction, H, W) and the calls that are refused before anything touches the device.

The literals were printed by the library as it was before the host code was folded into one layout function and one
driver per direction; they pin the workspace layout and, for every launch entry point, the order of the argument checks,
the return codes and the ``nqa_last_error()`` texts of the C ABI."""

import ctypes

MODES, HS, WS = (0, 1, 2, 3), (0, 64, 128), (0, 4, 31, 32, 33, 192, 704, 2944)
F32, FP32, BF16X6, F16X3, IDLE = 0, 0, 1, 2, 0x100
BIG = 1 << 40

# argument names of the launch entry points, in the order of include/nequip_amd.h
TWO = ("emb", "w0", "alpha0", "w1", "alpha1")
DIMS = ("nb", "H", "W", "E")
TAIL = ("ws", "ws_bytes", "ready", "stream")
ENTRY = {
    "fwd": ("dtype", "mode") + TWO + DIMS + ("out",) + TAIL,
    "fwd_tangent": ("dtype", "mode", "emb", "cot") + TWO[1:] + DIMS + ("out",) + TAIL,
    "bwd": ("dtype", "mode") + TWO + ("g",) + DIMS + ("out",) + TAIL,
    "bwd_paired": ("dtype", "mode") + TWO + ("g", "g2") + DIMS + ("out",) + TAIL,
    "bwd_train": ("dtype", "mode", "emb", "cot") + TWO[1:] + ("g",) + DIMS + ("out", "hid", "parts") + TAIL,
    "last_fwd": ("dtype", "mode", "emb", "w1", "alpha1", "H", "W", "E", "out") + TAIL,
    "last_bwd": ("dtype", "mode", "emb", "w1", "alpha1", "g", "g2", "H", "W", "E", "out") + TAIL,
}
SCALARS = dict(dtype=F32, alpha0=0.5, alpha1=0.25, nb=8, H=128, W=192, E=1000, ws_bytes=BIG, ready=0, stream=None)


def _call(lib, entry, p, **over):
    """One call of ``nqa_radial_mlp_<entry>``: valid arguments (every pointer = the host buffer ``p`` that nothing reads, a
    workspace declared large enough) with ``over`` on top."""
    vals = dict(SCALARS, mode=F16X3 if entry.startswith("last") else BF16X6)
    vals.update(over)
    return getattr(lib, "nqa_radial_mlp_" + entry)(*[vals.get(name, p) for name in ENTRY[entry]])


def _refusals(lib):
    """``(name, call)``: calls that return before the first device call: every one breaks a precondition that is checked
    ahead of the launch.  Left out: ``nqa_radial_mlp_fwd`` in ``NQA_MLP_FP32`` mode with a workspace that is too small --
    that mode needs none, so the call is valid and launches."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    for entry in ENTRY:
        last = entry.startswith("last")
        cases = [("wrong dtype", dict(dtype=1)), ("unknown mode", dict(mode=7)), ("H = 96", dict(H=96)),
                 ("W = 6", dict(W=6)), ("W = 0", dict(W=0)), ("E = -1", dict(E=-1)), ("null input", dict(emb=None)),
                 ("null weights", dict(w1=None)), ("null output", dict(out=None)), ("null workspace", dict(ws=None)),
                 ("one-byte workspace", dict(ws_bytes=1)), ("H = 96 and W = 6", dict(H=96, W=6))]
        if not last:
            cases += [("nb = 9", dict(nb=9)), ("nb = 0", dict(nb=0)), ("null w0", dict(w0=None)),
                      ("f16x3 mode, one-byte workspace", dict(mode=F16X3, ws_bytes=1))]
            if entry != "fwd":  # (the exact-fp32 forward has no workspace: that call would be launched)
                cases += [("fp32 mode, one-byte workspace", dict(mode=FP32, ws_bytes=1))]
        else:
            cases += [("bf16x6 mode", dict(mode=BF16X6)), ("fp32 mode", dict(mode=FP32))]
        if "g" in ENTRY[entry]:
            cases += [("null gradient", dict(g=None)), ("idle hint, one-byte workspace", dict(mode=F16X3 | IDLE, ws_bytes=1)),
                      ("idle hint alone", dict(mode=IDLE, ws_bytes=1))]
        if entry == "fwd_tangent":
            cases += [("null cotangent", dict(cot=None)), ("f16x3 mode", dict(mode=F16X3)), ("fp32 mode", dict(mode=FP32)),
                      ("null cotangent and wrong dtype", dict(cot=None, dtype=1))]
        if entry == "bwd_paired":
            cases += [("null second stream", dict(g2=None)), ("fp32 mode", dict(mode=FP32)),
                      ("null second stream and H = 96", dict(g2=None, H=96))]
        if entry == "bwd_train":
            cases += [("null hidden_out", dict(hid=None)), ("null w0_partials", dict(parts=None)),
                      ("fp32 mode", dict(mode=FP32)), ("fp32 mode, second order off", dict(mode=FP32, cot=None)),
                      ("null hidden_out and unknown mode", dict(hid=None, mode=7))]
        for what, over in cases:
            yield f"{entry}: {what}", (lambda entry=entry, over=over: _call(lib, entry, p, **over))


def _empty(lib):
    """``(name, call)``: launches over zero rows, with null pointers throughout."""
    for entry in ENTRY:
        null = {name: None for name in ENTRY[entry] if name not in SCALARS and name != "mode"}
        yield entry, (lambda entry=entry, null=null: _call(lib, entry, None, E=0, ws_bytes=0, **null))


WORKSPACE = {(0, 0, 0, 0): -1,
 (0, 0, 0, 4): -1,
 (0, 0, 0, 31): -1,
 (0, 0, 0, 32): -1,
 (0, 0, 0, 33): -1,
 (0, 0, 0, 192): -1,
 (0, 0, 0, 704): -1,
 (0, 0, 0, 2944): -1,
 (0, 0, 64, 0): -1,
 (0, 0, 64, 4): 0,
 (0, 0, 64, 31): 0,
 (0, 0, 64, 32): 0,
 (0, 0, 64, 33): 0,
 (0, 0, 64, 192): 0,
 (0, 0, 64, 704): 0,
 (0, 0, 64, 2944): 0,
 (0, 0, 128, 0): -1,
 (0, 0, 128, 4): 0,
 (0, 0, 128, 31): 0,
 (0, 0, 128, 32): 0,
 (0, 0, 128, 33): 0,
 (0, 0, 128, 192): 0,
 (0, 0, 128, 704): 0,
 (0, 0, 128, 2944): 0,
 (0, 1, 0, 0): -1,
 (0, 1, 0, 4): -1,
 (0, 1, 0, 31): -1,
 (0, 1, 0, 32): -1,
 (0, 1, 0, 33): -1,
 (0, 1, 0, 192): -1,
 (0, 1, 0, 704): -1,
 (0, 1, 0, 2944): -1,
 (0, 1, 64, 0): -1,
 (0, 1, 64, 4): 66560,
 (0, 1, 64, 31): 73472,
 (0, 1, 64, 32): 73728,
 (0, 1, 64, 33): 73984,
 (0, 1, 64, 192): 114688,
 (0, 1, 64, 704): 245760,
 (0, 1, 64, 2944): 819200,
 (0, 1, 128, 0): -1,
 (0, 1, 128, 4): 133120,
 (0, 1, 128, 31): 146944,
 (0, 1, 128, 32): 147456,
 (0, 1, 128, 33): 147968,
 (0, 1, 128, 192): 229376,
 (0, 1, 128, 704): 491520,
 (0, 1, 128, 2944): 1638400,
 (1, 0, 0, 0): -1,
 (1, 0, 0, 4): -1,
 (1, 0, 0, 31): -1,
 (1, 0, 0, 32): -1,
 (1, 0, 0, 33): -1,
 (1, 0, 0, 192): -1,
 (1, 0, 0, 704): -1,
 (1, 0, 0, 2944): -1,
 (1, 0, 64, 0): -1,
 (1, 0, 64, 4): 12288,
 (1, 0, 64, 31): 12288,
 (1, 0, 64, 32): 12288,
 (1, 0, 64, 33): 24576,
 (1, 0, 64, 192): 73728,
 (1, 0, 64, 704): 270336,
 (1, 0, 64, 2944): 1130496,
 (1, 0, 128, 0): -1,
 (1, 0, 128, 4): 24576,
 (1, 0, 128, 31): 24576,
 (1, 0, 128, 32): 24576,
 (1, 0, 128, 33): 49152,
 (1, 0, 128, 192): 147456,
 (1, 0, 128, 704): 540672,
 (1, 0, 128, 2944): 2260992,
 (1, 1, 0, 0): -1,
 (1, 1, 0, 4): -1,
 (1, 1, 0, 31): -1,
 (1, 1, 0, 32): -1,
 (1, 1, 0, 33): -1,
 (1, 1, 0, 192): -1,
 (1, 1, 0, 704): -1,
 (1, 1, 0, 2944): -1,
 (1, 1, 64, 0): -1,
 (1, 1, 64, 4): 12288,
 (1, 1, 64, 31): 12288,
 (1, 1, 64, 32): 12288,
 (1, 1, 64, 33): 24576,
 (1, 1, 64, 192): 73728,
 (1, 1, 64, 704): 270336,
 (1, 1, 64, 2944): 1130496,
 (1, 1, 128, 0): -1,
 (1, 1, 128, 4): 24576,
 (1, 1, 128, 31): 24576,
 (1, 1, 128, 32): 24576,
 (1, 1, 128, 33): 49152,
 (1, 1, 128, 192): 147456,
 (1, 1, 128, 704): 540672,
 (1, 1, 128, 2944): 2260992,
 (2, 0, 0, 0): -1,
 (2, 0, 0, 4): -1,
 (2, 0, 0, 31): -1,
 (2, 0, 0, 32): -1,
 (2, 0, 0, 33): -1,
 (2, 0, 0, 192): -1,
 (2, 0, 0, 704): -1,
 (2, 0, 0, 2944): -1,
 (2, 0, 64, 0): -1,
 (2, 0, 64, 4): 8448,
 (2, 0, 64, 31): 8448,
 (2, 0, 64, 32): 8448,
 (2, 0, 64, 33): 16640,
 (2, 0, 64, 192): 49408,
 (2, 0, 64, 704): 180480,
 (2, 0, 64, 2944): 754176,
 (2, 0, 128, 0): -1,
 (2, 0, 128, 4): 16640,
 (2, 0, 128, 31): 16640,
 (2, 0, 128, 32): 16640,
 (2, 0, 128, 33): 33024,
 (2, 0, 128, 192): 98560,
 (2, 0, 128, 704): 360704,
 (2, 0, 128, 2944): 1507840,
 (2, 1, 0, 0): -1,
 (2, 1, 0, 4): -1,
 (2, 1, 0, 31): -1,
 (2, 1, 0, 32): -1,
 (2, 1, 0, 33): -1,
 (2, 1, 0, 192): -1,
 (2, 1, 0, 704): -1,
 (2, 1, 0, 2944): -1,
 (2, 1, 64, 0): -1,
 (2, 1, 64, 4): 8448,
 (2, 1, 64, 31): 8448,
 (2, 1, 64, 32): 8448,
 (2, 1, 64, 33): 16640,
 (2, 1, 64, 192): 49408,
 (2, 1, 64, 704): 180480,
 (2, 1, 64, 2944): 754176,
 (2, 1, 128, 0): -1,
 (2, 1, 128, 4): 16640,
 (2, 1, 128, 31): 16640,
 (2, 1, 128, 32): 16640,
 (2, 1, 128, 33): 33024,
 (2, 1, 128, 192): 98560,
 (2, 1, 128, 704): 360704,
 (2, 1, 128, 2944): 1507840,
 (3, 0, 0, 0): -1,
 (3, 0, 0, 4): -1,
 (3, 0, 0, 31): -1,
 (3, 0, 0, 32): -1,
 (3, 0, 0, 33): -1,
 (3, 0, 0, 192): -1,
 (3, 0, 0, 704): -1,
 (3, 0, 0, 2944): -1,
 (3, 0, 64, 0): -1,
 (3, 0, 64, 4): -1,
 (3, 0, 64, 31): -1,
 (3, 0, 64, 32): -1,
 (3, 0, 64, 33): -1,
 (3, 0, 64, 192): -1,
 (3, 0, 64, 704): -1,
 (3, 0, 64, 2944): -1,
 (3, 0, 128, 0): -1,
 (3, 0, 128, 4): -1,
 (3, 0, 128, 31): -1,
 (3, 0, 128, 32): -1,
 (3, 0, 128, 33): -1,
 (3, 0, 128, 192): -1,
 (3, 0, 128, 704): -1,
 (3, 0, 128, 2944): -1,
 (3, 1, 0, 0): -1,
 (3, 1, 0, 4): -1,
 (3, 1, 0, 31): -1,
 (3, 1, 0, 32): -1,
 (3, 1, 0, 33): -1,
 (3, 1, 0, 192): -1,
 (3, 1, 0, 704): -1,
 (3, 1, 0, 2944): -1,
 (3, 1, 64, 0): -1,
 (3, 1, 64, 4): -1,
 (3, 1, 64, 31): -1,
 (3, 1, 64, 32): -1,
 (3, 1, 64, 33): -1,
 (3, 1, 64, 192): -1,
 (3, 1, 64, 704): -1,
 (3, 1, 64, 2944): -1,
 (3, 1, 128, 0): -1,
 (3, 1, 128, 4): -1,
 (3, 1, 128, 31): -1,
 (3, 1, 128, 32): -1,
 (3, 1, 128, 33): -1,
 (3, 1, 128, 192): -1,
 (3, 1, 128, 704): -1,
 (3, 1, 128, 2944): -1}
REFUSED = {'bwd: E = -1': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: H = 96': (-2, 'nqa_radial_mlp_bwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'bwd: H = 96 and W = 6': (-2, 'nqa_radial_mlp_bwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'bwd: W = 0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: W = 6': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd: f16x3 mode, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd: fp32 mode, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd: idle hint alone': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd: idle hint, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd: nb = 0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: nb = 9': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: null gradient': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd: null input': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: null output': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd: null w0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: null weights': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd: null workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd: one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd: unknown mode': (-1, 'nqa_radial_mlp_bwd: unknown mode'),
 'bwd: wrong dtype': (-2, 'nqa_radial_mlp_bwd: only float32 is implemented on MFMA'),
 'bwd_paired: E = -1': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: H = 96': (-2, 'nqa_radial_mlp_bwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'bwd_paired: H = 96 and W = 6': (-2, 'nqa_radial_mlp_bwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'bwd_paired: W = 0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: W = 6': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd_paired: f16x3 mode, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_paired: fp32 mode': (-2, 'nqa_radial_mlp_bwd_train / _paired: NQA_MLP_BF16X6 or NQA_MLP_F16X3 (no exact-fp32 form)'),
 'bwd_paired: fp32 mode, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_paired: idle hint alone': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_paired: idle hint, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_paired: nb = 0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: nb = 9': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: null gradient': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd_paired: null input': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: null output': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd_paired: null second stream': (-1, 'nqa_radial_mlp_bwd_paired: second gradient stream is required'),
 'bwd_paired: null second stream and H = 96': (-1, 'nqa_radial_mlp_bwd_paired: second gradient stream is required'),
 'bwd_paired: null w0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: null weights': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_paired: null workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_paired: one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_paired: unknown mode': (-1, 'nqa_radial_mlp_bwd: unknown mode'),
 'bwd_paired: wrong dtype': (-2, 'nqa_radial_mlp_bwd: only float32 is implemented on MFMA'),
 'bwd_train: E = -1': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: H = 96': (-2, 'nqa_radial_mlp_bwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'bwd_train: H = 96 and W = 6': (-2, 'nqa_radial_mlp_bwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'bwd_train: W = 0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: W = 6': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd_train: f16x3 mode, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_train: fp32 mode': (-2, 'nqa_radial_mlp_bwd_train / _paired: NQA_MLP_BF16X6 or NQA_MLP_F16X3 (no exact-fp32 form)'),
 'bwd_train: fp32 mode, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_train: fp32 mode, second order off': (-2,
                                            'nqa_radial_mlp_bwd_train / _paired: NQA_MLP_BF16X6 or NQA_MLP_F16X3 (no exact-fp32 form)'),
 'bwd_train: idle hint alone': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_train: idle hint, one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_train: nb = 0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: nb = 9': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: null gradient': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd_train: null hidden_out': (-1, 'nqa_radial_mlp_bwd_train: hidden_out and w0_partials are required'),
 'bwd_train: null hidden_out and unknown mode': (-1,
                                                 'nqa_radial_mlp_bwd_train: hidden_out and w0_partials are required'),
 'bwd_train: null input': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: null output': (-1, 'nqa_radial_mlp_bwd: invalid argument (needs out_features % 4 == 0)'),
 'bwd_train: null w0': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: null w0_partials': (-1, 'nqa_radial_mlp_bwd_train: hidden_out and w0_partials are required'),
 'bwd_train: null weights': (-1, 'nqa_radial_mlp_bwd: invalid argument'),
 'bwd_train: null workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_train: one-byte workspace': (-4, 'nqa_radial_mlp_bwd: workspace missing or too small'),
 'bwd_train: unknown mode': (-1, 'nqa_radial_mlp_bwd: unknown mode'),
 'bwd_train: wrong dtype': (-2, 'nqa_radial_mlp_bwd: only float32 is implemented on MFMA'),
 'fwd: E = -1': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: H = 96': (-2, 'nqa_radial_mlp_fwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'fwd: H = 96 and W = 6': (-2, 'nqa_radial_mlp_fwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'fwd: W = 0': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: W = 6': (-1, 'nqa_radial_mlp_fwd: invalid output (needs out_features % 4 == 0)'),
 'fwd: f16x3 mode, one-byte workspace': (-4, 'nqa_radial_mlp_fwd: workspace missing or too small'),
 'fwd: nb = 0': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: nb = 9': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: null input': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: null output': (-1, 'nqa_radial_mlp_fwd: invalid output (needs out_features % 4 == 0)'),
 'fwd: null w0': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: null weights': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd: null workspace': (-4, 'nqa_radial_mlp_fwd: workspace missing or too small'),
 'fwd: one-byte workspace': (-4, 'nqa_radial_mlp_fwd: workspace missing or too small'),
 'fwd: unknown mode': (-1, 'nqa_radial_mlp_fwd: unknown mode'),
 'fwd: wrong dtype': (-2, 'nqa_radial_mlp_fwd: only float32 is implemented on MFMA'),
 'fwd_tangent: E = -1': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: H = 96': (-2, 'nqa_radial_mlp_fwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'fwd_tangent: H = 96 and W = 6': (-2,
                                   'nqa_radial_mlp_fwd: hidden width must be 64 or 128 for the fused MFMA kernel'),
 'fwd_tangent: W = 0': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: W = 6': (-1, 'nqa_radial_mlp_fwd: invalid output (needs out_features % 4 == 0)'),
 'fwd_tangent: f16x3 mode': (-2,
                             'nqa_radial_mlp_fwd_tangent: NQA_MLP_F16X3 is a mode of the plain forward (use '
                             'NQA_MLP_BF16X6)'),
 'fwd_tangent: f16x3 mode, one-byte workspace': (-4, 'nqa_radial_mlp_fwd: workspace missing or too small'),
 'fwd_tangent: fp32 mode': (-2, 'nqa_radial_mlp_fwd_tangent: only NQA_MLP_BF16X6 is implemented'),
 'fwd_tangent: fp32 mode, one-byte workspace': (-2, 'nqa_radial_mlp_fwd_tangent: only NQA_MLP_BF16X6 is implemented'),
 'fwd_tangent: nb = 0': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: nb = 9': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: null cotangent': (-1, 'nqa_radial_mlp_fwd_tangent: cotangent is required'),
 'fwd_tangent: null cotangent and wrong dtype': (-1, 'nqa_radial_mlp_fwd_tangent: cotangent is required'),
 'fwd_tangent: null input': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: null output': (-1, 'nqa_radial_mlp_fwd: invalid output (needs out_features % 4 == 0)'),
 'fwd_tangent: null w0': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: null weights': (-1, 'nqa_radial_mlp_fwd: invalid argument'),
 'fwd_tangent: null workspace': (-4, 'nqa_radial_mlp_fwd: workspace missing or too small'),
 'fwd_tangent: one-byte workspace': (-4, 'nqa_radial_mlp_fwd: workspace missing or too small'),
 'fwd_tangent: unknown mode': (-1, 'nqa_radial_mlp_fwd: unknown mode'),
 'fwd_tangent: wrong dtype': (-2, 'nqa_radial_mlp_fwd: only float32 is implemented on MFMA'),
 'last_bwd: E = -1': (-1, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: H = 96': (-2, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: H = 96 and W = 6': (-2,
                                'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: W = 0': (-1, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: W = 6': (-1, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: bf16x6 mode': (-2, 'nqa_radial_mlp_last_bwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_bwd: fp32 mode': (-2, 'nqa_radial_mlp_last_bwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_bwd: idle hint alone': (-2,
                               'nqa_radial_mlp_last_bwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_bwd: idle hint, one-byte workspace': (-2,
                                             'nqa_radial_mlp_last_bwd: float32 on the two-plane fp16 split '
                                             '(NQA_MLP_F16X3) only'),
 'last_bwd: null gradient': (-1,
                             'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: null input': (-1, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: null output': (-1, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: null weights': (-1, 'nqa_radial_mlp_last_bwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_bwd: null workspace': (-4, 'nqa_radial_mlp_last_bwd: workspace missing or too small'),
 'last_bwd: one-byte workspace': (-4, 'nqa_radial_mlp_last_bwd: workspace missing or too small'),
 'last_bwd: unknown mode': (-2, 'nqa_radial_mlp_last_bwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_bwd: wrong dtype': (-2, 'nqa_radial_mlp_last_bwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_fwd: E = -1': (-1, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: H = 96': (-2, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: H = 96 and W = 6': (-2,
                                'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: W = 0': (-1, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: W = 6': (-1, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: bf16x6 mode': (-2, 'nqa_radial_mlp_last_fwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_fwd: fp32 mode': (-2, 'nqa_radial_mlp_last_fwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_fwd: null input': (-1, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: null output': (-1, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: null weights': (-1, 'nqa_radial_mlp_last_fwd: invalid argument (hidden 64 / 128, out_features % 4 == 0)'),
 'last_fwd: null workspace': (-4, 'nqa_radial_mlp_last_fwd: workspace missing or too small'),
 'last_fwd: one-byte workspace': (-4, 'nqa_radial_mlp_last_fwd: workspace missing or too small'),
 'last_fwd: unknown mode': (-2, 'nqa_radial_mlp_last_fwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only'),
 'last_fwd: wrong dtype': (-2, 'nqa_radial_mlp_last_fwd: float32 on the two-plane fp16 split (NQA_MLP_F16X3) only')}


def test_workspace_bytes_of_every_form():
    from nequip_amd import _lib

    lib = _lib.load()
    assert set(WORKSPACE) == {(m, b, h, w) for m in MODES for b in (0, 1) for h in HS for w in WS}
    for (m, b, h, w), want in WORKSPACE.items():
        assert lib.nqa_radial_mlp_workspace_bytes(m, b, h, w) == want, (m, b, h, w)
    # the fp16 split keeps its scales / exponents behind the fragments, in whole 256-byte units
    for b in (0, 1):
        for w in (4, 704, 2944):
            assert WORKSPACE[(F16X3, b, 128, w)] % 256 == 0 and WORKSPACE[(F16X3, b, 128, w)] > 0
    assert all(v == -1 for (m, b, h, w), v in WORKSPACE.items() if m == 3 or h == 0 or w == 0)


def test_calls_refused_before_the_device_is_touched():
    from nequip_amd import _lib

    lib = _lib.load()
    seen = []
    for name, call in _refusals(lib):
        rc = call()
        assert rc in (-1, -2, -4) and (rc, lib.nqa_last_error().decode()) == REFUSED[name], name  # (-3 would be a launch)
        seen.append(name)
    assert sorted(seen) == sorted(REFUSED)


def test_zero_rows_are_accepted_without_a_launch():
    from nequip_amd import _lib

    lib = _lib.load()
    for name, call in _empty(lib):
        assert call() == _lib.NQA_OK, name
