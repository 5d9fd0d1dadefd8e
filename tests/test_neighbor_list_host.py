"""Host side of the device neighbour list (``nequip_amd/csrc/neighbor_list.hip``), no GPU: the workspace sizes of every form of
the list and the calls that are refused before anything is launched.

The literals were printed by the library as it was before the host code was folded into one layout function and one driver
per pass; they pin the layout (order of the fields, 256-byte alignment) and the argument checks of the C ABI."""

import ctypes

NS, FS, TS = (0, 1, 63, 64, 1000, 10125), (1, 4, 256), (1, 3, 32768)

SINGLE = {0: 1024, 1: 3072, 63: 7168, 64: 7424, 1000: 101120, 10125: 1014784}
TYPED = {(0, 1): 1280,
 (0, 3): 1280,
 (0, 32768): 8589935616,
 (1, 1): 3584,
 (1, 3): 3584,
 (1, 32768): 8589937920,
 (63, 1): 7680,
 (63, 3): 7680,
 (63, 32768): 8589942016,
 (64, 1): 7936,
 (64, 3): 7936,
 (64, 32768): 8589942272,
 (1000, 1): 105472,
 (1000, 3): 105472,
 (1000, 32768): 8590039808,
 (10125, 1): 1055744,
 (10125, 3): 1055744,
 (10125, 32768): 8590990080}
BATCHED = {(0, 1): 1280,
 (0, 4): 2048,
 (0, 256): 81664,
 (1, 1): 3584,
 (1, 4): 4352,
 (1, 256): 83968,
 (63, 1): 7680,
 (63, 4): 8448,
 (63, 256): 87552,
 (64, 1): 7936,
 (64, 4): 8704,
 (64, 256): 88320,
 (1000, 1): 105472,
 (1000, 4): 106752,
 (1000, 256): 185856,
 (10125, 1): 1055744,
 (10125, 4): 1056512,
 (10125, 256): 1136128}
BATCHED_TYPED = {(0, 1, 1): 1536,
 (0, 1, 3): 1536,
 (0, 1, 32768): 8589935872,
 (0, 4, 1): 2304,
 (0, 4, 3): 2304,
 (0, 4, 32768): 8589936640,
 (0, 256, 1): 81920,
 (0, 256, 3): 81920,
 (0, 256, 32768): 8590016256,
 (1, 1, 1): 4096,
 (1, 1, 3): 4096,
 (1, 1, 32768): 8589938432,
 (1, 4, 1): 4864,
 (1, 4, 3): 4864,
 (1, 4, 32768): 8589939200,
 (1, 256, 1): 84480,
 (1, 256, 3): 84480,
 (1, 256, 32768): 8590018816,
 (63, 1, 1): 8192,
 (63, 1, 3): 8192,
 (63, 1, 32768): 8589942528,
 (63, 4, 1): 8960,
 (63, 4, 3): 8960,
 (63, 4, 32768): 8589943296,
 (63, 256, 1): 88064,
 (63, 256, 3): 88064,
 (63, 256, 32768): 8590022400,
 (64, 1, 1): 8448,
 (64, 1, 3): 8448,
 (64, 1, 32768): 8589942784,
 (64, 4, 1): 9216,
 (64, 4, 3): 9216,
 (64, 4, 32768): 8589943552,
 (64, 256, 1): 88832,
 (64, 256, 3): 88832,
 (64, 256, 32768): 8590023168,
 (1000, 1, 1): 109824,
 (1000, 1, 3): 109824,
 (1000, 1, 32768): 8590044160,
 (1000, 4, 1): 111104,
 (1000, 4, 3): 111104,
 (1000, 4, 32768): 8590045440,
 (1000, 256, 1): 190208,
 (1000, 256, 3): 190208,
 (1000, 256, 32768): 8590124544,
 (10125, 1, 1): 1096704,
 (10125, 1, 3): 1096704,
 (10125, 1, 32768): 8591031040,
 (10125, 4, 1): 1097472,
 (10125, 4, 3): 1097472,
 (10125, 4, 32768): 8591031808,
 (10125, 256, 1): 1177088,
 (10125, 256, 3): 1177088,
 (10125, 256, 32768): 8591111424}


def test_workspace_sizes_of_every_form():
    from nequip_amd import _lib

    lib = _lib.load()
    assert set(SINGLE) == set(NS) and set(TYPED) == {(n, t) for n in NS for t in TS}
    assert set(BATCHED) == {(n, f) for n in NS for f in FS}
    assert set(BATCHED_TYPED) == {(n, f, t) for n in NS for f in FS for t in TS}
    for n, want in SINGLE.items():
        assert lib.nqa_neighbor_list_workspace_bytes(n) == want, n
    for (n, t), want in TYPED.items():
        assert lib.nqa_neighbor_list_typed_workspace_bytes(n, t) == want, (n, t)
    for (n, f), want in BATCHED.items():
        assert lib.nqa_neighbor_list_batched_workspace_bytes(n, f) == want, (n, f)
    for (n, f, t), want in BATCHED_TYPED.items():
        assert lib.nqa_neighbor_list_batched_typed_workspace_bytes(n, f, t) == want, (n, f, t)
    # a typed workspace begins with the untyped one: the typed fields come last
    for (n, f, t), want in BATCHED_TYPED.items():
        assert want > BATCHED[(n, f)] and TYPED[(n, t)] > SINGLE[n]
    # no size for counts outside the domain
    assert lib.nqa_neighbor_list_workspace_bytes(-1) == -1
    for n, t in ((-1, 3), (64, 0), (64, -1), (64, 32769)):
        assert lib.nqa_neighbor_list_typed_workspace_bytes(n, t) == -1, (n, t)
    for n, f in ((-1, 4), (64, 0), (64, -1)):
        assert lib.nqa_neighbor_list_batched_workspace_bytes(n, f) == -1, (n, f)
    for n, f, t in ((-1, 4, 3), (64, 0, 3), (64, 4, 0), (64, 4, 32769)):
        assert lib.nqa_neighbor_list_batched_typed_workspace_bytes(n, f, t) == -1, (n, f, t)


def _refusals(lib):
    """``(name, call)``: calls that return before a launch.  The pointers are host buffers nothing reads; the single-frame
    typed count gets a null ``status`` because it zeroes a non-null one on the stream before it looks at its arguments."""
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    N, F, T = 10, 2, 3
    big = lib.nqa_neighbor_list_batched_typed_workspace_bytes(N, F, T)
    count = lib.nqa_neighbor_list_count
    yield "count: num_atoms = -1", lambda: count(p, p, p, 4.0, -1, p, big, p, None)
    yield "count: r_max = 0", lambda: count(p, p, p, 0.0, N, p, big, p, None)
    yield "count: null rowptr", lambda: count(p, p, p, 4.0, N, p, big, None, None)
    yield "count: one-byte workspace", lambda: count(p, p, p, 4.0, N, p, 1, p, None)
    yield "count: null workspace", lambda: count(p, p, p, 4.0, N, None, big, p, None)
    yield "count_typed: null status", lambda: lib.nqa_neighbor_list_count_typed(
        p, p, p, 4.0, p, p, T, 0, N, p, big, p, None, None)
    yield "fill_padded: odd capacity", lambda: lib.nqa_neighbor_list_fill_padded(p, p, N, 7, p, p, p, p, p, None)
    yield "batched_count: num_frames = 0", lambda: lib.nqa_neighbor_list_batched_count(p, p, p, p, 4.0, N, 0, p, big, p, p, None)
    yield "batched_count: one-byte workspace", lambda: lib.nqa_neighbor_list_batched_count(
        p, p, p, p, 4.0, N, F, p, 1, p, p, None)
    yield "batched_count_typed: num_types = 32769", lambda: lib.nqa_neighbor_list_batched_count_typed(
        p, p, p, p, 4.0, p, p, 32769, N, F, p, big, p, p, None)
    yield "fill: num_edges = -1", lambda: lib.nqa_neighbor_list_fill(p, p, N, -1, p, p, None)
    yield "fill_typed: num_types = 0", lambda: lib.nqa_neighbor_list_fill_typed(p, p, p, N, 0, 8, p, p, None)
    yield "fill_padded_typed: num_types = 0", lambda: lib.nqa_neighbor_list_fill_padded_typed(
        p, p, p, N, 0, 8, p, p, p, p, p, None)
    yield "batched_fill: num_frames = 0", lambda: lib.nqa_neighbor_list_batched_fill(p, p, N, 0, 8, p, p, None)
    yield "batched_fill_typed: num_types = 0", lambda: lib.nqa_neighbor_list_batched_fill_typed(p, p, p, N, F, 0, 8, p, p, None)


REFUSED = {
    "count: num_atoms = -1": (-1, "nqa_neighbor_list_count: invalid argument"),
    "count: r_max = 0": (-1, "nqa_neighbor_list_count: invalid argument"),
    "count: null rowptr": (-1, "nqa_neighbor_list_count: invalid argument"),
    "count: one-byte workspace": (-4, "nqa_neighbor_list_count: workspace missing or too small"),
    "count: null workspace": (-4, "nqa_neighbor_list_count: workspace missing or too small"),
    "count_typed: null status": (-1, "nqa_neighbor_list_count_typed: invalid argument"),
    "fill_padded: odd capacity": (
        -1, "nqa_neighbor_list_fill_padded: invalid argument (needs atoms and an even capacity below 2^31)"),
    "batched_count: num_frames = 0": (-1, "nqa_neighbor_list_batched_count: invalid argument"),
    "batched_count: one-byte workspace": (-4, "nqa_neighbor_list_batched_count: workspace missing or too small"),
    "batched_count_typed: num_types = 32769": (-1, "nqa_neighbor_list_batched_count_typed: invalid argument"),
    "fill: num_edges = -1": (-1, "nqa_neighbor_list_fill: invalid argument"),
    "fill_typed: num_types = 0": (-1, "nqa_neighbor_list_fill_typed: invalid argument"),
    "fill_padded_typed: num_types = 0": (
        -1, "nqa_neighbor_list_fill_padded_typed: invalid argument (needs atoms, types and an even capacity below 2^31)"),
    "batched_fill: num_frames = 0": (-1, "nqa_neighbor_list_batched_fill: invalid argument"),
    "batched_fill_typed: num_types = 0": (-1, "nqa_neighbor_list_batched_fill_typed: invalid argument"),
}


def test_calls_refused_before_any_launch():
    from nequip_amd import _lib

    lib = _lib.load()
    seen = []
    for name, call in _refusals(lib):
        rc = call()
        assert (rc, lib.nqa_last_error().decode()) == REFUSED[name], name
        seen.append(name)
    assert sorted(seen) == sorted(REFUSED)
    # the fills of an empty list are accepted without a launch
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.nqa_neighbor_list_fill(p, p, 0, 0, None, None, None) == _lib.NQA_OK
    assert lib.nqa_neighbor_list_fill(p, p, 10, 0, None, None, None) == _lib.NQA_OK
    assert lib.nqa_neighbor_list_fill_typed(p, p, None, 0, 3, 0, None, None, None) == _lib.NQA_OK
    assert lib.nqa_neighbor_list_batched_fill(p, p, 10, 2, 0, None, None, None) == _lib.NQA_OK
    assert lib.nqa_neighbor_list_batched_fill_typed(p, p, p, 10, 2, 3, 0, None, None, None) == _lib.NQA_OK
