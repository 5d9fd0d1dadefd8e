"""sha256 of every result of the slot-reduction kernels (``csrc/metrics.hip``, ``csrc/stats.hip``, ``csrc/training_stats.hip``) on
the inputs of the GPU tests, to compare two builds bit for bit:

    python scripts/slot_reduce_checksums.py <tree with a built nequip_amd> <out file> [label]

Run it once per build in separate processes and compare the lines that do not start with ``#``.  The inputs come from this
checkout's tests (``test_metrics_gpu.py``: its rows x cols x dtype grid, the 32-term stream, the energy/force/stress manager;
``stats_cases.py`` at ``COUNTS`` on node and edge streams, the NaN cases and the neighbour counts; the training-statistics
cases), the library and its Python host layer from ``<tree>``.  Hashed: metrics -- the value vector, ``saved``, the epoch state
and every ``grad_pred`` (upstream: ``weighted_sum``, then a fixed weight on every value); statistics -- the whole state after
the batches and the neighbour counts; training statistics -- the device tables and ``compute()``."""
import hashlib, itertools, math, os, struct, sys
tree, out_path = os.path.abspath(sys.argv[1]), sys.argv[2]
label = sys.argv[3] if len(sys.argv) > 3 else ""
sys.path.insert(0, tree)
import torch
import nequip_amd  # (before the test modules, which put their own checkout in front of sys.path)
from nequip_amd import _lib
assert os.path.dirname(os.path.abspath(nequip_amd.__file__)) == os.path.join(tree, "nequip_amd"), nequip_amd.__file__
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import stats_cases as sc
import test_data_statistics_gpu as tds
import test_metrics_gpu as tm
import test_training_stats_gpu as tts
from nequip_amd.data import DataStatisticsManager
from nequip_amd.train import MetricsManager, TrainingStatsMonitor
dev = torch.device("cuda:0")
F32, F64 = torch.float32, torch.float64
lines = []


def sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


# ---- metrics ----------------------------------------------------------------------------------------------------------------
def metrics_case(name, manager, preds, target):
    plan, vectors = manager.__dict__["_plan"], []
    evaluate = plan.evaluate
    plan.evaluate = lambda *a, **k: vectors.append(evaluate(*a, **k)) or vectors[-1]
    floats = [k for k, v in preds.items() if v.is_floating_point()]
    p = {k: (v.to(dev).requires_grad_(True) if k in floats else v.to(dev)) for k, v in preds.items()}
    out = manager(p, {k: v.to(dev) for k, v in target.items()})
    (vec,) = vectors
    lines.append(f"metrics {name} values {sha(vec)}")
    lines.append(f"metrics {name} state {sha(plan.buffers(dev)['state'])}")
    if vec.grad_fn is None:
        return
    lines.append(f"metrics {name} saved {sha(vec.grad_fn.saved_tensors[0])}")
    weights = torch.linspace(0.5, 1.5, vec.numel(), dtype=F64, device=dev)
    for up_name, up in (("weighted_sum", out["weighted_sum"]), ("all", (vec * weights).sum())):
        grads = torch.autograd.grad(up, [p[k] for k in floats], allow_unused=True, retain_graph=True)
        for k, g in zip(floats, grads):
            lines.append(f"metrics {name} d {up_name} / d {k} {'none' if g is None else sha(g)}")


entries = tm.entries_for_kernel_test()
dtypes = [(F32, F32), (F32, F64), (F64, F32), (F64, F64)]
for rows, cols, (pd, td) in itertools.product([0, 1, 3, 257, tm.G * 256 + 5], [1, 3, 9], dtypes):
    g = torch.Generator().manual_seed(rows * 10 + cols)  # (the inputs of test_kernel_against_restatement)
    types = torch.randint(0, 2, (rows,), generator=g)
    types[:1] = 0
    preds = {"forces": torch.randn(rows, 2 * cols, generator=g, dtype=pd)[:, ::2],
             "fnan": torch.randn(rows, cols, generator=g, dtype=pd), "fall": torch.randn(rows, cols, generator=g, dtype=pd),
             "atom_types": types}
    target = {"forces": (2.0 * torch.randn(rows, cols, generator=g, dtype=F64)).to(td),
              "fnan": torch.randn(rows, cols, generator=g, dtype=F64).to(td),
              "fall": torch.full((rows, cols), math.nan, dtype=td)}
    target["fnan"][torch.rand(rows, cols, generator=g) < 0.25] = math.nan
    manager = MetricsManager([tm.to_dict(e) for e in entries], type_names=tm.TYPES)
    metrics_case(f"grid rows={rows} cols={cols} {str(pd)[6:]}/{str(td)[6:]}", manager, preds, target)

kinds = [("mse", {}), ("mae", {}), ("rmse", {}), ("max_ae", {}), ("huber", {"delta": 0.7}),
         ("huber", {"delta": 0.4, "reduction": "sum"}), ("stratified huber", {"delta_dict": {1.0: 0.5, 3.0: 0.2}})]
entries = []
for i in range(32):  # (test_thirty_two_terms_on_one_stream)
    kind, kw = kinds[i % len(kinds)]
    e = {"name": f"t{i}", "field": "forces", "kind": kind, "coeff": None if kind == "max_ae" else 1.0 + i, **kw}
    if i >= 28 and kind != "stratified huber":
        e["per_type"] = True
    entries.append(e)
g = torch.Generator().manual_seed(11)
types = torch.randint(0, 2, (257,), generator=g)
preds = {"forces": torch.randn(257, 3, generator=g), "atom_types": types}
target = {"forces": 2.0 * torch.randn(257, 3, generator=g, dtype=F64)}
metrics_case("32 terms", MetricsManager([tm.to_dict(e) for e in entries], type_names=tm.TYPES), preds, target)

manager = tm.efs_metrics()  # (test_fused_manager_energy_force_stress_metrics: two batches into one epoch state)
metrics_case("efs batch 1", manager, *tm.efs_batch([5, 64, 300], seed=1, absent_type=2, nan_frames=[1]))
metrics_case("efs batch 2", manager, *tm.efs_batch([7, 33], seed=2, absent_type=None, nan_frames=[]))


# ---- dataset statistics -----------------------------------------------------------------------------------------------------
def stats_case(name, entries, batches):
    m = DataStatisticsManager(sc.to_dicts(entries), type_names=sc.TYPES)
    m.get_statistics([dict(b) for b in batches])
    lines.append(f"stats {name} state {sha(m._plan.buffers(dev)['state'])}")
    return m


for dtype, n in itertools.product([F32, F64], tds.COUNTS):
    entries = sc.entries_for(("charges",)) + sc.entries_for(("forces",), kinds=["rms", "std", "max"])
    batches = [sc.make_batch(tds.frames_of(k, 3), 100 + i, dtype, num_edges=8, device=dev)
               for i, k in enumerate([n, (n + 1) // 2, n])]
    stats_case(f"node n={n} {str(dtype)[6:]}", entries, batches)
for e in tds.COUNTS:
    batches = [sc.make_batch([20, 30], 200 + i, num_edges=k, type_choices=(0, 1, 2), device=dev)
               for i, k in enumerate([e, (e + 1) // 2, e])]
    stats_case(f"edge e={e}", sc.entries_for(("edge_lengths",)), batches)
for dtype in (F32, F64):
    entries = sc.entries_for(("fnan",), kinds=["mean", "rms", "std", "max", "absmin", "count"], ignore_nan=(False, True))
    stats_case(f"nan {str(dtype)[6:]}", entries, sc.three_batches(dtype, device=dev))
batches = [sc.make_batch(tds.frames_of(n, 3), 400 + i, device=dev) for i, n in enumerate([257, 1, 700])]
m = stats_case("num_neighbors", sc.entries_for(("num_neighbors",)), batches)
for i, b in enumerate(batches):
    lines.append(f"stats neighbor_counts batch {i} {sha(m._plan.neighbor_counts(b['edge_index'], len(b['pos'])))}")


# ---- training statistics ----------------------------------------------------------------------------------------------------
def tstats_case(name, mon):
    for s in (mon._gradients, mon._step):
        if s.tables is not None:
            lines.append(f"tstats {name} {s.what} table {sha(s.tables.out[:s.tables.n_tensors])}")
    got = mon.compute()
    packed = b"".join(k.encode() + struct.pack("<d", float(v)) for k, v in sorted(got.items()))
    lines.append(f"tstats {name} compute {hashlib.sha256(packed).hexdigest()}")


c = tts._chunk()
shapes = {"1": (1,), "5": (5,), "c-1": (c - 1,), "c": (c,), "c+1": (c + 1,), "2c+3": (2 * c + 3,), "64x64": (64, 64),
          "negative": (c + 5,), "float64": (c + 7,), "view": (c + 2,)}
for case in tts.CASES:  # (test_one_tensor_against_the_restatement)
    x = tts._randn(shapes[case], seed=tts.CASES.index(case), dtype=F64 if case == "float64" else F32)
    if case == "negative":
        x = -x.abs() - 0.25
    if case == "view":
        buf = torch.zeros(x.numel() + 9, device=dev)
        buf[1:1 + x.numel()] = x.to(dev)
        x = buf[1:1 + x.numel()]
    model = tts._module([x.to(dev)])
    model.p[0].grad = (model.p[0].detach() * 3.0).clone()
    mon = TrainingStatsMonitor(log_freq=1)
    mon.on_after_backward(model)
    mon.on_before_optimizer_step(model, [])
    tstats_case(f"one tensor {case}", mon)
for case in ("nan", "+inf", "+inf-inf"):  # (test_non_finite_elements)
    xs = [tts._randn((2 * c + 3,), 1), tts._randn((c + 1,), 2), tts._randn((17,), 3)]
    xs[0][c + c // 2] = math.nan if case == "nan" else math.inf
    if case == "+inf-inf":
        xs[0][5] = -math.inf
    model = tts._module([x.to(dev) for x in xs])
    for p in model.parameters():
        p.grad = p.detach().clone()
    mon = TrainingStatsMonitor(log_freq=1)
    mon.on_after_backward(model)
    mon.on_before_optimizer_step(model, [])
    tstats_case(f"non-finite {case}", mon)
model = tts.Mixed(c).to(dev)  # (the whole module with Adam: weights, gradients, both moments, three steps)
opt = torch.optim.Adam(model.parameters(), lr=1e-3, capturable=True)
mon = TrainingStatsMonitor(log_freq=1)
tts._train(model, opt, mon, 3)
tstats_case("mixed module, 3 Adam steps", mon)

torch.cuda.synchronize()
open(out_path, "w").write(f"# {label}: python scripts/slot_reduce_checksums.py <tree> <out> on {torch.cuda.get_device_name(0)}\n"
                          + "\n".join(lines) + "\n")
print("wrote", len(lines), "checksums to", out_path, "from", _lib.LIB_PATH)
