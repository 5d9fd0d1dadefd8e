"""``nequip_amd.train.EMAWeights`` on the multi-tensor HIP kernels (``nqa_ema_update`` / ``nqa_ema_swap``, csrc/ema.hip): against
the float64 restatement one step at a time (``tests/ema_restatement.py``: bound ``4 2^-24 (|a| + |b|)`` in float32,
``8 2^-53 (|a| + |b|)`` in float64), at misaligned views, under graph capture, and with the modules' weight caches."""
import copy
import os
import subprocess
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.join(HERE, "..")
sys.path.insert(0, HERE)
import ema_restatement as er  # noqa: E402

pytestmark = pytest.mark.gpu
NAN = float("nan")


@pytest.fixture(scope="module")
def fx():
    return er.Fixture()


def _model(tensors, device):
    m = torch.nn.Module()
    m.p = torch.nn.ParameterList([torch.nn.Parameter(t.clone().to(device)) for t in tensors])
    return m


def _set(tensors, values):
    with torch.no_grad():
        for t, v in zip(tensors, values):
            t.copy_(v)


def _native_launches(monkeypatch):
    """Counts the calls into the library: the tests below are about the kernels, not about the ATen form."""
    from nequip_amd import _lib

    lib, calls = _lib.load(), {"nqa_ema_update": 0, "nqa_ema_swap": 0}

    class Counting:
        def __getattr__(self, name):
            fn = getattr(lib, name)
            if name in calls:
                def counted(*a):
                    calls[name] += 1
                    return fn(*a)
                return counted
            return fn

    counting = Counting()
    monkeypatch.setattr(_lib, "load", lambda: counting)
    return calls


# ---- 1 ----------------------------------------------------------------------------------------------------------------------
def test_kernel_update_is_the_restatement_one_step_at_a_time(device, fx, monkeypatch):
    from nequip_amd import _lib
    from nequip_amd.train import EMAWeights

    assert fx.chunk == _lib.load().nqa_ema_chunk_elems()
    calls = _native_launches(monkeypatch)
    worst = 0.0
    for decay, steps in er.CHECKED.items():
        model = _model(fx.params(1), device)  # 7 float32 and 7 float64 parameters in ONE EMAWeights
        ema = EMAWeights(model, decay).to(device)
        for b in ema.ema_weights:
            b.fill_(NAN)
        for k in steps:
            params = fx.params(k)
            _set(model.parameters(), params)
            if k > 1:
                _set(ema.ema_weights, fx.ema(decay, k - 1))
                ema.num_updates = k - 1
            before = [b.clone() for b in ema.ema_weights]
            ema.update_parameters(model)
            assert ema.num_updates == k and ema.get_extra_state()["num_updates"] == k
            for i, (a, b, p) in enumerate(zip(ema.ema_weights, before, params)):
                worst = max(worst, er.assert_update(a, b, p, k - 1, decay, f"decay {decay} update {k} tensor {i}"))
    print(f"worst error / bound of the kernel: {worst:.3f}")
    assert calls["nqa_ema_update"] == sum(len(s) for s in er.CHECKED.values())


# ---- 2 ----------------------------------------------------------------------------------------------------------------------
def _views(chunk, device, seed):
    """A flat float32 buffer and views into it: every length at every element offset (mod 8), guard elements between them;
    then a view without elements."""
    lengths = [1, 3, 4, 7, chunk - 1, chunk, chunk + 1]
    offsets = [1, 2, 3, 5, 8]  # (8: the 16-byte aligned case, whose vectorised body ends in a tail for the odd lengths)
    spans, cursor = [], 0
    for j, off in enumerate(offsets):
        for n in lengths:
            start = (cursor + 5 + 7) // 8 * 8 + off
            spans.append((start, n))
            cursor = start + n
    spans.append((cursor + 3, 0))
    g = torch.Generator().manual_seed(seed)
    flat = torch.randn(cursor + 16, generator=g).to(device)
    return flat, spans


def test_misaligned_views_and_odd_lengths_stay_inside_their_bounds(device, fx, monkeypatch):
    """Parameters AND EMA buffers are views into flat buffers (at different offsets: every combination of aligned and
    misaligned sides occurs), so that a write past a view lands in a guard element of a buffer that is compared bit for bit."""
    from nequip_amd.train import EMAWeights

    calls = _native_launches(monkeypatch)
    chunk = fx.chunk
    p_flat, p_spans = _views(chunk, device, seed=1)
    e_flat, _ = _views(chunk, device, seed=2)
    e_spans = [(s + (3 if i % 2 else 0), n) for i, (s, n) in enumerate(p_spans)]  # (the guards are 5 elements and more)
    model = torch.nn.Module()
    model.p = torch.nn.ParameterList([torch.nn.Parameter(p_flat[s:s + n]) for s, n in p_spans])
    ema = EMAWeights(model, 0.5).to(device)
    for i, (s, n) in enumerate(e_spans):
        setattr(ema, f"ema_weight_{i}", e_flat[s:s + n])
    assert {p.data_ptr() % 16 for p in model.parameters()} >= {0, 4, 8, 12}
    inside = torch.zeros_like(e_flat, dtype=torch.bool)
    for s, n in e_spans:
        inside[s:s + n] = True

    def check_update(n_before):
        p0, e0 = p_flat.clone(), e_flat.clone()
        ema.update_parameters(model)
        assert torch.equal(er.bits(p_flat), er.bits(p0)), "an update must not write the parameters"
        assert torch.equal(er.bits(e_flat)[~inside], er.bits(e0)[~inside]), "written outside the EMA views"
        for (ps, n), (es, _) in zip(p_spans, e_spans):
            er.assert_update(e_flat[es:es + n], e0[es:es + n], p0[ps:ps + n], n_before, 0.5, f"view at {ps} / {es}, {n} elements")

    e_flat[inside] = NAN
    check_update(0)
    p_flat.add_(torch.randn(p_flat.shape, generator=torch.Generator().manual_seed(3)).to(device))
    check_update(1)
    assert ema.num_updates == 2

    p0, e0 = p_flat.clone(), e_flat.clone()
    ema.swap_parameters(model)
    for (ps, n), (es, _) in zip(p_spans, e_spans):
        assert torch.equal(er.bits(p_flat[ps:ps + n]), er.bits(e0[es:es + n]))
        assert torch.equal(er.bits(e_flat[es:es + n]), er.bits(p0[ps:ps + n]))
    p_inside = torch.zeros_like(inside)
    for s, n in p_spans:
        p_inside[s:s + n] = True
    assert torch.equal(er.bits(p_flat)[~p_inside], er.bits(p0)[~p_inside]), "swap wrote outside the parameter views"
    assert torch.equal(er.bits(e_flat)[~inside], er.bits(e0)[~inside]), "swap wrote outside the EMA views"
    assert calls == {"nqa_ema_update": 2, "nqa_ema_swap": 1}


def test_float64_views_take_the_two_element_packs_inside_their_bounds(device, fx, monkeypatch):
    """The float64 form of the shared chunk walker (packs of two elements): float64 EMA and parameter views of 1, C - 1, C and
    C + 1 elements at byte offsets 0 and 8 (mod 16) into guarded flat buffers, every combination of the two sides (only 0 / 0
    takes the 16-byte accesses, with a one-element tail for the odd lengths).  One copying update, one averaging update and one
    swap; the guards are compared bit for bit."""
    from nequip_amd.train import EMAWeights

    calls = _native_launches(monkeypatch)
    chunk = fx.chunk
    p_spans, e_spans, cursor = [], [], 0
    for n in (1, chunk - 1, chunk, chunk + 1):
        for p_off in (0, 1):
            for e_off in (0, 1):
                start = (cursor + 3 + 1) // 2 * 2  # an even element (16 bytes) behind three guard elements or more
                p_spans.append((start + p_off, n))
                e_spans.append((start + e_off, n))
                cursor = start + 1 + n
    g = torch.Generator().manual_seed(5)
    p_flat = torch.randn(cursor + 4, generator=g, dtype=torch.float64).to(device)
    e_flat = torch.randn(cursor + 4, generator=g, dtype=torch.float64).to(device)
    assert p_flat.data_ptr() % 16 == 0 and e_flat.data_ptr() % 16 == 0
    model = torch.nn.Module()
    model.p = torch.nn.ParameterList([torch.nn.Parameter(p_flat[s:s + n]) for s, n in p_spans])
    ema = EMAWeights(model, 0.5).to(device)
    for i, (s, n) in enumerate(e_spans):
        setattr(ema, f"ema_weight_{i}", e_flat[s:s + n])
    assert {(p.data_ptr() % 16, b.data_ptr() % 16) for p, b in zip(model.parameters(), ema.ema_weights)} == \
        {(0, 0), (0, 8), (8, 0), (8, 8)}
    p_inside, e_inside = torch.zeros_like(p_flat, dtype=torch.bool), torch.zeros_like(e_flat, dtype=torch.bool)
    for (ps, n), (es, _) in zip(p_spans, e_spans):
        p_inside[ps:ps + n] = True
        e_inside[es:es + n] = True

    e_flat[e_inside] = NAN
    for n_before in (0, 1):
        p0, e0 = p_flat.clone(), e_flat.clone()
        ema.update_parameters(model)
        assert torch.equal(er.bits(p_flat), er.bits(p0)), "an update must not write the parameters"
        assert torch.equal(er.bits(e_flat)[~e_inside], er.bits(e0)[~e_inside]), "written outside the EMA views"
        for (ps, n), (es, _) in zip(p_spans, e_spans):
            er.assert_update(e_flat[es:es + n], e0[es:es + n], p0[ps:ps + n], n_before, 0.5, f"view at {ps} / {es}, {n} elements")
        p_flat.add_(torch.randn(p_flat.shape, generator=g, dtype=torch.float64).to(device))

    p0, e0 = p_flat.clone(), e_flat.clone()
    ema.swap_parameters(model)
    for (ps, n), (es, _) in zip(p_spans, e_spans):
        assert torch.equal(er.bits(p_flat[ps:ps + n]), er.bits(e0[es:es + n]))
        assert torch.equal(er.bits(e_flat[es:es + n]), er.bits(p0[ps:ps + n]))
    assert torch.equal(er.bits(p_flat)[~p_inside], er.bits(p0)[~p_inside]), "swap wrote outside the parameter views"
    assert torch.equal(er.bits(e_flat)[~e_inside], er.bits(e0)[~e_inside]), "swap wrote outside the EMA views"
    assert calls == {"nqa_ema_update": 2, "nqa_ema_swap": 1}


# ---- 3 ----------------------------------------------------------------------------------------------------------------------
def test_swap_is_exact_in_place_and_bumps_versions(device, fx, monkeypatch):
    from nequip_amd.train import EMAWeights

    calls = _native_launches(monkeypatch)
    model = _model(fx.params(1), device)
    ema = EMAWeights(model, 0.5).to(device)
    ema.update_parameters(model)
    _set(model.parameters(), fx.params(2))
    ema.update_parameters(model)
    with torch.no_grad():
        model.p[2][0], model.p[9][1] = NAN, -0.0  # (payloads and signed zeros travel too)
    p0, e0 = [p.detach().clone() for p in model.parameters()], [b.clone() for b in ema.ema_weights]
    tensors = list(model.parameters()) + ema.ema_weights
    versions = [t._version for t in tensors]
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(device)
    allocated = torch.cuda.memory_allocated(device)
    ema.swap_parameters(model)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated(device) == allocated, "a swap must not allocate"
    assert calls["nqa_ema_swap"] == 1 and not ema.is_holding_ema_weights
    assert all(t._version > v for t, v in zip(tensors, versions))
    for p, b, pw, ew in zip(model.parameters(), ema.ema_weights, p0, e0):
        assert torch.equal(er.bits(p), er.bits(ew)) and torch.equal(er.bits(b), er.bits(pw))
    with pytest.raises(AssertionError, match="not holding EMA weights"):
        ema.update_parameters(model)
    ema.swap_parameters(model)
    assert ema.is_holding_ema_weights
    for p, b, pw, ew in zip(model.parameters(), ema.ema_weights, p0, e0):
        assert torch.equal(er.bits(p), er.bits(pw)) and torch.equal(er.bits(b), er.bits(ew))


# ---- 4 ----------------------------------------------------------------------------------------------------------------------
def test_captured_update_advances_the_warm_up_on_every_replay(device, fx):
    from nequip_amd.train import EMAWeights

    decay, replays = 0.5, 12
    model = _model(fx.params(1), device)
    ema = EMAWeights(model, decay).to(device)
    deltas = [(0.05 * (p.detach().abs() + 1.0)).clone() for p in model.parameters()]

    def step():
        with torch.no_grad():
            for p, d in zip(model.parameters(), deltas):
                p.add_(d)
        ema.update_parameters(model)

    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="once eagerly"):
        with torch.cuda.graph(graph):
            ema.update_parameters(model)
    torch.cuda.synchronize()
    assert ema.num_updates == 0

    ema.update_parameters(model)  # eagerly: builds the device tables, copies
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with pytest.raises(RuntimeError, match="cannot be captured"):
        with torch.cuda.graph(graph):
            ema.swap_parameters(model)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        step()
    torch.cuda.synchronize()
    assert ema.num_updates == 1 and ema.is_holding_ema_weights, "capturing must not run the update"

    capture_weight = er.weight(decay, 1)  # what a host scalar would have frozen into the graph
    frozen = [b.detach().cpu().double() for b in ema.ema_weights]
    for r in range(1, replays + 1):
        before = [b.clone() for b in ema.ema_weights]
        graph.replay()
        torch.cuda.synchronize()
        params = [p.detach().clone() for p in model.parameters()]
        for i, (a, b, p) in enumerate(zip(ema.ema_weights, before, params)):
            er.assert_update(a, b, p, r, decay, f"replay {r} tensor {i}")
        frozen = [f + (p.cpu().double() - f) * capture_weight for f, p in zip(frozen, params)]
    assert ema.num_updates == replays + 1 == 13
    # the frozen-scalar form is a different average, by far more than the bound
    for a, f, p in zip(ema.ema_weights, frozen, params):
        gap = (a.cpu().double() - f).abs()
        bound = er.EPS[a.dtype] * (a.cpu().double().abs() + p.cpu().double().abs())
        assert bool((gap > 1000.0 * bound).all())


# ---- 5 ----------------------------------------------------------------------------------------------------------------------
def test_swapped_weights_reach_the_cached_weight_images(device, monkeypatch):
    """The modules keep derived weight images keyed on ``(data_ptr, _version)``; the kernels write through raw pointers.  An
    eval-mode model with filled caches must evaluate with the averaged weights inside ``average_parameters`` and with its own
    again afterwards: this fails without the version bumps."""
    from nequip_amd.data import AtomicDataDict as K
    from nequip_amd.train import EMAWeights
    from nequip_amd.utils import synthetic as syn
    from test_zbl_gpu import _models

    calls = _native_launches(monkeypatch)
    pos, types, cell, names = syn.water_box(n_side=3, seed=8)
    data = K.to_device(syn.make_data(pos, types, 4.5, cell), device)
    model = _models(device)[1].eval()
    twin = copy.deepcopy(model)  # never evaluated before it gets the averaged weights: nothing cached

    def evaluate(m):
        out = m(dict(data))
        return out[K.TOTAL_ENERGY_KEY].detach().clone(), out[K.FORCE_KEY].detach().clone()

    evaluate(model)
    ema = EMAWeights(model, 0.5)
    ema.update_parameters(model)
    g = torch.Generator().manual_seed(11)
    for _ in range(3):
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(1.0 + 0.05 * torch.randn(p.shape, generator=g).to(device))
        ema.update_parameters(model)
    e_raw, f_raw = evaluate(model)  # fills the caches with the images of the raw weights

    with ema.average_parameters(model):
        e_avg, f_avg = evaluate(model)
    _set(twin.parameters(), ema.ema_weights)
    e_twin, f_twin = evaluate(twin)
    assert not torch.equal(e_raw, e_twin), "the averaged weights must differ from the raw ones for this test to say anything"
    assert torch.equal(e_avg, e_twin) and torch.equal(f_avg, f_twin)
    e_back, f_back = evaluate(model)
    assert torch.equal(e_back, e_raw) and torch.equal(f_back, f_raw)
    assert calls == {"nqa_ema_update": 4, "nqa_ema_swap": 2}


# ---- 6 ----------------------------------------------------------------------------------------------------------------------
_TRAIN_CAPTURE = r"""
import sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[2])
import torch
import ema_restatement as er
from nequip_amd.data import AtomicDataDict as K
from nequip_amd.train import EMAWeights, EnergyForceLoss
from nequip_amd.utils import synthetic as syn
from test_zbl_gpu import _models

device = torch.device("cuda:0")
pos, types, cell, names = syn.water_box(n_side=3, seed=8)
data = K.to_device(syn.make_data(pos, types, 4.5, cell), device)
n = len(pos)
model = _models(device)[1].train()
gen = torch.Generator().manual_seed(0)
target = {"forces": torch.randn(n, 3, generator=gen, dtype=torch.float64).to(device),
          "total_energy": torch.randn(1, 1, generator=gen, dtype=torch.float64).to(device),
          "num_atoms": torch.tensor([n], device=device)}
loss_fn = EnergyForceLoss()
opt = torch.optim.Adam(model.parameters(), lr=1e-2, capturable=True)
decay = 0.999
ema = EMAWeights(model, decay)

def step():
    opt.zero_grad(set_to_none=True)
    out = dict(model(dict(data)))
    out["num_atoms"] = target["num_atoms"]
    loss_fn(out, target)["weighted_sum"].backward()
    opt.step()
    ema.update_parameters(model)

side = torch.cuda.Stream(device=device)
side.wait_stream(torch.cuda.current_stream(device))
with torch.cuda.stream(side):
    for _ in range(2):
        step()
torch.cuda.current_stream(device).wait_stream(side)
torch.cuda.synchronize()
graph = torch.cuda.CUDAGraph()
opt.zero_grad(set_to_none=True)
with torch.cuda.graph(graph):
    step()
torch.cuda.synchronize()
assert ema.num_updates == 2
for r in range(2):
    before = [b.clone() for b in ema.ema_weights]
    old = [p.detach().clone() for p in model.parameters()]
    graph.replay()
    torch.cuda.synchronize()
    params = [p.detach().clone() for p in model.parameters()]
    assert any(not torch.equal(a, b) for a, b in zip(old, params)), "the optimizer did not move the parameters"
    worst = 0.0
    for i, (a, b, p) in enumerate(zip(ema.ema_weights, before, params)):
        worst = max(worst, er.assert_update(a, b, p, 2 + r, decay, f"replay {r} parameter {i}"))
    print(f"replay {r}: worst error / bound {worst:.3f}")
assert ema.num_updates == 4
print("EMA_CAPTURE_OK")
"""


def test_training_step_with_ema_is_capturable(device):
    """Forward, double backward, ``EnergyForceLoss``, capturable Adam and the EMA update in one hipGraph, replayed twice (a
    fresh process under one time limit, as ``test_energy_head_train.py`` does for its captured step)."""
    r = subprocess.run([sys.executable, "-c", _TRAIN_CAPTURE, ROOT, HERE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "EMA_CAPTURE_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
