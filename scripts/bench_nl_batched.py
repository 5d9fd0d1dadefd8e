"""Per-frame loop vs batched device neighbour list on batches of many systems (NQA_NL_PER_FRAME=1 is the loop), and one
NequIPTorchSimCalc.forward on the first shape.  Prints one JSON line per case; `--out FILE` also writes them to FILE."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from nequip_amd.data import AtomicDataDict as K  # noqa: E402
from nequip_amd.data._nl import compute_neighborlist_  # noqa: E402
from nequip_amd.utils import synthetic as syn  # noqa: E402

R_MAX = 4.5


def _box(n, seed, density=0.08):
    """n random atoms in a periodic cubic box (no minimum distance: a stand-in for a small crystal)."""
    rng = np.random.default_rng(seed)
    L = (n / density) ** (1.0 / 3.0)
    return rng.uniform(0.0, L, size=(n, 3)), np.eye(3) * L, (True,) * 3


def _molecule(n, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(0.0, 0.9 * n ** (1.0 / 3.0), size=(n, 3)), np.zeros((3, 3)), (False,) * 3


def _batch(frames, device):
    n = [len(p) for p, _, _ in frames]
    return {
        K.POSITIONS_KEY: torch.tensor(np.concatenate([p for p, _, _ in frames]), dtype=torch.float64, device=device),
        K.CELL_KEY: torch.tensor(np.stack([c for _, c, _ in frames]), dtype=torch.float64, device=device),
        K.PBC_KEY: torch.tensor([b for _, _, b in frames], dtype=torch.bool, device=device),
        K.BATCH_KEY: torch.repeat_interleave(torch.arange(len(frames)), torch.tensor(n)).to(device),
        K.NUM_NODES_KEY: torch.tensor(n, dtype=torch.long, device=device),
    }


def _time(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts)) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(0)
    cases = {
        "256x64_periodic": [_box(int(rng.integers(56, 73)), s) for s in range(256)],
        "32x256_train256": [_box(256, 1000 + s) for s in range(32)],
        "mixed_128": [(_molecule(int(rng.integers(8, 40)), s) if s % 2 else _box(int(rng.integers(32, 128)), s))
                      for s in range(128)],
    }
    lines = []
    for name, frames in cases.items():
        data = _batch(frames, dev)
        res = {"case": name, "frames": len(frames), "atoms": int(data[K.POSITIONS_KEY].shape[0])}
        for mode, env in (("per_frame", "1"), ("batched", "0")):
            os.environ["NQA_NL_PER_FRAME"] = env
            res[f"{mode}_ms"] = _time(lambda: compute_neighborlist_(dict(data), R_MAX), args.warmup, args.reps)
        os.environ.pop("NQA_NL_PER_FRAME")
        res["edges"] = int(compute_neighborlist_(dict(data), R_MAX)[K.EDGE_INDEX_KEY].shape[1])
        res["speedup"] = res["per_frame_ms"] / res["batched_ms"]
        lines.append(res)
        print(json.dumps(res), flush=True)

    # one calculator call on the first shape: neighbour list + the eager model (energy, forces, stress)
    from dataclasses import dataclass

    from nequip_amd.integrations.torchsim import NequIPTorchSimCalc
    from nequip_amd.model import NequIPGNNModel

    @dataclass
    class State:
        positions: torch.Tensor
        row_vector_cell: torch.Tensor
        pbc: object
        atomic_numbers: torch.Tensor
        system_idx: torch.Tensor

    data = _batch(cases["256x64_periodic"], dev)
    N = data[K.POSITIONS_KEY].shape[0]
    z = torch.tensor(np.random.default_rng(1).choice([1, 8], size=N), device=dev)
    model = NequIPGNNModel(seed=0, model_dtype="float32", r_max=R_MAX, type_names=["H", "O"], num_layers=3, l_max=2,
                           parity=False, num_features=64, radial_mlp_depth=1, radial_mlp_width=128,
                           avg_num_neighbors=38.0).to(dev).eval()
    calc = NequIPTorchSimCalc(model, device=dev)
    state = State(data[K.POSITIONS_KEY], data[K.CELL_KEY], True, z, data[K.BATCH_KEY])
    res = {"case": "torchsim_forward_256x64", "frames": 256, "atoms": int(N)}
    for mode, env in (("per_frame", "1"), ("batched", "0")):
        os.environ["NQA_NL_PER_FRAME"] = env
        res[f"{mode}_nl_forward_ms"] = _time(lambda: calc(state), args.warmup, max(args.reps // 2, 3))
    os.environ.pop("NQA_NL_PER_FRAME")
    lines.append(res)
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
