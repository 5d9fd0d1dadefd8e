"""``MetricsManager.compute()`` under ``torch.distributed`` (CPU, gloo, world size 2, after ``tests/test_ddp_gloo.py``): every
rank accumulates batches of its own; ``compute()`` all-reduces the epoch state first (sums and counts by sum, maxima by max:
the ``dist_reduce_fx`` of the reference's metric states) and must equal ``tests/metrics_restatement.py`` on the union."""

import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
TYPES = ["H", "O", "Cs"]
ENTRIES = [{"name": "e", "field": "total_energy", "kind": "rmse", "per_atom": True, "coeff": 1.0},
           {"name": "f", "field": "forces", "kind": "mse", "per_type": True, "per_type_coeffs": [5.0, 1.0, 0.5], "coeff": 3.0},
           {"name": "fmax", "field": "forces", "kind": "max_ae", "per_type": True},
           {"name": "s", "field": "stress", "kind": "mae", "ignore_nan": True}]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _batches(rank):
    """Two batches per rank, of different sizes; ``Cs`` occurs on rank 1 only, rank 0 has a frame without stress labels."""
    out = []
    for i, sizes in enumerate([[3, 5], [4, 2, 6]] if rank == 0 else [[7], [2, 9]]):
        g = torch.Generator().manual_seed(10 * rank + i)
        n, b = sum(sizes), len(sizes)
        preds = {"total_energy": torch.randn(b, 1, generator=g), "forces": torch.randn(n, 3, generator=g),
                 "stress": torch.randn(b, 3, 3, generator=g), "num_atoms": torch.tensor(sizes),
                 "atom_types": torch.randint(0, 2 + rank, (n,), generator=g)}
        target = {"total_energy": torch.randn(b, 1, generator=g, dtype=torch.float64),
                  "forces": torch.randn(n, 3, generator=g, dtype=torch.float64),
                  "stress": torch.randn(b, 3, 3, generator=g, dtype=torch.float64), "num_atoms": torch.tensor(sizes)}
        if rank == 0:
            target["stress"][0] = float("nan")
        out.append((preds, target))
    return out


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from nequip_amd.data import PerAtomModifier
    from nequip_amd.train import (MaximumAbsoluteError, MeanAbsoluteError, MeanSquaredError, MetricsManager,
                                  RootMeanSquaredError)

    m = MetricsManager([
        {"name": "e", "field": PerAtomModifier("total_energy"), "metric": RootMeanSquaredError(), "coeff": 1.0},
        {"name": "f", "field": "forces", "metric": MeanSquaredError(), "per_type": True,
         "per_type_coeffs": {"H": 5.0, "O": 1.0, "Cs": 0.5}, "coeff": 3.0},
        {"name": "fmax", "field": "forces", "metric": MaximumAbsoluteError(), "per_type": True},
        {"name": "s", "field": "stress", "metric": MeanAbsoluteError(), "ignore_nan": True}], type_names=TYPES)
    for preds, target in _batches(rank):
        m(preds, target)
    got = {k: v.clone() for k, v in m.compute().items()}
    torch.save(got, os.path.join(out_dir, f"rank{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


def test_compute_all_reduces_the_epoch_state_gloo(tmp_path):
    import metrics_restatement as mr

    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    ref = mr.evaluate(ENTRIES, _batches(0) + _batches(1), TYPES, epoch=True)
    for rank in range(world):
        got = torch.load(os.path.join(str(tmp_path), f"rank{rank}.pt"))
        assert list(got) == list(ref)
        for k in ref:
            torch.testing.assert_close(got[k], torch.as_tensor(ref[k], dtype=torch.float64), rtol=1e-10, atol=0.0,
                                       equal_nan=True, msg=lambda s, k=k: f"rank {rank} {k}: {s}")
    assert not torch.isnan(ref["f_Cs"])  # a type only one rank has seen
