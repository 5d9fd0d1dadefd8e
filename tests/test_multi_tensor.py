"""Host side of the multi-tensor chunk layout (``nequip_amd/train/_multi_tensor.py``) without a GPU: the chunk map against rows
written down by hand, and the rewrite in place of the tables."""
import pytest
import torch

from nequip_amd.train import _multi_tensor as mt


@pytest.mark.parametrize("c", [1024, 4096])
def test_chunk_map_is_the_rows_one_writes_down_by_hand(c):
    rows, chunk0 = mt.chunk_map((0, 1, c - 1, c, c + 1, 2 * c + 3), c)
    assert rows.dtype == torch.int64 and rows.device.type == "cpu"
    assert rows.tolist() == [
        # (tensor 0 has no elements: an entry in the table, no chunk)
        [0, 1],
        [0, 2],
        [0, 3],
        [0, 4], [c, 4],
        [0, 5], [c, 5], [2 * c, 5],
    ]
    assert chunk0 == [0, 0, 1, 2, 3, 5]
    assert mt.n_chunks((0, 1, c - 1, c, c + 1, 2 * c + 3), c) == 8


def test_no_tensors_and_empty_tensors_give_an_empty_map():
    for numels in ((), (0,), (0, 0)):
        rows, chunk0 = mt.chunk_map(numels, 1024)
        assert rows.shape == (0, 2) and rows.dtype == torch.int64 and chunk0 == [0] * len(numels)


def test_rewrite_with_fewer_tensors_is_in_place_and_updates_the_counts():
    c, device = 1024, torch.device("cpu")
    numels = [c + 1, 3, 0, 2 * c]
    t = mt.ChunkTables(device, c, len(numels), mt.n_chunks(numels, c), words=3)
    assert t.capacity == 5 and t.tensors.shape == (4, 3) and t.chunks.shape == (5, 2)
    ptrs = (t.tensors.data_ptr(), t.chunks.data_ptr(), t.counts.data_ptr())
    t.write("first", numels, [[100 + i, n, 7 | (i << 32)] for i, n in enumerate(numels)], with_chunk0=False)
    assert t.key == "first" and t.counts.tolist() == [5, 4]
    assert t.tensors.tolist() == [[100 + i, n, 7 | (i << 32)] for i, n in enumerate(numels)]
    assert t.chunks.tolist() == [[0, 0], [c, 0], [0, 1], [0, 3], [c, 3]]

    assert t.fits(device, [3, c]) and not t.fits(device, [1] * 5) and not t.fits(device, [6 * c])
    assert not t.fits(torch.device("meta"), [3, c])
    t.write("second", [3, c], [[5, 3, 0], [6, c, 1]])
    assert (t.tensors.data_ptr(), t.chunks.data_ptr(), t.counts.data_ptr()) == ptrs
    assert t.key == "second" and t.counts.tolist() == [2, 2]
    assert t.tensors[:2].tolist() == [[5, 3, 0], [6, c, 1]] and t.chunks[:2].tolist() == [[0, 0], [0, 1]]
    # what lies past the counts is left as it was: the kernels do not read it
    assert t.tensors[2:].tolist() == [[102, 0, 7 | (2 << 32)], [103, 2 * c, 7 | (3 << 32)]]

    t.write("third", [c + 2, 1], [[8, c + 2], [9, 1]], with_chunk0=True)
    assert t.tensors[:2].tolist() == [[8, c + 2, 0], [9, 1, 2]] and t.counts.tolist() == [3, 2]
    with pytest.raises(AssertionError):
        t.write("too many", [c] * 6, [[0, 0, 0]] * 6)
