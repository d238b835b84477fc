"""Host-side grouping plan of encode_many / decode_many (no GPU)."""
import numpy as np
import pytest


@pytest.mark.parametrize("n,max_batch", [(0, 4), (1, 1), (7, 3), (70, 32), (256, 64), (100, 1000)])
def test_batch_plan_groups_sorts_and_restores_order(n, max_batch):
    from bvcodec import ragged
    rng = np.random.default_rng(n + max_batch)
    lengths = rng.integers(513, 22050 * 10, size=n)
    lengths[: n // 4] = 513                                    # ties: the sort is stable
    perm, bounds, inv = ragged.batch_plan(lengths.tolist(), max_batch)
    assert sorted(perm.tolist()) == list(range(n))
    assert [perm[k] for k in inv] == list(range(n))           # inverse permutation restores input order
    assert all(0 < e - a <= max_batch for a, e in bounds)
    assert [a for a, _ in bounds] == list(range(0, n, max_batch)) and (not bounds or bounds[-1][1] == n)
    assert len(bounds) == -(-n // max_batch)
    s = lengths[perm]
    assert (np.diff(s) >= 0).all()                            # sorted, hence sorted within every group
    for a, e in bounds:
        g = perm[a:e]
        assert (np.diff(lengths[g]) >= 0).all()
        ties = [i for i in g if lengths[i] == 513]
        assert ties == sorted(ties)


def test_batch_plan_rejects_empty_groups():
    from bvcodec import ragged
    with pytest.raises(ValueError):
        ragged.batch_plan([600, 700], 0)


def test_per_row_values():
    import torch
    from bvcodec import ragged
    assert ragged.per_row(3000, 4, "bitrate") is None
    assert ragged.per_row(torch.tensor(3000.0), 4, "bitrate") is None
    assert ragged.per_row(np.float32(700), 4, "bitrate") is None
    assert ragged.per_row([1, 2, 3], 3, "bitrate").tolist() == [1.0, 2.0, 3.0]
    assert ragged.per_row(torch.tensor([5, 6]), 2, "bitrate").tolist() == [5.0, 6.0]
    with pytest.raises(RuntimeError, match="entries for a batch"):
        ragged.per_row([1, 2], 3, "bitrate")
    assert ragged.per_row_ints(600, 3, "lengths").tolist() == [600, 600, 600]
    assert ragged.per_row_ints(torch.tensor([600, 700]), 2, "lengths").dtype == np.int64
    with pytest.raises(RuntimeError, match="whole numbers"):
        ragged.per_row_ints([600.5, 700], 2, "lengths")
