"""Host-side planning for corpora of utterances of different lengths (``encode_many`` / ``decode_many``).

Pure Python/numpy: nothing here touches the GPU, so the grouping can be tested anywhere.
"""
import numpy as np


def batch_plan(lengths, max_batch):
    """Groups items for mixed-length batch calls.

    Sorts the items by length (stable, shortest first) and cuts the sorted order into consecutive groups of at most
    ``max_batch`` items, so every call pads its rows to a length close to their own.  Returns ``(perm, bounds, inv)``:
    ``perm[k]`` is the input index of the k-th item in sorted order, group g holds ``perm[bounds[g][0]:bounds[g][1]]``,
    and ``inv[i]`` is the sorted position of input item i (so ``sorted_results[inv[i]]`` is item i's result)."""
    max_batch = int(max_batch)
    if max_batch < 1:
        raise ValueError(f"max_batch must be at least 1, got {max_batch}")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    n = lengths.shape[0]
    perm = np.argsort(lengths, kind="stable")
    bounds = [(a, min(a + max_batch, n)) for a in range(0, n, max_batch)]
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n, dtype=np.int64)
    return perm, bounds, inv


def per_row(value, B, what):
    """None for a scalar (Python number, 0-d tensor or array), else the values as a 1-D float64 array of B entries."""
    if hasattr(value, "detach"):
        value = value.detach().cpu().numpy()
    arr = np.asarray(value, dtype=np.float64)
    if arr.ndim == 0:
        return None
    arr = arr.reshape(-1)
    if arr.shape[0] != B:
        raise RuntimeError(f"{what} has {arr.shape[0]} entries for a batch of {B}")
    return arr


def per_row_ints(value, B, what):
    """Like per_row, for counts: a 1-D int64 array (a scalar is repeated B times); non-integral values are an error."""
    arr = per_row(value, B, what)
    if arr is None:
        arr = np.full(B, float(np.asarray(value.detach().cpu() if hasattr(value, "detach") else value)), dtype=np.float64)
    if not np.all(np.isfinite(arr)) or not np.all(arr == np.round(arr)):
        raise RuntimeError(f"{what} must be whole numbers")
    return arr.astype(np.int64)
