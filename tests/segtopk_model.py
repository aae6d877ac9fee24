"""The numpy model of CloSegTopK (include/clo_segtopk.h) the tests compare against, bit for bit. The ends are
expand_model's; clipped at n they bound every segment's rows. The order keys are merge_model's (unsigned by bits, signed
with the sign bit flipped, floating point in IEEE total order), complemented for "largest". Per clipped segment the chosen
rows are np.argsort(x, kind="stable")[:k]; np.lexsort by (segment, x) is that stable argsort of every segment at once,
and row j of its result has the place j - (first row of its segment) inside its segment."""
import numpy as np

from expand_model import FORMS, ends_of  # noqa: F401
from merge_model import order_key
from segsort_model import KEY_NP  # noqa: F401

WHICH = ("smallest", "largest")


def selection_key(which, keys):
    """x: the unsigned number the rows are sorted by."""
    x = order_key(keys)
    return ~x if which == "largest" else x


def segtopk(which, form, counts_or_offsets, keys, k, num_in=None):
    """(idx, counts, total): idx[r, j], int64, is the global index of the j-th chosen row of segment r < m, -1 for the
    slots j >= counts[r] that the call does not write; counts[r] = min(k, len_r) as uint32; total is unclamped.
    keys_out[r, j] = keys[idx[r, j]], values_out[r, j] = values[idx[r, j]], and in the arg form values_out = idx."""
    assert which in WHICH
    keys = np.ascontiguousarray(keys)
    ends, m = ends_of(form, counts_or_offsets, num_in)
    n, k = keys.size, int(k)
    total = int(ends[-1]) if m else 0
    clipped = np.minimum(ends, np.uint64(n)).astype(np.int64)
    clipped = np.maximum.accumulate(clipped) if m else clipped               # (ascending ends are the precondition)
    starts = np.concatenate((np.zeros(1, np.int64), clipped[:-1])) if m else clipped
    rows = int(clipped[-1]) if m else 0
    seg = np.searchsorted(clipped, np.arange(rows, dtype=np.int64), "right")
    p = np.lexsort((selection_key(which, keys[:rows]), seg))                  # the last key is the primary one; stable
    place = np.arange(rows, dtype=np.int64) - starts[seg]                     # sorting by segment first leaves every segment on its rows
    idx = np.full((m, k), -1, np.int64)
    keep = place < k
    idx[seg[keep], place[keep]] = p[keep]
    counts = np.minimum(clipped - starts, k).astype(np.uint32)
    return idx, counts, total


def dense(idx, column, fill):
    """column[idx] where idx >= 0 and `fill` (an array of idx's shape, or a scalar) elsewhere: what an output prefilled
    with `fill` holds after the call."""
    out = np.empty(idx.shape, column.dtype)
    out[...] = fill
    out[idx >= 0] = column[idx[idx >= 0]]
    return out
