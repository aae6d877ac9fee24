"""The numpy model of CloSegArg (include/clo_segarg.h) the tests compare against, bit for bit. The ends are
expand_model's; clipped at n they bound every segment's rows. The order is merge_model's order_key, complemented for
argmax. The rows that some segment owns are sorted, stably, by (segment, key, +index or -index); the first entry of every
segment that has a row is its winner. Whether a segment has a row comes from its clipped ends."""
import numpy as np

from expand_model import FORMS, ends_of  # noqa: F401
from merge_model import order_key

OPS = ("argmin", "argmax")
TIES = ("first", "last")
NONE = 0xffffffff
NP = {"int": np.int32, "uint": np.uint32, "long": np.int64, "ulong": np.uint64, "float": np.float32, "double": np.float64}


def none_value(op, value_type):
    """val_out of a segment without a row: the value that comes last in the order for argmin, first for argmax."""
    dt = np.dtype(NP[value_type])
    if dt.kind == "f":
        u = np.dtype("u%d" % dt.itemsize)
        ones = np.iinfo(u).max
        return np.array([ones >> 1 if op == "argmin" else ones], u).view(dt)[0]
    return dt.type(np.iinfo(dt).max if op == "argmin" else np.iinfo(dt).min)


def segarg(op, tie, form, counts_or_offsets, values, num_in=None):
    """(idx, vals, total): the m row indices as uint32 (NONE without a row), the m values with their original bits, and
    the unclamped total."""
    assert op in OPS and tie in TIES
    ends, m = ends_of(form, counts_or_offsets, num_in)
    v = np.ascontiguousarray(values)
    n = v.size
    total = int(ends[-1]) if m else 0
    hi = np.minimum(ends, np.uint64(n)).astype(np.int64)                       # the clipped ends
    lo = np.concatenate((np.zeros(1, np.int64), hi[:-1])) if m else hi
    idx = np.full(m, NONE, np.uint32)
    vals = np.full(m, none_value(op, {np.dtype(t): k for k, t in NP.items()}[v.dtype]), v.dtype)
    full = hi > lo
    if full.any():
        # the segments that have a row tile [first, last) without a gap: seg[i - first] = the segment that owns row i
        first, last = int(lo[full][0]), int(hi[full][-1])
        lengths = (hi - lo)[full]
        seg = np.repeat(np.flatnonzero(full), lengths)
        x = order_key(v[first:last])
        if op == "argmax":
            x = ~x
        i = np.arange(first, last, dtype=np.int64)
        p = np.lexsort((i if tie == "first" else -i, x, seg))                  # the last key is the primary one
        win = i[p[np.concatenate(([0], np.cumsum(lengths)[:-1]))]]
        idx[full] = win.astype(np.uint32)
        vals[full] = v[win]
    return idx, vals, total
