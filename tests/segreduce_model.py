"""The numpy model of CloSegReduce (include/clo_segreduce.h) the tests compare against, bit for bit. The ends are
expand_model's; clipped at n they bound every segment's rows. A sum is the difference of two entries of the wrapped
cumsum of the values in the sum type; min and max come from np.minimum / np.maximum.reduceat over the segments that
have a row, the identity standing in the others."""
import numpy as np

from expand_model import FORMS, ends_of  # noqa: F401

OPS = ("sum", "min", "max")
NP = {"int": np.int32, "uint": np.uint32, "long": np.int64, "ulong": np.uint64}
# every legal (value, sum) pair: the sum type at least as wide as the value type
PAIRS = tuple((v, s) for v in NP for s in NP if np.dtype(NP[s]).itemsize >= np.dtype(NP[v]).itemsize)


def identity(op, sum_type):
    dt = np.dtype(NP[sum_type])
    return dt.type(0) if op == "sum" else dt.type(np.iinfo(dt).max if op == "min" else np.iinfo(dt).min)


def segreduce(op, form, counts_or_offsets, values, sum_type, num_in=None):
    """(aggr, total): the m aggregates in the sum type, and the unclamped total."""
    ends, m = ends_of(form, counts_or_offsets, num_in)
    dt = np.dtype(NP[sum_type])
    v = np.asarray(values).astype(dt)                                          # C's cast: sign extension, or the same bits
    n = v.size
    total = int(ends[-1]) if m else 0
    hi = np.minimum(ends, np.uint64(n)).astype(np.int64)                       # the clipped ends
    lo = np.concatenate((np.zeros(1, np.int64), hi[:-1])) if m else hi
    if op == "sum":
        u = np.dtype("u%d" % dt.itemsize)
        run = np.concatenate((np.zeros(1, u), np.cumsum(v.view(u), dtype=u)))  # wraps modulo 2^bits
        return (run[hi] - run[lo]).view(dt), total
    out = np.full(m, identity(op, sum_type), dt)
    full = hi > lo
    if full.any():
        # reduceat over [lo_k, lo_(k+1)) of the segments that have a row: they tile [lo_first, hi_last) without a gap
        f = np.minimum.reduceat if op == "min" else np.maximum.reduceat
        last = int(hi[full][-1])
        out[full] = f(v[:last], lo[full])
    return out, total
