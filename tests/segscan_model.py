"""The numpy model of CloSegScan (include/clo_segscan.h) the tests compare against, bit for bit. The ends are
expand_model's; clipped at n they bound every segment's rows, and every row below ct = min(total, n) finds its segment's
first row through np.searchsorted. A sum is the difference of two entries of the wrapped cumsum of the values in the sum
type; min and max come from a doubling scan that never reaches across a row's segment start. merge_steps says where the
ends fall in the merge of ends and rows the kernels tile by, for the tests that aim at tile edges."""
import numpy as np

from expand_model import FORMS, ends_of  # noqa: F401

OPS = ("sum", "min", "max")
NP = {"int": np.int32, "uint": np.uint32, "long": np.int64, "ulong": np.uint64}
# every legal (value, sum) pair: the sum type at least as wide as the value type
PAIRS = tuple((v, s) for v in NP for s in NP if np.dtype(NP[s]).itemsize >= np.dtype(NP[v]).itemsize)
LONG = 128   # rows: a segment above this is scanned on its own (a model of 36 M rows must not take 25 passes over them)


def identity(op, sum_type):
    dt = np.dtype(NP[sum_type])
    return dt.type(0) if op == "sum" else dt.type(np.iinfo(dt).max if op == "min" else np.iinfo(dt).min)


def segscan(op, form, counts_or_offsets, values, sum_type, inclusive=False, num_in=None):
    """(data, total): the ct = min(total, n) rows that are written, in the sum type, and the unclamped total."""
    ends, m = ends_of(form, counts_or_offsets, num_in)
    dt = np.dtype(NP[sum_type])
    v = np.asarray(values).astype(dt)                                          # C's cast: sign extension, or the same bits
    n = v.size
    total = int(ends[-1]) if m else 0
    ct = min(total, n)
    if ct == 0:
        return np.zeros(0, dt), total
    clipped = np.minimum(ends, np.uint64(n))
    i = np.arange(ct, dtype=np.int64)
    seg = np.searchsorted(clipped, i.astype(np.uint64), "right")              # the ends <= i: empty segments own no row
    start = np.concatenate((np.zeros(1, np.uint64), clipped))[seg].astype(np.int64)
    if op == "sum":
        u = np.dtype("u%d" % dt.itemsize)
        run = np.concatenate((np.zeros(1, u), np.cumsum(v.view(u), dtype=u)))  # wraps modulo 2^bits
        return (run[i + 1 if inclusive else i] - run[start]).view(dt), total
    f = np.minimum if op == "min" else np.maximum
    acc = v[:ct].copy()
    # inclusive: the few long segments one by one, the others by doubling, acc[i] covering [max(start, i - d + 1), i]
    # after the pass of distance d / 2; a row leaves once its whole segment is covered
    lo = np.concatenate((np.zeros(1, np.uint64), clipped[:-1])).astype(np.int64)
    hi = np.minimum(clipped.astype(np.int64), ct)
    long = hi - lo > LONG
    for r in np.flatnonzero(long):
        acc[lo[r]:hi[r]] = f.accumulate(v[lo[r]:hi[r]])
    idx = i[~long[seg]] if long.any() else i
    d = 1
    while idx.size:
        idx = idx[idx - d >= start[idx]]
        acc[idx] = f(acc[idx], acc[idx - d])
        d *= 2
    if inclusive:
        return acc, total
    out = np.full(ct, identity(op, sum_type), dt)
    inner = i > start
    out[inner] = acc[i[inner] - 1]
    return out, total


def merge_steps(form, counts_or_offsets, n, num_in=None):
    """(close, m, total): close[r] = the step of the merge of the m clipped ends with the n row indices at which segment
    r closes (an end goes before the row it equals), ascending; the merge has m + n steps."""
    ends, m = ends_of(form, counts_or_offsets, num_in)
    total = int(ends[-1]) if m else 0
    close = np.minimum(ends, np.uint64(n)).astype(np.int64) + np.arange(m, dtype=np.int64)
    return close, m, total
