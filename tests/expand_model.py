"""The numpy model of CloExpand (include/clo_expand.h) the tests compare against, bit for bit. The inclusive ends come
from np.cumsum in uint64 (counts) or from offsets[1:] - offsets[0] (offsets); the segment of row j is
np.searchsorted(ends, j, "right"), the number of ends <= j, so that empty segments own no row."""
import numpy as np

FORMS = ("counts", "offsets")


def ends_of(form, counts_or_offsets, num_in=None):
    """(ends, m): the inclusive ends of the first m = min(numel_in, num_in) segments, uint64."""
    c = np.asarray(counts_or_offsets).astype(np.uint64)
    m_h = c.size - 1 if form == "offsets" else c.size
    m = m_h if num_in is None else min(m_h, int(num_in))
    if form == "offsets":
        return c[1:m + 1] - c[0], m
    return np.cumsum(c[:m], dtype=np.uint64), m


def expand(form, counts_or_offsets, capacity, num_in=None):
    """(seg, rank, total): the segment id and the rank within its segment of the rows [0, min(total, capacity)), both
    uint32, and the unclamped total."""
    ends, m = ends_of(form, counts_or_offsets, num_in)
    total = int(ends[-1]) if m else 0
    rows = min(total, int(capacity))
    j = np.arange(rows, dtype=np.uint64)
    seg = np.searchsorted(ends, j, "right")
    starts = np.concatenate((np.zeros(1, np.uint64), ends))[seg]
    return seg.astype(np.uint32), (j - starts).astype(np.uint32), total
