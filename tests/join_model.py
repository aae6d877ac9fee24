"""The numpy model of CloJoin (include/clo_join.h) the tests compare against, bit for bit. Both inputs are mapped to the
unsigned integers of merge_model.order_key, whose order is the join's order and which are equal iff the keys' bits are.
np.searchsorted gives every row its run's bounds in the other array; the rows are then built group by group in
ascending key order: for a key in both inputs the m * n pairs ordered by A's row, then B's; for a key of A alone its rows
with NONE (left, full); for a key of B alone its rows with NONE (right, full). tests/test_join_cpu.py checks this model
against a two-pointer loop over Python integers and, for inner joins of duplicate-free inputs, against np.intersect1d."""
import numpy as np

from merge_model import order_key

KINDS = ("inner", "left", "right", "full")
NONE = 0xFFFFFFFF


def max_rows(kind, na, nb):
    """The largest K of a join of these sizes: one key everywhere, or nothing shared."""
    alone = (na if kind in ("left", "full") else 0) + (nb if kind in ("right", "full") else 0)
    return max(na * nb, alone)


def join(kind, keys_a, keys_b, capacity=None):
    """(idx_a, idx_b, keys, K): the first min(K, capacity) rows (all of them with capacity None) as uint32, uint32 and
    the keys' dtype, and the row count K of the whole join as a Python int."""
    assert kind in KINDS
    a, b = np.ascontiguousarray(keys_a), np.ascontiguousarray(keys_b)
    assert a.dtype == b.dtype and a.ndim == 1 and b.ndim == 1
    oa, ob = order_key(a), order_key(b)
    emits_a, emits_b = kind in ("left", "full"), kind in ("right", "full")
    # per row of A: its run in B; per row of B: whether A has its key
    lb = np.searchsorted(ob, oa, side="left").astype(np.int64)
    n = np.searchsorted(ob, oa, side="right").astype(np.int64) - lb
    b_alone = np.searchsorted(oa, ob, side="left") == np.searchsorted(oa, ob, side="right")
    rows_a = np.where(n > 0, n, 1 if emits_a else 0)
    rows_b = np.where(b_alone, 1, 0) if emits_b else np.zeros(b.size, np.int64)
    # the emitters in merge order (equal keys: A first, but a B row that emits has no equal key in A)
    order = np.argsort(np.concatenate((oa, ob)), kind="stable")
    rows = np.concatenate((rows_a, rows_b)).astype(np.int64)[order]
    K = int(rows.sum())                    # < 2^63: numel_a + numel_b < 2^32
    lim = K if capacity is None else min(K, capacity)
    starts = np.cumsum(rows) - rows
    take = np.flatnonzero((rows > 0) & (starts < lim))                 # the emitters that reach below lim
    cnt = np.minimum(rows[take], lim - starts[take])
    who = np.repeat(take, cnt)
    rank = np.arange(who.size, dtype=np.int64) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    src = order[who]                       # index in A || B
    from_a = src < a.size
    ia = np.where(from_a, src, NONE).astype(np.uint32)
    src_a = np.where(from_a, src, 0)
    src_b = np.where(from_a, 0, src - a.size)
    matched = from_a & (n[src_a] > 0) if a.size else np.zeros(who.size, bool)
    ib = np.where(from_a, np.where(matched, (lb[src_a] if a.size else 0) + rank, NONE), src_b).astype(np.uint32)
    keys = np.empty(who.size, a.dtype)
    if a.size:
        keys[from_a] = a[src_a[from_a]]
    if b.size:
        keys[~from_a] = b[src_b[~from_a]]
    assert ia.size == lim
    return ia, ib, keys, K
