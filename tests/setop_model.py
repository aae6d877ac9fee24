"""The numpy model of CloSetOp (include/clo_setop.h) the tests compare against, bit for bit, built from the
definition: with the order keys of merge_model.order_key, np.searchsorted gives every element its rank in its run of
equal keys (r for A, s for B) and the length of that run in A (m) and in B (n); the table of clo_setop.h turns those
into a keep flag per element, and the kept subsequence of merge_model.merge is the result. tests/test_setop_cpu.py
checks this model against a two-pointer loop over Python integers, collections.Counter and numpy's set routines."""
import numpy as np

from merge_model import merge, order_key

OPS = ("union", "intersection", "difference", "symmetric_difference")   # in the thin ABI's numbering


def capacity(op, na, nb):
    """The elements the outputs must hold (clo_setop_get_max_numel_out)."""
    return {"union": na + nb, "symmetric_difference": na + nb, "intersection": min(na, nb), "difference": na}[op]


def keep_flags(op, keys_a, keys_b):
    """(keep_a, keep_b): which elements of A and of B the op keeps."""
    oa, ob = order_key(keys_a), order_key(keys_b)
    r = np.arange(oa.size) - np.searchsorted(oa, oa, "left")                    # rank in A's run
    s = np.arange(ob.size) - np.searchsorted(ob, ob, "left")
    n_of_a = np.searchsorted(ob, oa, "right") - np.searchsorted(ob, oa, "left")   # copies in B of each key of A
    m_of_b = np.searchsorted(oa, ob, "right") - np.searchsorted(oa, ob, "left")
    none = np.zeros(ob.size, dtype=bool)
    if op == "union":
        return np.ones(oa.size, dtype=bool), s >= m_of_b
    if op == "intersection":
        return r < n_of_a, none
    if op == "difference":
        return r >= n_of_a, none
    assert op == "symmetric_difference"
    return r >= n_of_a, s >= m_of_b


def setop(op, keys_a, keys_b):
    """(keys_out, p): the kept keys in merge order with their original bits, and for each the index of its element in
    A || B (i for A[i], len(A) + i for B[i]) as uint32."""
    merged, p = merge(keys_a, keys_b)
    keep = np.concatenate(keep_flags(op, np.ascontiguousarray(keys_a), np.ascontiguousarray(keys_b)))[p]
    return merged[keep], p[keep]
