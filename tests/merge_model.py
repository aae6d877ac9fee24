"""The numpy model of CloMerge (include/clo_merge.h) the tests compare against, bit for bit. The keys of the
concatenation A || B are mapped to unsigned integers whose order is the merge's order (unsigned keys by their bits,
signed keys with the sign bit flipped, half / float / double keys in IEEE total order: negative numbers with every bit
flipped, the others with the sign bit flipped), and numpy's stable argsort of those is the permutation p: ties keep the
order of the concatenation, so equal keys of A come before those of B. tests/test_merge_cpu.py checks this model against
a two-pointer loop over Python integers and against np.sort(kind="stable")."""
import numpy as np

_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def order_key(keys):
    """The keys as unsigned integers of the same width whose numeric order is the merge's order; equal iff the keys'
    bits are equal."""
    keys = np.ascontiguousarray(keys)
    ut = np.dtype(_U[keys.dtype.itemsize])
    bits = keys.view(ut)
    sign = ut.type(1 << (8 * ut.itemsize - 1))
    if keys.dtype.kind == "u":
        return bits.copy()
    if keys.dtype.kind == "i":
        return bits ^ sign
    assert keys.dtype.kind == "f"
    return np.where((bits & sign) != 0, ~bits, bits ^ sign)


def merge(keys_a, keys_b):
    """(keys_out, p): the merged keys with their original bits, and for every output position the index of its
    element in A || B (i for A[i], len(A) + i for B[i]) as uint32."""
    keys_a, keys_b = np.ascontiguousarray(keys_a), np.ascontiguousarray(keys_b)
    assert keys_a.dtype == keys_b.dtype and keys_a.ndim == 1 and keys_b.ndim == 1
    cat = np.concatenate((keys_a, keys_b))
    p = np.argsort(order_key(cat), kind="stable")
    return cat[p], p.astype(np.uint32)


def sort_keys(keys):
    """keys in the merge's order (what a test feeds as a sorted input), stable."""
    keys = np.ascontiguousarray(keys)
    return keys[np.argsort(order_key(keys), kind="stable")]
