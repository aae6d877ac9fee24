"""The numpy model of CloTopK (include/clo_topk.h) the tests compare against, bit for bit. The keys become the order keys
of tests/merge_model.py (unsigned integers whose numeric order is the by-key sort's order, equal iff the keys' bits are
equal), complemented for "largest"; numpy's stable argsort of those is the sort the contract names, its first m =
min(k, numel) entries are the chosen elements, and for "input" order they are sorted by index. tests/test_topk_cpu.py
checks this model against a plain Python loop."""
import numpy as np

from merge_model import order_key

WHICH = ("smallest", "largest")
ORDERS = ("input", "sorted")


def topk(which, order, keys, k):
    """(p, kth): for every row written, the index of its element as uint32, and the key of the m-th chosen element of
    the sort as a 1-element array (empty when m == 0). keys_out is keys[p], values_out values[p] or p itself."""
    keys = np.ascontiguousarray(keys)
    x = order_key(keys)
    if which == "largest":
        x = ~x
    m = min(int(k), keys.size)
    p = np.argsort(x, kind="stable")[:m]
    kth = keys[p[m - 1:m]].copy()
    if order == "input":
        p = np.sort(p)
    return p.astype(np.uint32), kth
