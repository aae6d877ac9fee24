"""The numpy model of CloSelect (include/clo_select.h) the tests compare against, bit for bit. The mask comes from the
flags (kept iff the byte is not 0) or from the order keys of tests/merge_model.py (unsigned integers whose numeric order
is the by-key sort's order, equal iff the keys' bits are equal) compared with the threshold's order key; the rows are
keys[mask], or concatenate(keys[mask], keys[~mask]) for a partition. tests/test_select_cpu.py checks this model against
a plain Python loop."""
import numpy as np

from merge_model import order_key

OPS = ("select", "partition")
PREDS = ("flagged", "lt", "le", "gt", "ge", "eq", "ne")
_CMP = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal, "eq": np.equal, "ne": np.not_equal}


def keep_mask(pred, keys, flags_or_threshold):
    """Which elements are kept. flagged: flags_or_threshold is the flag bytes (keys may be None); else one key."""
    if pred == "flagged":
        return np.ascontiguousarray(flags_or_threshold).view(np.uint8) != 0
    keys = np.ascontiguousarray(keys)
    t = order_key(np.array([flags_or_threshold], dtype=keys.dtype).reshape(1))[0]
    return _CMP[pred](order_key(keys), t)


def select(op, pred, keys, flags_or_threshold):
    """(p, k): for every row written, the index of its element as uint32 — the k kept ones in input order, then for a
    partition the rejected ones in input order — and k. keys_out is keys[p], values_out values[p] or p itself."""
    mask = keep_mask(pred, keys, flags_or_threshold)
    i = np.arange(mask.size, dtype=np.uint32)
    kept = i[mask]
    return (np.concatenate((kept, i[~mask])) if op == "partition" else kept), int(kept.size)
