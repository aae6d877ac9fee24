"""The numpy model of CloSearch (include/clo_search.h) the tests compare against, bit for bit: both arrays are mapped to
unsigned integers whose numeric order is the library's key order (merge_model.order_key: unsigned keys by their bits,
signed keys with the sign bit flipped, half / float / double keys in IEEE total order), and np.searchsorted of those is
the answer. tests/test_search_cpu.py checks this model against a linear count over Python integers."""
import numpy as np

from merge_model import order_key, sort_keys  # noqa: F401  (sort_keys: what a test feeds as a sorted input)


def search(haystack, needles, upper=False):
    """For every needle, how many haystack keys are < it (upper: <= it), as uint32. haystack ascending in the
    library's order."""
    haystack, needles = np.ascontiguousarray(haystack), np.ascontiguousarray(needles)
    assert haystack.dtype == needles.dtype and haystack.ndim == 1 and needles.ndim == 1
    return np.searchsorted(order_key(haystack), order_key(needles), side="right" if upper else "left").astype(np.uint32)
