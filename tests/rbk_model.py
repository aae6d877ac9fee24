"""Reference model of CloReduceByKey (include/clo_reduce.h) in numpy, for the CPU and GPU tests: one row per maximal
stretch of consecutive elements whose keys have the same bytes. Everything is integer arithmetic on bytes, so the
tests compare bit for bit."""
import numpy as np

_BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def rbk(keys, values=None, op="sum", sum_dtype=np.uint32):
    """(keys_out, aggr_out, m). values None: every value is 1. `dtype=` in reduceat matters: without it numpy widens
    32-bit sums to 64 bits and the wrap-around cases compare wrongly."""
    n = keys.size
    if n == 0:
        return keys[:0], np.zeros(0, sum_dtype), 0
    bits = keys.view(_BITS[keys.dtype.itemsize])
    heads = np.flatnonzero(np.concatenate(([True], bits[1:] != bits[:-1])))
    v = np.ones(n, sum_dtype) if values is None else values.astype(sum_dtype)
    f = {"sum": np.add, "min": np.minimum, "max": np.maximum}[op]
    with np.errstate(over="ignore"):
        return keys[heads], f.reduceat(v, heads, dtype=sum_dtype), heads.size
