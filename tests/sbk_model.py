"""Reference model of CloScanByKey (include/clo_scan_by_key.h) in numpy, for the CPU and GPU tests: every element's
running sum / min / max within its run (a maximal stretch of consecutive elements whose keys have the same bytes),
inclusive or exclusive. Everything is integer arithmetic in the sum dtype, so the tests compare bit for bit.
sbk_loop() is the plain Python loop the vectorised form is checked against (tests/test_scan_by_key_cpu.py)."""
import numpy as np

_BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def identity(op, sum_dtype):
    """What the exclusive form holds at a run's first element."""
    dt = np.dtype(sum_dtype)
    if op == "sum":
        return dt.type(0)
    return dt.type(np.iinfo(dt).max if op == "min" else np.iinfo(dt).min)


def heads_of(keys):
    """Boolean: element i starts a run (keys compared by their bits)."""
    bits = keys.view(_BITS[keys.dtype.itemsize])
    return np.concatenate(([True], bits[1:] != bits[:-1])) if keys.size else np.zeros(0, bool)


def _ordered_bits32(v):
    """32-bit values as uint64 numbers whose unsigned order is the values' order."""
    if v.dtype.kind == "i":
        return (v.view(np.uint32) ^ np.uint32(0x80000000)).astype(np.uint64)
    return v.astype(np.uint64)


def sbk(keys, values=None, op="sum", sum_dtype=np.uint32, inclusive=False):
    """out[i] for every i. values None: every value is 1 (op "sum" only)."""
    dt = np.dtype(sum_dtype)
    n = keys.size
    if n == 0:
        return np.zeros(0, dt)
    head = heads_of(keys)
    starts = np.flatnonzero(head)
    v = np.ones(n, dt) if values is None else values.astype(dt)
    with np.errstate(over="ignore"):
        if op == "sum":
            c = np.cumsum(v, dtype=dt)
            lens = np.diff(np.append(starts, n))
            base = np.where(starts > 0, c[starts - 1], dt.type(0)).astype(dt)
            incl = (c - np.repeat(base, lens)).astype(dt)           # wraps in the sum dtype
            return incl if inclusive else (incl - v).astype(dt)
        if dt.itemsize == 4:
            # (run number << 32) | order-preserving bits of the value: run numbers never decrease, so the running
            # maximum of the packed words is a segmented running maximum (the value bits complemented for min)
            run = (np.cumsum(head) - 1).astype(np.uint64)
            b = _ordered_bits32(v)
            if op == "min":
                b = b ^ np.uint64(0xffffffff)
            packed = np.maximum.accumulate((run << np.uint64(32)) | b)
            b = (packed & np.uint64(0xffffffff))
            if op == "min":
                b = b ^ np.uint64(0xffffffff)
            b = b.astype(np.uint32)
            incl = (b ^ np.uint32(0x80000000)).view(np.int32) if dt.kind == "i" else b
            incl = incl.astype(dt)
        else:
            f = np.minimum if op == "min" else np.maximum
            incl = np.empty(n, dt)
            ends = np.append(starts[1:], n)
            for b0, e0 in zip(starts, ends):                        # 64-bit sums: run by run
                incl[b0:e0] = f.accumulate(v[b0:e0])
    if inclusive:
        return incl
    excl = np.empty(n, dt)
    excl[1:] = incl[:-1]
    excl[head] = identity(op, dt)
    return excl


def sbk_loop(keys, values=None, op="sum", sum_dtype=np.uint32, inclusive=False):
    """The definition, element by element in Python integers."""
    dt = np.dtype(sum_dtype)
    n = keys.size
    bits = 8 * dt.itemsize
    mask = (1 << bits) - 1
    bk = keys.view(_BITS[keys.dtype.itemsize])
    signed = dt.kind == "i"

    def wrap(x):
        x &= mask
        return x - (1 << bits) if signed and x >> (bits - 1) else x

    ident = int(identity(op, dt))
    out = []
    acc = ident
    for i in range(n):
        x = wrap(1 if values is None else int(values[i]))           # the C cast (sum type) value
        head = i == 0 or bk[i] != bk[i - 1]
        before = ident if head else acc
        if head:
            acc = x
        elif op == "sum":
            acc = wrap(acc + x)
        elif op == "min":
            acc = min(acc, x)
        else:
            acc = max(acc, x)
        out.append(acc if inclusive else before)
    return np.array([o & mask for o in out], dtype=_BITS[dt.itemsize]).view(dt) if n else np.zeros(0, dt)
