"""The numpy model of CloSegSort (include/clo_segsort.h) the tests compare against, bit for bit. The ends are
expand_model's; clipped at n they bound every segment's rows. The order keys are merge_model's (unsigned by bits, signed
with the sign bit flipped, floating point in IEEE total order). Row i < min(total, n) lies in segment seg(i) = the number
of clipped ends <= i, and np.lexsort by (segment, order key) is stable, so that equal keys of a segment keep their input
order: its result is the permutation p, output row j holding input row p[j]."""
import numpy as np

from expand_model import FORMS, ends_of  # noqa: F401
from merge_model import order_key

KEY_NP = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
          "long": np.int64, "ulong": np.uint64, "half": np.float16, "float": np.float32, "double": np.float64}


def segsort(form, counts_or_offsets, keys, num_in=None):
    """(p, total): p[j], uint32, is the global index of the input row that output row j holds, for the rows j <
    min(total, n) that are written; total is unclamped. keys_out[:p.size] = keys[p], values_out[:p.size] = values[p],
    and in the arg form values_out[:p.size] = p."""
    keys = np.ascontiguousarray(keys)
    ends, m = ends_of(form, counts_or_offsets, num_in)
    n = keys.size
    total = int(ends[-1]) if m else 0
    rows = min(total, n)
    clipped = np.minimum(ends, np.uint64(n))
    seg = np.searchsorted(clipped, np.arange(rows, dtype=np.uint64), "right")
    p = np.lexsort((order_key(keys[:rows]), seg))                             # the last key is the primary one; stable
    return p.astype(np.uint32), total
