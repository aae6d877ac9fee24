"""The numpy model of CloHistogram (include/clo_histogram.h) the tests compare against, bit for bit. d = key - lower
is taken over the integers (in int64 for keys of up to 4 bytes, where nothing can wrap; for 8-byte keys d >= 0 is
decided by comparing in the key type and d is computed only where it holds), then the two conditions d >= 0 and
(d >> shift) < num_bins are tested; the sums are np.add.at in the sum type, which wraps as the C cast and the
device's addition do. tests/test_histogram_cpu.py checks this model against np.bincount and a loop over Python ints."""
import numpy as np


def bins_of(keys, lower, shift, num_bins):
    """(counted, bin): a boolean mask of the counted elements and the bins of those."""
    keys = np.asarray(keys)
    assert keys.dtype.kind in "iu"
    if keys.dtype.itemsize == 8:
        # d >= 0 is the comparison in the key type itself (lower is a value of that type). Where it holds, d lies in
        # [0, 2^64) and the subtraction modulo 2^64 gives exactly d; elsewhere the difference is not looked at.
        ge = keys >= np.array(int(lower), dtype=keys.dtype)
        d = keys.view(np.uint64) - np.array(int(lower) & (2 ** 64 - 1), dtype=np.uint64)
        counted = ge & ((d >> np.uint64(shift)) < np.uint64(num_bins))
        b = np.where(counted, d >> np.uint64(shift), np.uint64(0)).astype(np.int64)   # (num_bins < 2^32)
    else:
        d = keys.astype(np.int64) - np.int64(int(lower))   # |d| < 2^33
        counted = (d >= 0) & ((d >> shift) < num_bins)
        b = np.where(counted, d >> shift, 0)
    return counted, b[counted]


def histogram(keys, values, sum_dtype, lower=0, shift=0, num_bins=1, onto=None):
    """hist_out of a call; onto: what hist_out held before, for an accumulating call."""
    sum_dtype = np.dtype(sum_dtype)
    counted, b = bins_of(keys, lower, shift, num_bins)
    out = np.zeros(num_bins, sum_dtype) if onto is None else np.array(onto, dtype=sum_dtype, copy=True)
    assert out.size == num_bins
    with np.errstate(over="ignore"):
        if values is None:
            x = np.ones(b.size, sum_dtype)
        else:
            x = np.asarray(values)[counted].astype(sum_dtype)   # the C cast: sign- or zero-extends, keeps the low bits
        np.add.at(out, b, x)
    return out
