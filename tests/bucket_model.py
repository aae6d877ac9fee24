"""The numpy model of CloBucket (include/clo_bucket.h) the tests compare against, bit for bit: the bins are those of
hist_model.bins_of (CloHistogram's mapping), the rest counts as bin num_bins, and the rows leave in the order of a
stable argsort by that number. tests/test_bucket_cpu.py checks this model against a plain loop over Python integers."""
import numpy as np

from hist_model import bins_of

COUNT_NP = {"uint": np.uint32, "ulong": np.uint64}


def bin_or_rest(keys, lower, shift, num_bins):
    """The bin of every row, num_bins for the rows of the rest."""
    keys = np.asarray(keys)
    counted, b = bins_of(keys, lower, shift, num_bins)
    out = np.full(keys.size, num_bins, np.int64)
    out[counted] = b
    return out


def bucket(keys, values=None, lower=0, shift=0, num_bins=1, count_type="uint"):
    """(keys_out, values_out, perm, offsets): values_out is None without values; perm (uint32) is what the arg form
    writes; offsets has num_bins + 1 entries of the count type."""
    keys = np.asarray(keys)
    b = bin_or_rest(keys, lower, shift, num_bins)
    perm = np.argsort(b.astype(np.uint16), kind="stable")   # (num_bins <= 65535; numpy sorts 16-bit integers by radix)
    counts = np.bincount(b[b < num_bins], minlength=num_bins)
    offsets = np.concatenate(([0], np.cumsum(counts))).astype(COUNT_NP[count_type])
    return keys[perm], (np.asarray(values)[perm] if values is not None else None), perm.astype(np.uint32), offsets
