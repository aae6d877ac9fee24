"""Python view of CloBucket (include/clo_bucket.h): stable multi-way partition of rows by the bin of an integer key,
bin = (key - lower) >> shift, with values carried along or the indices written, and the buckets' CSR offsets. A thin
ctypes wrapper like histogram.py: every call goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_bucket_new", vp, C.c_char_p, vp, ci, sz, ci, _E)
_sig("clo_bucket_destroy", None, vp)
_sig("clo_bucket_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, C.c_uint, sz, _E)
_sig("clo_bucket_with_host_data", _u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, vp, C.c_uint, sz, _E)
_sig("clo_bucket_get_context", vp, vp)
_sig("clo_bucket_get_key_type", ci, vp)
_sig("clo_bucket_get_key_size", sz, vp)
_sig("clo_bucket_get_value_size", sz, vp)
_sig("clo_bucket_get_count_type", ci, vp)
_sig("clo_bucket_get_count_size", sz, vp)
_sig("clo_hip_bucket_tile", sz, ci, ci)
_sig("clo_hip_bucket_workspace_bytes", sz, sz, ci, ci, sz)
_sig("clo_hip_bucket", ci, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci, C.c_uint64, C.c_uint, sz, vp, sz, vp)

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}

BUCKET_MAX_BINS = 65535       # CLO_BUCKET_MAX_BINS
BUCKET_SCAN_GROUP = 4096      # CLO_HIP_BUCKET_SCAN_GROUP: the counters (digits of the pass x tiles) a work-group of the counter scan takes
BUCKET_SCAN_TRIP = 2048       # CLO_HIP_BUCKET_SCAN_TRIP: the groups' sums the one-group scan takes per trip of its loop


def bucket_tile(key_size, value_size=0):
    """Rows per tile of the kernels for keys of key_size and values of value_size (0: none) bytes; 0 for sizes that
    are not built."""
    return lib.clo_hip_bucket_tile(key_size, value_size)


class Bucket(_Handle):
    """CloBucket. value_size: 0 (keys only), 4 or 8 bytes per value; with 4 and no values the calls write the rows'
    input indices. count_type: 'uint' or 'ulong', the type of the offsets."""
    _destroy = "clo_bucket_destroy"

    def __init__(self, ctx, key_type, value_size=0, count_type="uint", options=None):
        self._new("clo_bucket_new", _b(options), ctx.h, clo_type(key_type), value_size, clo_type(count_type))
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_bucket_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_bucket_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_bucket_get_value_size(self.h))
    count_type = property(lambda self: lib.clo_bucket_get_count_type(self.h))
    count_size = property(lambda self: lib.clo_bucket_get_count_size(self.h))

    def _lower(self, lower):
        """One host value of the key type (what the C API's `lower` points to), kept alive by the caller."""
        return np.array([lower], dtype=CLO_TYPE_NP[_TYPE_NAMES[self.key_type]])

    def with_device_data(self, q, keys_in, values_in, keys_out, values_out, offsets_out, numel, lower=0, shift=0, num_bins=None, q_comm=None):
        """clo_bucket_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        lo = self._lower(lower)
        evt = lib.clo_bucket_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_in), _h(values_in), _h(keys_out), _h(values_out),
                                              _h(offsets_out), numel, lo.ctypes.data_as(vp), shift, num_bins, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys, values=None, lower=0, shift=0, num_bins=None, keys_out=True, q_exec=None, q_comm=None):
        """clo_bucket_with_host_data: (keys, values, offsets) as numpy arrays. keys: the rows' keys bin by bin, None with
        keys_out=False (the arg form only). values: their values, their input indices when an object made with
        value_size 4 is given no values, None with value_size 0. offsets: num_bins + 1 entries of the count type."""
        k = _keys_1d(keys, self.key_size, "keys")
        v = _values_like(values, k, self.value_size, "values")
        ko = np.empty(k.size, dtype=k.dtype) if keys_out else None
        vo = None
        if self.value_size:
            vo = np.empty(k.size, dtype=v.dtype if v is not None else (np.uint32 if self.value_size == 4 else np.uint64))
        off = np.empty(num_bins + 1, dtype=CLO_TYPE_NP[_TYPE_NAMES[self.count_type]])
        lo = self._lower(lower)
        err = _Err()
        ok = lib.clo_bucket_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(k), _p(v), _p(ko), _p(vo), _p(off), k.size, _p(lo), shift, num_bins, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_bucket_with_host_data failed")
        return ko, vo, off
