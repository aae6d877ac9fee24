"""Python view of CloHistogram (include/clo_histogram.h): counts or sums of values per bin of integer keys,
bin = (key - lower) >> shift. A thin ctypes wrapper like reduce.py: every call goes through the C API, nothing is
computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_histogram_new", vp, C.c_char_p, vp, ci, ci, ci, _E)
_sig("clo_histogram_destroy", None, vp)
_sig("clo_histogram_with_device_data", vp, vp, vp, vp, vp, vp, vp, sz, vp, C.c_uint, sz, _E)
_sig("clo_histogram_with_host_data", _u32, vp, vp, vp, vp, vp, vp, sz, vp, C.c_uint, sz, _E)
_sig("clo_histogram_get_context", vp, vp)
_sig("clo_histogram_get_key_type", ci, vp)
_sig("clo_histogram_get_key_size", sz, vp)
_sig("clo_histogram_get_value_type", ci, vp)
_sig("clo_histogram_get_value_size", sz, vp)
_sig("clo_histogram_get_sum_type", ci, vp)
_sig("clo_histogram_get_sum_size", sz, vp)
_sig("clo_histogram_get_accumulate", _u32, vp)
_sig("clo_hip_histogram_tile", sz, ci, ci)
_sig("clo_hip_histogram_lds_bins", sz, ci)
_sig("clo_hip_histogram_workspace_bytes", sz, sz, sz)
_sig("clo_hip_histogram", ci, vp, vp, vp, sz, ci, ci, ci, ci, C.c_uint64, C.c_uint, sz, ci, C.c_uint, vp, sz, vp)

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}


def histogram_tile(key_size, value_size=0):
    """Elements per tile of the kernels for keys of key_size and values of value_size (0: none) bytes."""
    return lib.clo_hip_histogram_tile(key_size, value_size)


def histogram_lds_bins(sum_size=4):
    """The largest num_bins whose counters a work-group keeps in LDS, for sums of sum_size bytes."""
    return lib.clo_hip_histogram_lds_bins(sum_size)


class Histogram(_Handle):
    """CloHistogram. value_type None: 'uint' (calls without values ignore it); sum_type None: the value type.
    options: None or 'accumulate'."""
    _destroy = "clo_histogram_destroy"

    def __init__(self, ctx, key_type, value_type=None, sum_type=None, options=None):
        kt = clo_type(key_type)
        vt = clo_type(value_type) if value_type is not None else CLO_TYPES["uint"]
        st = clo_type(sum_type) if sum_type is not None else vt
        self._new("clo_histogram_new", _b(options), ctx.h, kt, vt, st)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_histogram_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_histogram_get_key_size(self.h))
    value_type = property(lambda self: lib.clo_histogram_get_value_type(self.h))
    value_size = property(lambda self: lib.clo_histogram_get_value_size(self.h))
    sum_type = property(lambda self: lib.clo_histogram_get_sum_type(self.h))
    sum_size = property(lambda self: lib.clo_histogram_get_sum_size(self.h))
    accumulate = property(lambda self: bool(lib.clo_histogram_get_accumulate(self.h)))

    def _lower(self, lower):
        """One host value of the key type (what the C API's `lower` points to), kept alive by the caller."""
        return np.array([lower], dtype=CLO_TYPE_NP[_TYPE_NAMES[self.key_type]])

    def with_device_data(self, q, keys_in, values_in, hist_out, numel, lower=0, shift=0, num_bins=None, q_comm=None):
        """clo_histogram_with_device_data on Buffers (values_in may be None); asynchronous on q. Returns the event."""
        err = _Err()
        lo = self._lower(lower)
        evt = lib.clo_histogram_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_in), _h(values_in), _h(hist_out), numel,
                                                 lo.ctypes.data_as(vp), shift, num_bins, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys, values=None, lower=0, shift=0, num_bins=None, out=None, q_exec=None, q_comm=None):
        """clo_histogram_with_host_data: the num_bins sums as a numpy array of the sum type. out: the array the
        results are written to (under 'accumulate': added onto; without one, onto zeros)."""
        k = _keys_1d(keys, self.key_size, "keys")
        v = _values_like(values, k, self.value_size, "values")
        st = CLO_TYPE_NP[_TYPE_NAMES[self.sum_type]]
        if out is None:
            out = np.zeros(num_bins, dtype=st)
        elif out.dtype != np.dtype(st) or out.ndim != 1 or out.size != num_bins or not out.flags.c_contiguous:
            raise ValueError("out: a contiguous 1-D array of num_bins elements of the sum type")
        lo = self._lower(lower)
        err = _Err()
        ok = lib.clo_histogram_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(k), _p(v), _p(out), k.size, _p(lo), shift, num_bins, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_histogram_with_host_data failed")
        return out
