"""Python view of CloScanByKey (include/clo_scan_by_key.h): the running sum / min / max of every element within its
run of equal keys, exclusive or inclusive, or without values the element's rank in its run. A thin ctypes wrapper
like reduce.py: every call goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_scan_by_key_new", vp, C.c_char_p, C.c_char_p, vp, ci, ci, ci, _E)
_sig("clo_scan_by_key_destroy", None, vp)
_sig("clo_scan_by_key_with_device_data", vp, vp, vp, vp, vp, vp, vp, sz, _E)
_sig("clo_scan_by_key_with_host_data", _u32, vp, vp, vp, vp, vp, vp, sz, _E)
_sig("clo_scan_by_key_get_context", vp, vp)
_sig("clo_scan_by_key_get_key_type", ci, vp)
_sig("clo_scan_by_key_get_key_size", sz, vp)
_sig("clo_scan_by_key_get_value_type", ci, vp)
_sig("clo_scan_by_key_get_value_size", sz, vp)
_sig("clo_scan_by_key_get_sum_type", ci, vp)
_sig("clo_scan_by_key_get_sum_size", sz, vp)
_sig("clo_scan_by_key_get_op", C.c_char_p, vp)
_sig("clo_scan_by_key_get_inclusive", _u32, vp)
_sig("clo_hip_scan_by_key_tile", sz, ci, ci)
_sig("clo_hip_scan_by_key_workspace_bytes", sz, sz)
_sig("clo_hip_scan_by_key", ci, vp, vp, vp, sz, ci, ci, ci, ci, ci, vp, sz, vp)

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}


def scan_by_key_tile(key_size, value_size=0):
    """Elements per tile of the kernels for keys of key_size and values of value_size (0: none) bytes."""
    return lib.clo_hip_scan_by_key_tile(key_size, value_size)


class ScanByKey(_Handle):
    """CloScanByKey. value_type None: 'uint' (calls without values ignore it); sum_type None: the value type.
    inclusive: the option string "inclusive=1" of the C API."""
    _destroy = "clo_scan_by_key_destroy"

    def __init__(self, ctx, key_type, value_type=None, sum_type=None, op="sum", inclusive=False):
        kt = clo_type(key_type)
        vt = clo_type(value_type) if value_type is not None else CLO_TYPES["uint"]
        st = clo_type(sum_type) if sum_type is not None else vt
        options = "inclusive=1" if inclusive else None
        self._new("clo_scan_by_key_new", _b(op), _b(options), ctx.h, kt, vt, st)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_scan_by_key_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_scan_by_key_get_key_size(self.h))
    value_type = property(lambda self: lib.clo_scan_by_key_get_value_type(self.h))
    value_size = property(lambda self: lib.clo_scan_by_key_get_value_size(self.h))
    sum_type = property(lambda self: lib.clo_scan_by_key_get_sum_type(self.h))
    sum_size = property(lambda self: lib.clo_scan_by_key_get_sum_size(self.h))
    op = property(lambda self: lib.clo_scan_by_key_get_op(self.h).decode())
    inclusive = property(lambda self: bool(lib.clo_scan_by_key_get_inclusive(self.h)))

    def with_device_data(self, q, keys_in, values_in, data_out, numel, q_comm=None):
        """clo_scan_by_key_with_device_data on Buffers (values_in may be None; data_out may be values_in itself when
        the sum type is as wide as the value type); asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_scan_by_key_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_in), _h(values_in), _h(data_out), numel, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys, values=None, q_exec=None, q_comm=None, out=None):
        """clo_scan_by_key_with_host_data: the results as a numpy array of the sum type. out: an array to write them
        to (`values` itself for the in-place form) instead of a new one."""
        k = _keys_1d(keys, self.key_size, "keys")
        v = None
        if values is not None:
            v = values if out is values else np.ascontiguousarray(values)
            if v.shape != k.shape or v.itemsize != self.value_size:
                raise ValueError("values: %d-byte elements, as many as keys" % self.value_size)
        if out is None:
            out = np.empty(k.shape, dtype=CLO_TYPE_NP[_TYPE_NAMES[self.sum_type]])
        elif out.shape != k.shape or out.itemsize != self.sum_size or not out.flags.c_contiguous:
            raise ValueError("out: a contiguous array of %d-byte elements, as many as keys" % self.sum_size)
        err = _Err()
        ok = lib.clo_scan_by_key_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(k), _p(v), _p(out), k.size, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_scan_by_key_with_host_data failed")
        return out
