"""Python view of CloSelect (include/clo_select.h): stable selection and partition by flags or by comparison with a
threshold, with values carried along or the indices written. A thin ctypes wrapper like setop.py: every call goes
through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY

_sig("clo_select_new", vp, C.c_char_p, C.c_char_p, C.c_char_p, vp, ci, sz, _E)
_sig("clo_select_destroy", None, vp)
_sig("clo_select_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, _E)
_sig("clo_select_with_host_data", _u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, C.POINTER(sz), _E)
_sig("clo_select_get_context", vp, vp)
_sig("clo_select_get_key_type", ci, vp)
_sig("clo_select_get_key_size", sz, vp)
_sig("clo_select_get_value_size", sz, vp)
_sig("clo_select_get_op", C.c_char_p, vp)
_sig("clo_select_get_pred", C.c_char_p, vp)
_sig("clo_hip_select_tile", sz, ci, ci)
_sig("clo_hip_select_workspace_bytes", sz, sz, ci, ci)
_sig("clo_hip_select", ci, ci, ci, vp, vp, vp, vp, vp, vp, sz, ci, ci, ci, vp, sz, vp)

SELECT_OPS = ("select", "partition")                            # the thin ABI's op numbers, in order
SELECT_PREDS = ("flagged", "lt", "le", "gt", "ge", "eq", "ne")  # and its pred numbers
SELECT_SCAN_TRIP = 2048   # CLO_HIP_SELECT_SCAN_TRIP: the tile counts the count scan takes per trip of its loop


def select_tile(key_size, value_size=0):
    """Elements per tile of the kernels for keys of key_size and values of value_size (0: none) bytes; 0 for sizes
    that are not built."""
    return lib.clo_hip_select_tile(key_size, value_size)


class Select(_Handle):
    """CloSelect. op: one of SELECT_OPS, pred: one of SELECT_PREDS. value_size: 0 (keys only), 4 or 8 bytes per value;
    with 4 and no values the calls write the elements' indices."""
    _destroy = "clo_select_destroy"

    def __init__(self, op, pred, ctx, key_type, value_size=0, options=None):
        self._new("clo_select_new", _b(op), _b(pred), _b(options), ctx.h, clo_type(key_type), value_size)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_select_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_select_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_select_get_value_size(self.h))
    op = property(lambda self: lib.clo_select_get_op(self.h).decode())
    pred = property(lambda self: lib.clo_select_get_pred(self.h).decode())

    def with_device_data(self, q, keys_in, values_in, flags_or_threshold, keys_out, values_out, num_out, numel, q_comm=None):
        """clo_select_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_select_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_in), _h(values_in), _h(flags_or_threshold),
                                              _h(keys_out), _h(values_out), _h(num_out), numel, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys, flags_or_threshold, values=None, keys_out=True, q_exec=None, q_comm=None):
        """clo_select_with_host_data: (keys, values, k) as numpy arrays. keys: the k kept keys of a select, all numel
        rows of a partition, None with keys_out=False. values: their values, their indices when an object made with
        value_size 4 is given no values, None with value_size 0. flags_or_threshold: numel flag bytes for "flagged",
        else one key. keys may be None where no keys are read (then flags_or_threshold gives numel)."""
        flagged = self.pred == "flagged"
        if flagged:
            f = np.ascontiguousarray(flags_or_threshold)
            if f.ndim != 1 or f.itemsize != 1:
                raise ValueError("flags: a 1-D array of bytes")
        k = None
        if keys is not None:
            k = _keys_1d(keys, self.key_size, "keys")
            if not flagged:
                f = np.ascontiguousarray(flags_or_threshold, dtype=k.dtype).reshape(-1)
                if f.size != 1:
                    raise ValueError("threshold: one key")
        elif not flagged:
            raise ValueError("keys: required by a comparison")
        n = k.size if k is not None else f.size
        if flagged and f.size != n:
            raise ValueError("flags: as many as keys")
        v = _values_like(values, k if k is not None else f, self.value_size, "values")
        ko = np.empty(n, dtype=k.dtype) if keys_out and k is not None else None
        vo = None
        if self.value_size:
            vo = np.empty(n, dtype=v.dtype if v is not None else (np.uint32 if self.value_size == 4 else np.uint64))
        num = sz(0)
        err = _Err()
        ok = lib.clo_select_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(k), _p(v), _p(f), _p(ko), _p(vo), n, C.byref(num), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_select_with_host_data failed")
        rows = n if self.op == "partition" else num.value
        return (ko[:rows] if ko is not None else None), (vo[:rows] if vo is not None else None), num.value
