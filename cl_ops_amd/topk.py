"""Python view of CloTopK (include/clo_topk.h): the k smallest or largest keys, with values carried along or the indices
written, and the k-th key. A thin ctypes wrapper like select.py: every call goes through the C API, nothing is computed
in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY

_sig("clo_topk_new", vp, C.c_char_p, C.c_char_p, C.c_char_p, vp, ci, sz, _E)
_sig("clo_topk_destroy", None, vp)
_sig("clo_topk_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, _E)
_sig("clo_topk_with_host_data", _u32, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, _E)
_sig("clo_topk_get_context", vp, vp)
_sig("clo_topk_get_key_type", ci, vp)
_sig("clo_topk_get_key_size", sz, vp)
_sig("clo_topk_get_value_size", sz, vp)
_sig("clo_topk_get_which", C.c_char_p, vp)
_sig("clo_topk_get_order", C.c_char_p, vp)
_sig("clo_hip_topk_tile", sz, ci, ci)
_sig("clo_hip_topk_sorted_max", sz, ci, ci)
_sig("clo_hip_topk_sweep_groups", sz)
_sig("clo_hip_topk_workspace_bytes", sz, sz, ci, ci)
_sig("clo_hip_topk", ci, ci, ci, vp, vp, vp, vp, vp, sz, sz, ci, ci, ci, vp, sz, vp)

TOPK_WHICH = ("smallest", "largest")   # the thin ABI's which numbers, in order
TOPK_ORDERS = ("input", "sorted")      # and its order numbers
TOPK_SCAN_TRIP = 2048   # CLO_HIP_TOPK_SCAN_TRIP: the tiles the count scan takes per trip of its loop


def topk_tile(key_size, value_size=0):
    """Elements per tile of the count and apply kernels for keys of key_size and values of value_size (0: none) bytes;
    0 for sizes that are not built."""
    return lib.clo_hip_topk_tile(key_size, value_size)


def topk_sweep_groups():
    """The work-groups a digit sweep launches on the current device where its tile count (tiles of topk_tile(key_size)
    keys) does not limit it; with more tiles than that a group takes several."""
    return lib.clo_hip_topk_sweep_groups()


def topk_sorted_max(key_size, value_size=0):
    """The largest min(k, numel) the "sorted" order takes; 0 for sizes that are not built."""
    return lib.clo_hip_topk_sorted_max(key_size, value_size)


class TopK(_Handle):
    """CloTopK. which: one of TOPK_WHICH, order: one of TOPK_ORDERS. value_size: 0 (keys only), 4 or 8 bytes per value;
    with 4 and no values the calls write the elements' indices."""
    _destroy = "clo_topk_destroy"

    def __init__(self, which, order, ctx, key_type, value_size=0, options=None):
        self._new("clo_topk_new", _b(which), _b(order), _b(options), ctx.h, clo_type(key_type), value_size)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_topk_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_topk_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_topk_get_value_size(self.h))
    which = property(lambda self: lib.clo_topk_get_which(self.h).decode())
    order = property(lambda self: lib.clo_topk_get_order(self.h).decode())

    def with_device_data(self, q, keys_in, values_in, keys_out, values_out, kth_out, numel, k, q_comm=None):
        """clo_topk_with_device_data on Buffers (any of which may be None where the contract allows NULL); asynchronous
        on q. Returns the event (None where min(k, numel) is 0 only if the call failed: errors raise)."""
        err = _Err()
        evt = lib.clo_topk_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_in), _h(values_in), _h(keys_out), _h(values_out),
                                            _h(kth_out), numel, k, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys, k, values=None, keys_out=True, kth=True, q_exec=None, q_comm=None):
        """clo_topk_with_host_data: (keys, values, kth) as numpy arrays of m = min(k, len(keys)) rows. keys: None with
        keys_out=False. values: the rows' values, their indices when an object made with value_size 4 is given no
        values, None with value_size 0. kth: the k-th key as a 0-d array, None with kth=False or m == 0."""
        a = _keys_1d(keys, self.key_size, "keys")
        n = a.size
        m = min(int(k), n)
        v = _values_like(values, a, self.value_size, "values")
        ko = np.empty(m, dtype=a.dtype) if keys_out else None
        vo = None
        if self.value_size:
            vo = np.empty(m, dtype=v.dtype if v is not None else (np.uint32 if self.value_size == 4 else np.uint64))
        kt = np.zeros(1, dtype=a.dtype) if kth else None
        err = _Err()
        ok = lib.clo_topk_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(a), _p(v), _p(ko), _p(vo), _p(kt), n, int(k), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_topk_with_host_data failed")
        return ko, vo, (kt[0] if kt is not None and m > 0 else None)
