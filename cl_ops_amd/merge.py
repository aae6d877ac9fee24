"""Python view of CloMerge (include/clo_merge.h): the stable merge of two sorted arrays, with values carried along or
the permutation written (argmerge). A thin ctypes wrapper like histogram.py: every call goes through the C API, nothing
is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY

_sig("clo_merge_new", vp, C.c_char_p, vp, ci, sz, _E)
_sig("clo_merge_destroy", None, vp)
_sig("clo_merge_with_device_data", vp, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, _E)
_sig("clo_merge_with_host_data", _u32, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, _E)
_sig("clo_merge_get_context", vp, vp)
_sig("clo_merge_get_key_type", ci, vp)
_sig("clo_merge_get_key_size", sz, vp)
_sig("clo_merge_get_value_size", sz, vp)
_sig("clo_hip_merge_tile", sz, ci, ci)
_sig("clo_hip_merge_workspace_bytes", sz, sz, sz)
_sig("clo_hip_merge", ci, vp, vp, sz, vp, vp, sz, vp, vp, ci, ci, ci, vp, sz, vp)


def merge_tile(key_size, value_size=0):
    """Output elements per tile of the kernels for keys of key_size and values of value_size (0: none) bytes; 0 for
    sizes that are not built."""
    return lib.clo_hip_merge_tile(key_size, value_size)


class Merge(_Handle):
    """CloMerge. value_size: 0 (keys only), 4 or 8 bytes per value; with 4 and no values the calls are argmerges."""
    _destroy = "clo_merge_destroy"

    def __init__(self, ctx, key_type, value_size=0, options=None):
        self._new("clo_merge_new", _b(options), ctx.h, clo_type(key_type), value_size)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_merge_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_merge_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_merge_get_value_size(self.h))

    def with_device_data(self, q, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out, q_comm=None):
        """clo_merge_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_merge_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_a), _h(values_a), numel_a, _h(keys_b), _h(values_b),
                                             numel_b, _h(keys_out), _h(values_out), err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys_a, keys_b, values_a=None, values_b=None, keys_out=True, q_exec=None, q_comm=None):
        """clo_merge_with_host_data: (merged keys, or None with keys_out=False; merged values, the permutation when a
        merge made with value_size 4 is given no values, or None with value_size 0) as numpy arrays."""
        ka, kb = _keys_1d(keys_a, self.key_size, "keys_a"), _keys_1d(keys_b, self.key_size, "keys_b")
        if ka.dtype != kb.dtype:
            raise ValueError("keys_a and keys_b: one dtype")
        va, vb = _values_like(values_a, ka, self.value_size, "values_a"), _values_like(values_b, kb, self.value_size, "values_b")
        n = ka.size + kb.size
        ko = np.empty(n, dtype=ka.dtype) if keys_out else None
        vo = None
        if self.value_size:
            given = va if va is not None else vb
            vo = np.empty(n, dtype=given.dtype if given is not None else (np.uint32 if self.value_size == 4 else np.uint64))
        err = _Err()
        ok = lib.clo_merge_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(ka), _p(va), ka.size, _p(kb), _p(vb), kb.size,
                                          _p(ko), _p(vo), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_merge_with_host_data failed")
        return ko, vo
