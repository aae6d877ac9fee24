"""Python view of CloMerge (include/clo_merge.h): the stable merge of two sorted arrays, with values carried along or
the permutation written (argmerge). A thin ctypes wrapper like histogram.py: every call goes through the C API, nothing
is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _sig, _E, _u32, clo_type, CloError, CLO_ERROR_LIBRARY

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


class Merge:
    """CloMerge. value_size: 0 (keys only), 4 or 8 bytes per value; with 4 and no values the calls are argmerges."""

    def __init__(self, ctx, key_type, value_size=0, options=None):
        err = _Err()
        self.h = lib.clo_merge_new(_b(options), ctx.h, clo_type(key_type), value_size, err.ref)
        err.raise_if_set()
        if not self.h:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_merge_new returned NULL")
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_merge_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_merge_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_merge_get_value_size(self.h))

    def with_device_data(self, q, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out, q_comm=None):
        """clo_merge_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        h = lambda b: b.h if b is not None else None
        evt = lib.clo_merge_with_device_data(self.h, h(q), h(q_comm), h(keys_a), h(values_a), numel_a, h(keys_b), h(values_b),
                                             numel_b, h(keys_out), h(values_out), err.ref)
        err.raise_if_set()
        return evt

    def _keys(self, keys, what):
        k = np.ascontiguousarray(keys)
        if k.ndim != 1 or k.itemsize != self.key_size:
            raise ValueError("%s: a 1-D array of %d-byte elements" % (what, self.key_size))
        return k

    def _values(self, values, keys, what):
        if values is None:
            return None
        v = np.ascontiguousarray(values)
        if v.shape != keys.shape or v.itemsize != self.value_size or self.value_size == 0:
            raise ValueError("%s: %d-byte elements, as many as keys" % (what, self.value_size))
        return v

    def with_host_data(self, keys_a, keys_b, values_a=None, values_b=None, keys_out=True, q_exec=None, q_comm=None):
        """clo_merge_with_host_data: (merged keys, or None with keys_out=False; merged values, the permutation when a
        merge made with value_size 4 is given no values, or None with value_size 0) as numpy arrays."""
        ka, kb = self._keys(keys_a, "keys_a"), self._keys(keys_b, "keys_b")
        if ka.dtype != kb.dtype:
            raise ValueError("keys_a and keys_b: one dtype")
        va, vb = self._values(values_a, ka, "values_a"), self._values(values_b, kb, "values_b")
        n = ka.size + kb.size
        ko = np.empty(n, dtype=ka.dtype) if keys_out else None
        vo = None
        if self.value_size:
            given = va if va is not None else vb
            vo = np.empty(n, dtype=given.dtype if given is not None else (np.uint32 if self.value_size == 4 else np.uint64))
        p = lambda a: a.ctypes.data_as(vp) if a is not None else None
        err = _Err()
        ok = lib.clo_merge_with_host_data(self.h, q_exec.h if q_exec else None, q_comm.h if q_comm else None,
                                          p(ka), p(va), ka.size, p(kb), p(vb), kb.size, p(ko), p(vo), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_merge_with_host_data failed")
        return ko, vo

    def close(self):
        if self.h:
            lib.clo_merge_destroy(self.h)
            self.h = None
