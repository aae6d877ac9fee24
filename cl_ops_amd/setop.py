"""Python view of CloSetOp (include/clo_setop.h): union, intersection, difference and symmetric difference of two
sorted arrays as multisets, with values carried along or the indices written. A thin ctypes wrapper like merge.py:
every call goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY

_sig("clo_setop_new", vp, C.c_char_p, C.c_char_p, vp, ci, sz, _E)
_sig("clo_setop_destroy", None, vp)
_sig("clo_setop_with_device_data", vp, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, vp, _E)
_sig("clo_setop_with_host_data", _u32, vp, vp, vp, vp, vp, sz, vp, vp, sz, vp, vp, C.POINTER(sz), _E)
_sig("clo_setop_get_context", vp, vp)
_sig("clo_setop_get_key_type", ci, vp)
_sig("clo_setop_get_key_size", sz, vp)
_sig("clo_setop_get_value_size", sz, vp)
_sig("clo_setop_get_op", C.c_char_p, vp)
_sig("clo_setop_get_max_numel_out", sz, vp, sz, sz)
_sig("clo_hip_setop_tile", sz, ci, ci)
_sig("clo_hip_setop_workspace_bytes", sz, sz, sz)
_sig("clo_hip_setop", ci, ci, vp, vp, sz, vp, vp, sz, vp, vp, vp, ci, ci, ci, vp, sz, vp)

SETOP_OPS = ("union", "intersection", "difference", "symmetric_difference")   # the thin ABI's op numbers, in order


def setop_tile(key_size, value_size=0):
    """Merged elements per tile of the kernels for keys of key_size and values of value_size (0: none) bytes; 0 for
    sizes that are not built."""
    return lib.clo_hip_setop_tile(key_size, value_size)


class SetOp(_Handle):
    """CloSetOp. op: one of SETOP_OPS. value_size: 0 (keys only), 4 or 8 bytes per value; with 4 and no values the
    calls write indices into A || B."""
    _destroy = "clo_setop_destroy"

    def __init__(self, op, ctx, key_type, value_size=0, options=None):
        self._new("clo_setop_new", _b(op), _b(options), ctx.h, clo_type(key_type), value_size)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_setop_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_setop_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_setop_get_value_size(self.h))
    op = property(lambda self: lib.clo_setop_get_op(self.h).decode())

    def max_numel_out(self, numel_a, numel_b):
        """The elements keys_out and values_out must hold."""
        return lib.clo_setop_get_max_numel_out(self.h, numel_a, numel_b)

    def with_device_data(self, q, keys_a, values_a, numel_a, keys_b, values_b, numel_b, keys_out, values_out, num_out, q_comm=None):
        """clo_setop_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_setop_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_a), _h(values_a), numel_a, _h(keys_b), _h(values_b),
                                             numel_b, _h(keys_out), _h(values_out), _h(num_out), err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys_a, keys_b, values_a=None, values_b=None, keys_out=True, q_exec=None, q_comm=None):
        """clo_setop_with_host_data: (the k kept keys, or None with keys_out=False; their values, their indices when
        an object made with value_size 4 is given no values, or None with value_size 0) as numpy arrays."""
        ka, kb = _keys_1d(keys_a, self.key_size, "keys_a"), _keys_1d(keys_b, self.key_size, "keys_b")
        if ka.dtype != kb.dtype:
            raise ValueError("keys_a and keys_b: one dtype")
        va, vb = _values_like(values_a, ka, self.value_size, "values_a"), _values_like(values_b, kb, self.value_size, "values_b")
        cap = self.max_numel_out(ka.size, kb.size)
        ko = np.empty(cap, dtype=ka.dtype) if keys_out else None
        vo = None
        if self.value_size:
            given = va if va is not None else vb
            vo = np.empty(cap, dtype=given.dtype if given is not None else (np.uint32 if self.value_size == 4 else np.uint64))
        k = sz(0)
        err = _Err()
        ok = lib.clo_setop_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(ka), _p(va), ka.size, _p(kb), _p(vb), kb.size,
                                          _p(ko), _p(vo), C.byref(k), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_setop_with_host_data failed")
        return (ko[:k.value] if ko is not None else None), (vo[:k.value] if vo is not None else None)
