"""Python view of CloJoin (include/clo_join.h): the inner, left, right or full outer equi-join of two sorted key arrays
as pairs of row indices, in ascending key order. A thin ctypes wrapper like setop.py: every call goes through the C
API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, clo_type, CloError, CLO_ERROR_LIBRARY

_sig("clo_join_new", vp, C.c_char_p, C.c_char_p, vp, ci, _E)
_sig("clo_join_destroy", None, vp)
_sig("clo_join_with_device_data", vp, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, vp, _E)
_sig("clo_join_with_host_data", _u32, vp, vp, vp, vp, sz, vp, sz, vp, vp, vp, sz, C.POINTER(sz), _E)
_sig("clo_join_get_context", vp, vp)
_sig("clo_join_get_key_type", ci, vp)
_sig("clo_join_get_key_size", sz, vp)
_sig("clo_join_get_kind", C.c_char_p, vp)
_sig("clo_join_get_max_numel_out", sz, vp, sz, sz)
_sig("clo_hip_join_tile", sz, ci)
_sig("clo_hip_join_out_tile", sz)
_sig("clo_hip_join_workspace_bytes", sz, ci, sz, sz)
_sig("clo_hip_join", ci, ci, vp, sz, vp, sz, vp, vp, vp, sz, vp, ci, ci, vp, sz, vp)

JOIN_KINDS = ("inner", "left", "right", "full")   # the thin ABI's kind numbers, in order
JOIN_NONE = 0xFFFFFFFF                            # the index of a side without a partner


def join_tile(key_size):
    """Merged elements per tile of the kernels for keys of key_size bytes; 0 for sizes that are not built."""
    return lib.clo_hip_join_tile(key_size)


def join_out_tile():
    """Result rows per work-group of the write."""
    return lib.clo_hip_join_out_tile()


class Join(_Handle):
    """CloJoin. kind: one of JOIN_KINDS."""
    _destroy = "clo_join_destroy"

    def __init__(self, kind, ctx, key_type, options=None):
        self._new("clo_join_new", _b(kind), _b(options), ctx.h, clo_type(key_type))
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_join_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_join_get_key_size(self.h))
    kind = property(lambda self: lib.clo_join_get_kind(self.h).decode())

    def max_numel_out(self, numel_a, numel_b):
        """The largest row count a join of inputs of these sizes can have (an upper bound, not a required capacity)."""
        return lib.clo_join_get_max_numel_out(self.h, numel_a, numel_b)

    def with_device_data(self, q, keys_a, numel_a, keys_b, numel_b, idx_a_out, idx_b_out, keys_out, capacity, num_out, q_comm=None):
        """clo_join_with_device_data on Buffers (any output may be None); asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_join_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_a), numel_a, _h(keys_b), numel_b,
                                            _h(idx_a_out), _h(idx_b_out), _h(keys_out), capacity, _h(num_out), err.ref)
        err.raise_if_set()
        return evt

    def _host(self, ka, kb, ia, ib, ko, capacity, q_exec, q_comm):
        k = sz(0)
        err = _Err()
        ok = lib.clo_join_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(ka), ka.size, _p(kb), kb.size,
                                         _p(ia), _p(ib), _p(ko), capacity, C.byref(k), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_join_with_host_data failed")
        return k.value

    def _inputs(self, keys_a, keys_b):
        ka, kb = _keys_1d(keys_a, self.key_size, "keys_a"), _keys_1d(keys_b, self.key_size, "keys_b")
        if ka.dtype != kb.dtype:
            raise ValueError("keys_a and keys_b: one dtype")
        return ka, kb

    def count(self, keys_a, keys_b, q_exec=None, q_comm=None):
        """The count form of clo_join_with_host_data: the rows of the whole join, nothing else written."""
        ka, kb = self._inputs(keys_a, keys_b)
        return self._host(ka, kb, None, None, None, 0, q_exec, q_comm)

    def with_host_data(self, keys_a, keys_b, capacity=None, keys_out=False, q_exec=None, q_comm=None):
        """clo_join_with_host_data: (idx_a, idx_b, the rows' keys or None with keys_out=False, K). The arrays hold the
        first min(K, capacity) rows; capacity None: the count form runs first and its result is the capacity."""
        ka, kb = self._inputs(keys_a, keys_b)
        if capacity is None:
            capacity = self._host(ka, kb, None, None, None, 0, q_exec, q_comm)
        ia, ib = np.empty(capacity, dtype=np.uint32), np.empty(capacity, dtype=np.uint32)
        ko = np.empty(capacity, dtype=ka.dtype) if keys_out else None
        k = self._host(ka, kb, ia, ib, ko, capacity, q_exec, q_comm)
        rows = min(k, capacity)
        return ia[:rows], ib[:rows], (ko[:rows] if ko is not None else None), k
