"""Python view of CloReduceByKey (include/clo_reduce.h): every run of equal keys collapsed into one row (the key,
and the sum / min / max of the run's values, or the run's length). A thin ctypes wrapper like api.py and rng.py:
every call goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, _values_like, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_reduce_by_key_new", vp, C.c_char_p, C.c_char_p, vp, ci, ci, ci, _E)
_sig("clo_reduce_by_key_destroy", None, vp)
_sig("clo_reduce_by_key_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, _E)
_sig("clo_reduce_by_key_with_host_data", _u32, vp, vp, vp, vp, vp, vp, vp, C.POINTER(sz), sz, _E)
_sig("clo_reduce_by_key_get_context", vp, vp)
_sig("clo_reduce_by_key_get_key_type", ci, vp)
_sig("clo_reduce_by_key_get_key_size", sz, vp)
_sig("clo_reduce_by_key_get_value_type", ci, vp)
_sig("clo_reduce_by_key_get_value_size", sz, vp)
_sig("clo_reduce_by_key_get_sum_type", ci, vp)
_sig("clo_reduce_by_key_get_sum_size", sz, vp)
_sig("clo_reduce_by_key_get_op", C.c_char_p, vp)
_sig("clo_hip_reduce_by_key_tile", sz, ci, ci)
_sig("clo_hip_reduce_by_key_workspace_bytes", sz, sz)
_sig("clo_hip_reduce_by_key", ci, vp, vp, vp, vp, vp, sz, ci, ci, ci, ci, vp, sz, vp)

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}


def reduce_by_key_tile(key_size, value_size=0):
    """Elements per tile of the kernels for keys of key_size and values of value_size (0: none) bytes."""
    return lib.clo_hip_reduce_by_key_tile(key_size, value_size)


class ReduceByKey(_Handle):
    """CloReduceByKey. value_type None: 'uint' (calls without values ignore it); sum_type None: the value type."""
    _destroy = "clo_reduce_by_key_destroy"

    def __init__(self, ctx, key_type, value_type=None, sum_type=None, op="sum", options=None):
        kt = clo_type(key_type)
        vt = clo_type(value_type) if value_type is not None else CLO_TYPES["uint"]
        st = clo_type(sum_type) if sum_type is not None else vt
        self._new("clo_reduce_by_key_new", _b(op), _b(options), ctx.h, kt, vt, st)
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_reduce_by_key_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_reduce_by_key_get_key_size(self.h))
    value_type = property(lambda self: lib.clo_reduce_by_key_get_value_type(self.h))
    value_size = property(lambda self: lib.clo_reduce_by_key_get_value_size(self.h))
    sum_type = property(lambda self: lib.clo_reduce_by_key_get_sum_type(self.h))
    sum_size = property(lambda self: lib.clo_reduce_by_key_get_sum_size(self.h))
    op = property(lambda self: lib.clo_reduce_by_key_get_op(self.h).decode())

    def with_device_data(self, q, keys_in, values_in, keys_out, aggr_out, num_runs_out, numel, q_comm=None):
        """clo_reduce_by_key_with_device_data on Buffers (values_in, keys_out or aggr_out may be None); asynchronous on
        q. num_runs_out: a Buffer of one uint64. Returns the event."""
        err = _Err()
        evt = lib.clo_reduce_by_key_with_device_data(self.h, _h(q), _h(q_comm), _h(keys_in), _h(values_in), _h(keys_out),
                                                     _h(aggr_out), _h(num_runs_out), numel, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, keys, values=None, q_exec=None, q_comm=None, want_keys=True, want_aggr=True):
        """clo_reduce_by_key_with_host_data: (keys_out[:m], aggr_out[:m]) as numpy arrays, None for an output that
        was not asked for."""
        k = _keys_1d(keys, self.key_size, "keys")
        v = _values_like(values, k, self.value_size, "values")
        ko = np.empty_like(k) if want_keys else None
        ao = np.empty(k.shape, dtype=CLO_TYPE_NP[_TYPE_NAMES[self.sum_type]]) if want_aggr else None
        m = sz(0)
        err = _Err()
        ok = lib.clo_reduce_by_key_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(k), _p(v), _p(ko), _p(ao), C.byref(m), k.size, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_reduce_by_key_with_host_data failed")
        return (ko[:m.value] if ko is not None else None), (ao[:m.value] if ao is not None else None)
