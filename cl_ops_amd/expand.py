"""Python view of CloExpand (include/clo_expand.h): run-length decode and segment ids from counts or from CSR offsets. A
thin ctypes wrapper like select.py: every call goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPE_NP

_sig("clo_expand_new", vp, C.c_char_p, C.c_char_p, vp, ci, ci, _E)
_sig("clo_expand_destroy", None, vp)
_sig("clo_expand_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, _E)
_sig("clo_expand_with_host_data", _u32, vp, vp, vp, vp, C.POINTER(sz), vp, vp, vp, vp, C.POINTER(sz), sz, sz, _E)
_sig("clo_expand_get_context", vp, vp)
_sig("clo_expand_get_form", C.c_char_p, vp)
_sig("clo_expand_get_value_type", ci, vp)
_sig("clo_expand_get_value_size", sz, vp)
_sig("clo_expand_get_count_type", ci, vp)
_sig("clo_expand_get_count_size", sz, vp)
_sig("clo_hip_expand_tile", sz, ci)
_sig("clo_hip_expand_lds_segments", sz)
_sig("clo_hip_expand_workspace_bytes", sz, sz, sz)
_sig("clo_hip_expand", ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, sz, sz, ci, vp, sz, vp)

EXPAND_FORMS = ("counts", "offsets")   # the thin ABI's form numbers, in order


def expand_tile(value_size=0):
    """T: output rows per tile of the kernels for values of value_size bytes (0: none); 0 for sizes that are not built."""
    return lib.clo_hip_expand_tile(value_size)


def expand_lds_segments():
    """L: the most segment ends a tile takes through LDS; above it every row of the tile searches global memory."""
    return lib.clo_hip_expand_lds_segments()


class Expand(_Handle):
    """CloExpand. form: one of EXPAND_FORMS. value_type: the type of the values (opaque words of its size), None where
    no values are passed. count_type: uint or ulong, the type of the counts or offsets."""
    _destroy = "clo_expand_destroy"

    def __init__(self, form, ctx, value_type=None, count_type="uint", options=None):
        self._new("clo_expand_new", _b(form), _b(options), ctx.h, clo_type(value_type if value_type is not None else "uchar"), clo_type(count_type))
        self.ctx = ctx

    form = property(lambda self: lib.clo_expand_get_form(self.h).decode())
    value_type = property(lambda self: lib.clo_expand_get_value_type(self.h))
    value_size = property(lambda self: lib.clo_expand_get_value_size(self.h))
    count_type = property(lambda self: lib.clo_expand_get_count_type(self.h))
    count_size = property(lambda self: lib.clo_expand_get_count_size(self.h))

    def with_device_data(self, q, counts_or_offsets, num_in, values_in, values_out, seg_out, rank_out, num_out, numel_in, capacity, q_comm=None):
        """clo_expand_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_expand_with_device_data(self.h, _h(q), _h(q_comm), _h(counts_or_offsets), _h(num_in), _h(values_in),
                                              _h(values_out), _h(seg_out), _h(rank_out), _h(num_out), numel_in, capacity, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, counts_or_offsets, capacity, values=None, num_in=None, seg=True, rank=False, q_exec=None, q_comm=None):
        """clo_expand_with_host_data: (values, seg, rank, total) with numpy arrays of min(total, capacity) rows, None for
        what was not asked for. counts_or_offsets: numel_in counts or numel_in + 1 offsets of the object's count type."""
        cdt = np.uint32 if self.count_size == 4 else np.uint64
        c = np.ascontiguousarray(counts_or_offsets)
        if c.ndim != 1 or c.dtype != cdt:
            raise ValueError("counts_or_offsets: a 1-D array of %s" % np.dtype(cdt).name)
        offsets = self.form == "offsets"
        if offsets and c.size == 0:
            raise ValueError("offsets: numel_in + 1 of them")
        n = c.size - 1 if offsets else c.size
        v = None
        if values is not None:
            v = np.ascontiguousarray(values)
            if v.ndim != 1 or v.dtype.itemsize != self.value_size or v.size != n:
                raise ValueError("values: numel_in words of %d bytes" % self.value_size)
        vo = np.empty(capacity, dtype=v.dtype) if v is not None else None
        so = np.empty(capacity, dtype=np.uint32) if seg else None
        ro = np.empty(capacity, dtype=np.uint32) if rank else None
        m = sz(num_in) if num_in is not None else None
        num = sz(0)
        err = _Err()
        ok = lib.clo_expand_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(c), C.byref(m) if m is not None else None, _p(v),
                                           _p(vo), _p(so), _p(ro), C.byref(num), n, capacity, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_expand_with_host_data failed")
        rows = min(num.value, capacity)
        return tuple(x[:rows] if x is not None else None for x in (vo, so, ro)) + (num.value,)
