"""Python view of CloSegFSum (include/clo_segfsum.h): the floating-point sum of every segment in a fixed, modelled
order, the segments given by counts or by CSR offsets. A thin ctypes wrapper like segreduce.py: every call goes through
the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_segfsum_new", vp, C.c_char_p, C.c_char_p, vp, ci, ci, ci, _E)
_sig("clo_segfsum_destroy", None, vp)
_sig("clo_segfsum_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, _E)
_sig("clo_segfsum_with_host_data", _u32, vp, vp, vp, vp, C.POINTER(sz), vp, vp, C.POINTER(sz), sz, sz, _E)
_sig("clo_segfsum_get_context", vp, vp)
_sig("clo_segfsum_get_form", C.c_char_p, vp)
_sig("clo_segfsum_get_value_type", ci, vp)
_sig("clo_segfsum_get_value_size", sz, vp)
_sig("clo_segfsum_get_sum_type", ci, vp)
_sig("clo_segfsum_get_sum_size", sz, vp)
_sig("clo_segfsum_get_count_type", ci, vp)
_sig("clo_segfsum_get_count_size", sz, vp)
_sig("clo_hip_segfsum_tile", sz, ci, ci)
_sig("clo_hip_segfsum_workspace_bytes", sz, sz, sz)
_sig("clo_hip_segfsum", ci, ci, vp, ci, vp, vp, vp, vp, sz, sz, ci, ci, vp, sz, vp)

SEGFSUM_PAIRS = (("half", "float"), ("float", "float"), ("float", "double"), ("double", "double"))   # value -> sum

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}


def segfsum_tile(value_size=4, sum_size=None):
    """T: merge steps (segment ends plus rows) per tile of the kernels for values of value_size and sums of sum_size
    (None: value_size) bytes; 0 for sizes that are not built."""
    return lib.clo_hip_segfsum_tile(value_size, sum_size if sum_size is not None else value_size)


class SegFSum(_Handle):
    """CloSegFSum. form: one of SEGREDUCE_FORMS; (value_type, sum_type): one of SEGFSUM_PAIRS, sum_type None: the
    value type; count_type: uint or ulong, the type of the counts or offsets."""
    _destroy = "clo_segfsum_destroy"

    def __init__(self, form, ctx, value_type="float", sum_type=None, count_type="uint", options=None):
        vt = clo_type(value_type)
        st = clo_type(sum_type) if sum_type is not None else vt
        self._new("clo_segfsum_new", _b(form), _b(options), ctx.h, vt, st, clo_type(count_type))
        self.ctx = ctx

    form = property(lambda self: lib.clo_segfsum_get_form(self.h).decode())
    value_type = property(lambda self: lib.clo_segfsum_get_value_type(self.h))
    value_size = property(lambda self: lib.clo_segfsum_get_value_size(self.h))
    sum_type = property(lambda self: lib.clo_segfsum_get_sum_type(self.h))
    sum_size = property(lambda self: lib.clo_segfsum_get_sum_size(self.h))
    count_type = property(lambda self: lib.clo_segfsum_get_count_type(self.h))
    count_size = property(lambda self: lib.clo_segfsum_get_count_size(self.h))

    def with_device_data(self, q, counts_or_offsets, num_in, values_in, sums_out, num_out, numel_seg, numel, q_comm=None):
        """clo_segfsum_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_segfsum_with_device_data(self.h, _h(q), _h(q_comm), _h(counts_or_offsets), _h(num_in), _h(values_in),
                                               _h(sums_out), _h(num_out), numel_seg, numel, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, counts_or_offsets, values, num_in=None, q_exec=None, q_comm=None):
        """clo_segfsum_with_host_data: (sums, total), sums a numpy array of m = min(numel_seg, num_in) rows of the
        sum type. counts_or_offsets: numel_seg counts or numel_seg + 1 offsets of the object's count type."""
        cdt = np.uint32 if self.count_size == 4 else np.uint64
        c = np.ascontiguousarray(counts_or_offsets)
        if c.ndim != 1 or c.dtype != cdt:
            raise ValueError("counts_or_offsets: a 1-D array of %s" % np.dtype(cdt).name)
        offsets = self.form == "offsets"
        if offsets and c.size == 0:
            raise ValueError("offsets: numel_seg + 1 of them")
        m_h = c.size - 1 if offsets else c.size
        v = np.ascontiguousarray(values)
        if v.ndim != 1 or v.dtype != CLO_TYPE_NP[_TYPE_NAMES[self.value_type]]:
            raise ValueError("values: a 1-D array of the value type")
        so = np.empty(m_h, dtype=CLO_TYPE_NP[_TYPE_NAMES[self.sum_type]])
        m = sz(num_in) if num_in is not None else None
        num = sz(0)
        err = _Err()
        ok = lib.clo_segfsum_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(c), C.byref(m) if m is not None else None,
                                            _p(v) if v.size else None, _p(so) if m_h else None, C.byref(num), m_h, v.size, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_segfsum_with_host_data failed")
        return so[:min(m_h, num_in) if num_in is not None else m_h], num.value
