"""Python view of CloSegArg (include/clo_segarg.h): where the minimum or maximum of every segment lies, and its value,
the segments given by counts or by CSR offsets. A thin ctypes wrapper like segreduce.py: every call goes through the C
API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_segarg_new", vp, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, vp, ci, ci, _E)
_sig("clo_segarg_destroy", None, vp)
_sig("clo_segarg_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, _E)
_sig("clo_segarg_with_host_data", _u32, vp, vp, vp, vp, C.POINTER(sz), vp, vp, vp, C.POINTER(sz), sz, sz, _E)
_sig("clo_segarg_get_context", vp, vp)
_sig("clo_segarg_get_op", C.c_char_p, vp)
_sig("clo_segarg_get_tie", C.c_char_p, vp)
_sig("clo_segarg_get_form", C.c_char_p, vp)
_sig("clo_segarg_get_value_type", ci, vp)
_sig("clo_segarg_get_value_size", sz, vp)
_sig("clo_segarg_get_count_type", ci, vp)
_sig("clo_segarg_get_count_size", sz, vp)
_sig("clo_hip_segarg_tile", sz, ci)
_sig("clo_hip_segarg_carry_tiles", sz)
_sig("clo_hip_segarg_workspace_bytes", sz, sz, sz)
_sig("clo_hip_segarg", ci, ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, sz, sz, ci, vp, sz, vp)

SEGARG_OPS = ("argmin", "argmax")   # the thin ABI's op numbers, in order
SEGARG_TIES = ("first", "last")     # and its tie numbers
SEGARG_NONE = 0xffffffff            # idx_out of a segment without a row

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}


def segarg_tile(value_size=4):
    """T: merge steps (segment ends plus rows) per tile of the kernels for values of value_size bytes; 0 for sizes that
    are not built."""
    return lib.clo_hip_segarg_tile(value_size)


def segarg_carry_tiles():
    """How many tiles' open aggregates the one work-group of the carry scan takes per trip."""
    return lib.clo_hip_segarg_carry_tiles()


class SegArg(_Handle):
    """CloSegArg. op: one of SEGARG_OPS; tie: one of SEGARG_TIES; form: one of SEGREDUCE_FORMS. value_type: int, uint,
    long, ulong, float or double. count_type: uint or ulong, the type of the counts or offsets."""
    _destroy = "clo_segarg_destroy"

    def __init__(self, op, tie, form, ctx, value_type="uint", count_type="uint", options=None):
        self._new("clo_segarg_new", _b(op), _b(tie), _b(form), _b(options), ctx.h, clo_type(value_type), clo_type(count_type))
        self.ctx = ctx

    op = property(lambda self: lib.clo_segarg_get_op(self.h).decode())
    tie = property(lambda self: lib.clo_segarg_get_tie(self.h).decode())
    form = property(lambda self: lib.clo_segarg_get_form(self.h).decode())
    value_type = property(lambda self: lib.clo_segarg_get_value_type(self.h))
    value_size = property(lambda self: lib.clo_segarg_get_value_size(self.h))
    count_type = property(lambda self: lib.clo_segarg_get_count_type(self.h))
    count_size = property(lambda self: lib.clo_segarg_get_count_size(self.h))

    def with_device_data(self, q, counts_or_offsets, num_in, values_in, idx_out, val_out, num_out, numel_seg, numel, q_comm=None):
        """clo_segarg_with_device_data on Buffers (any of which may be None where the contract allows NULL); asynchronous
        on q. Returns the event."""
        err = _Err()
        evt = lib.clo_segarg_with_device_data(self.h, _h(q), _h(q_comm), _h(counts_or_offsets), _h(num_in), _h(values_in),
                                              _h(idx_out), _h(val_out), _h(num_out), numel_seg, numel, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, counts_or_offsets, values, num_in=None, want_values=True, q_exec=None, q_comm=None):
        """clo_segarg_with_host_data: (idx, vals, total), idx a numpy array of m = min(numel_seg, num_in) uint32 row
        indices (SEGARG_NONE for a segment without a row), vals the m values of the value type or None when want_values
        is False. counts_or_offsets: numel_seg counts or numel_seg + 1 offsets of the object's count type."""
        cdt = np.uint32 if self.count_size == 4 else np.uint64
        c = np.ascontiguousarray(counts_or_offsets)
        if c.ndim != 1 or c.dtype != cdt:
            raise ValueError("counts_or_offsets: a 1-D array of %s" % np.dtype(cdt).name)
        offsets = self.form == "offsets"
        if offsets and c.size == 0:
            raise ValueError("offsets: numel_seg + 1 of them")
        m_h = c.size - 1 if offsets else c.size
        vdt = CLO_TYPE_NP[_TYPE_NAMES[self.value_type]]
        v = np.ascontiguousarray(values)
        if v.ndim != 1 or v.dtype != vdt:
            raise ValueError("values: a 1-D array of the value type")
        io = np.empty(m_h, dtype=np.uint32)
        vo = np.empty(m_h, dtype=vdt) if want_values else None
        m = sz(num_in) if num_in is not None else None
        num = sz(0)
        err = _Err()
        ok = lib.clo_segarg_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(c), C.byref(m) if m is not None else None,
                                           _p(v) if v.size else None, _p(io) if m_h else None,
                                           _p(vo) if want_values and m_h else None, C.byref(num), m_h, v.size, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_segarg_with_host_data failed")
        rows = min(m_h, num_in) if num_in is not None else m_h
        return io[:rows], vo[:rows] if want_values else None, num.value
