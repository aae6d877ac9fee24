"""Python view of CloSegTopK (include/clo_segtopk.h): the k smallest or largest rows of every segment, the segments given
by counts or by CSR offsets. A thin ctypes wrapper like segsort.py: every call goes through the C API, nothing is computed
in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, clo_type, CloError, CLO_ERROR_LIBRARY, CLO_TYPES, CLO_TYPE_NP

_sig("clo_segtopk_new", vp, C.c_char_p, C.c_char_p, C.c_char_p, vp, ci, sz, ci, _E)
_sig("clo_segtopk_destroy", None, vp)
_sig("clo_segtopk_with_device_data", vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, _E)
_sig("clo_segtopk_with_host_data", _u32, vp, vp, vp, vp, C.POINTER(sz), vp, vp, vp, vp, vp, C.POINTER(sz), sz, sz, sz, _E)
_sig("clo_segtopk_get_context", vp, vp)
_sig("clo_segtopk_get_which", C.c_char_p, vp)
_sig("clo_segtopk_get_form", C.c_char_p, vp)
_sig("clo_segtopk_get_key_type", ci, vp)
_sig("clo_segtopk_get_key_size", sz, vp)
_sig("clo_segtopk_get_value_size", sz, vp)
_sig("clo_segtopk_get_count_type", ci, vp)
_sig("clo_segtopk_get_count_size", sz, vp)
_sig("clo_hip_segtopk_tile", sz, ci, ci)
_sig("clo_hip_segtopk_k_max", sz, ci, ci)
_sig("clo_hip_segtopk_workspace_bytes", sz, sz, sz, sz, ci, ci)
_sig("clo_hip_segtopk", ci, ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, ci, ci, vp, sz, vp)

SEGTOPK_WHICH = ("smallest", "largest")   # the thin ABI's numbers, in order

_TYPE_NAMES = {v: k for k, v in CLO_TYPES.items()}


def segtopk_tile(key_size=4, value_size=0):
    """T: rows per tile of the kernels for keys of key_size and values of value_size bytes (a segment inside one tile is
    finished by one launch); 0 for sizes that are not built."""
    return lib.clo_hip_segtopk_tile(key_size, value_size)


def segtopk_k_max(key_size=4, value_size=0):
    """The largest k a call takes for keys of key_size and values of value_size bytes; 0 for sizes that are not built."""
    return lib.clo_hip_segtopk_k_max(key_size, value_size)


class SegTopK(_Handle):
    """CloSegTopK. which: one of SEGTOPK_WHICH; form: one of SEGREDUCE_FORMS; value_size: 0 (keys only), 4 or 8;
    count_type: uint or ulong, the type of the counts or offsets."""
    _destroy = "clo_segtopk_destroy"

    def __init__(self, which, form, ctx, key_type="uint", value_size=0, count_type="uint", options=None):
        self._new("clo_segtopk_new", _b(which), _b(form), _b(options), ctx.h, clo_type(key_type), value_size, clo_type(count_type))
        self.ctx = ctx

    which = property(lambda self: lib.clo_segtopk_get_which(self.h).decode())
    form = property(lambda self: lib.clo_segtopk_get_form(self.h).decode())
    key_type = property(lambda self: lib.clo_segtopk_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_segtopk_get_key_size(self.h))
    value_size = property(lambda self: lib.clo_segtopk_get_value_size(self.h))
    count_type = property(lambda self: lib.clo_segtopk_get_count_type(self.h))
    count_size = property(lambda self: lib.clo_segtopk_get_count_size(self.h))

    def with_device_data(self, q, counts_or_offsets, num_in, keys_in, values_in, keys_out, values_out, counts_out, num_out,
                         numel_seg, numel, k, q_comm=None):
        """clo_segtopk_with_device_data on Buffers (any of which may be None where the contract allows NULL);
        asynchronous on q. Returns the event."""
        err = _Err()
        evt = lib.clo_segtopk_with_device_data(self.h, _h(q), _h(q_comm), _h(counts_or_offsets), _h(num_in), _h(keys_in), _h(values_in),
                                               _h(keys_out), _h(values_out), _h(counts_out), _h(num_out), numel_seg, numel, k, err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, counts_or_offsets, keys, k, values=None, num_in=None, q_exec=None, q_comm=None, keys_out=True, fill=0):
        """clo_segtopk_with_host_data: (keys_out[m, k], values_out[m, k], counts[m], total) with m = min(numel_seg,
        num_in). values_out is None with value_size 0, keys_out with keys_out=False (which the arg form allows). values
        None with value_size 4: the arg form, values_out the global row indices as uint32. Slots j >= counts[r] of row r
        are not written by the call: they hold `fill` converted to the output's type as a C cast converts it (-1 is all
        ones in every integer type and -1.0 in a floating-point one); so do counts[r] for r >= m, which are not returned."""
        cdt = np.uint32 if self.count_size == 4 else np.uint64
        c = np.ascontiguousarray(counts_or_offsets)
        if c.ndim != 1 or c.dtype != cdt:
            raise ValueError("counts_or_offsets: a 1-D array of %s" % np.dtype(cdt).name)
        offsets = self.form == "offsets"
        if offsets and c.size == 0:
            raise ValueError("offsets: numel_seg + 1 of them")
        m_h = c.size - 1 if offsets else c.size
        kk = np.ascontiguousarray(keys)
        if kk.ndim != 1 or kk.dtype != CLO_TYPE_NP[_TYPE_NAMES[self.key_type]]:
            raise ValueError("keys: a 1-D array of the key type")
        vs = self.value_size
        v = None
        if values is not None:
            v = np.ascontiguousarray(values)
            if v.ndim != 1 or v.dtype.itemsize != vs or v.size != kk.size:
                raise ValueError("values: a 1-D array of as many rows as the keys, of itemsize value_size")
        k = int(k)
        # (at least one element: an empty numpy array may have no address, and a NULL output is refused)
        rows = max(m_h * k, 1)
        def filled(count, dt):   # (np.full itself refuses a number the type cannot hold)
            with np.errstate(all="ignore"):
                return np.full(count, np.array(fill).astype(dt), dt)
        ko = filled(rows, kk.dtype) if keys_out else None
        vo = filled(rows, v.dtype if v is not None else np.uint32) if vs else None
        co = filled(max(m_h, 1), np.uint32)
        m = sz(num_in) if num_in is not None else None
        num = sz(0)
        err = _Err()
        ok = lib.clo_segtopk_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(c), C.byref(m) if m is not None else None,
                                            _p(kk) if kk.size else None, _p(v if v.size else np.zeros(1, v.dtype)) if v is not None else None,
                                            _p(ko) if ko is not None else None, _p(vo) if vo is not None else None, _p(co),
                                            C.byref(num), m_h, kk.size, k, err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_segtopk_with_host_data failed")
        mm = min(m_h, num_in) if num_in is not None else m_h
        shape = lambda a: a[:mm * k].reshape(mm, k) if a is not None else None
        return shape(ko), shape(vo), co[:mm], num.value
