"""Python view of CloSearch (include/clo_search.h): lower and upper bounds of many keys in a sorted array. A thin
ctypes wrapper like merge.py: every call goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _h, _p, _sig, _E, _u32, _Handle, _keys_1d, clo_type, CloError, CLO_ERROR_LIBRARY

SEARCH_UPPER = 1
SEARCH_NEEDLES_SORTED = 2

_sig("clo_search_new", vp, C.c_char_p, vp, ci, _E)
_sig("clo_search_destroy", None, vp)
_sig("clo_search_with_device_data", vp, vp, vp, vp, vp, sz, vp, sz, C.c_uint, vp, _E)
_sig("clo_search_with_host_data", _u32, vp, vp, vp, vp, sz, vp, sz, C.c_uint, vp, _E)
_sig("clo_search_get_context", vp, vp)
_sig("clo_search_get_key_type", ci, vp)
_sig("clo_search_get_key_size", sz, vp)
_sig("clo_hip_search_tile", sz, ci)
_sig("clo_hip_search_lds_keys", sz, ci)
_sig("clo_hip_search_pivots", sz, ci)
_sig("clo_hip_search_workspace_bytes", sz, sz, sz, C.c_uint)
_sig("clo_hip_search", ci, vp, sz, vp, sz, vp, ci, ci, C.c_uint, C.c_uint, vp, sz, vp)


def search_tile(key_size):
    """Needles per tile of the kernels for keys of key_size bytes; 0 for sizes that are not built."""
    return lib.clo_hip_search_tile(key_size)


def search_lds_keys(key_size):
    """The longest haystack range a work-group keeps in LDS, in keys of key_size bytes; 0 for sizes not built."""
    return lib.clo_hip_search_lds_keys(key_size)


def search_pivots(key_size):
    """Entries of the sampled table the general path keeps in LDS for a longer haystack; 0 for sizes not built."""
    return lib.clo_hip_search_pivots(key_size)


def _flags(upper, needles_sorted):
    return (SEARCH_UPPER if upper else 0) | (SEARCH_NEEDLES_SORTED if needles_sorted else 0)


class Search(_Handle):
    """CloSearch. upper: upper instead of lower bounds; needles_sorted: the caller's promise that the needles ascend."""
    _destroy = "clo_search_destroy"

    def __init__(self, ctx, key_type, options=None):
        self._new("clo_search_new", _b(options), ctx.h, clo_type(key_type))
        self.ctx = ctx

    key_type = property(lambda self: lib.clo_search_get_key_type(self.h))
    key_size = property(lambda self: lib.clo_search_get_key_size(self.h))

    def with_device_data(self, q, haystack, numel_h, needles, numel_n, pos_out, upper=False, needles_sorted=False, q_comm=None):
        """clo_search_with_device_data on Buffers (haystack may be None with numel_h 0); asynchronous on q. Returns
        the event."""
        err = _Err()
        evt = lib.clo_search_with_device_data(self.h, _h(q), _h(q_comm), _h(haystack), numel_h, _h(needles), numel_n,
                                              _flags(upper, needles_sorted), _h(pos_out), err.ref)
        err.raise_if_set()
        return evt

    def with_host_data(self, haystack, needles, upper=False, needles_sorted=False, q_exec=None, q_comm=None):
        """clo_search_with_host_data: the positions as a numpy array of uint32, one per needle."""
        hs, nd = _keys_1d(haystack, self.key_size, "haystack"), _keys_1d(needles, self.key_size, "needles")
        if hs.dtype != nd.dtype:
            raise ValueError("haystack and needles: one dtype")
        pos = np.empty(nd.size, dtype=np.uint32)
        err = _Err()
        ok = lib.clo_search_with_host_data(self.h, _h(q_exec), _h(q_comm), _p(hs), hs.size, _p(nd), nd.size,
                                           _flags(upper, needles_sorted), _p(pos), err.ref)
        err.raise_if_set()
        if not ok:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_search_with_host_data failed")
        return pos
