"""Python view of CloRng (include/clo_rng.h): device random number generators with upstream's seeding
(src/cl_ops/rng/clo_rng.in.h:44-111) and the bulk fill clo_rng_fill. A thin ctypes wrapper like api.py: every call
goes through the C API, nothing is computed in Python."""
import ctypes as C

import numpy as np

from ._hip import lib, vp, sz, ci
from .api import _Err, _b, _sig, _E, Buffer, CloError, CLO_ERROR_LIBRARY


class RngInfo(C.Structure):
    _fields_ = [("name", C.c_char_p), ("src", C.c_char_p), ("seed_size", sz)]


_sig("clo_rng_get_infos", C.POINTER(RngInfo))
_sig("clo_rng_new", vp, C.c_char_p, ci, vp, sz, C.c_uint64, C.c_char_p, vp, vp, _E)
_sig("clo_rng_destroy", None, vp)
_sig("clo_rng_get_source", C.c_char_p, vp)
_sig("clo_rng_get_device_seeds", vp, vp)
_sig("clo_rng_get_size", sz, vp)
_sig("clo_rng_fill", vp, vp, vp, vp, sz, C.c_uint, C.c_uint, _E)

# CloRngSeedType, clo_rng.in.h:77-91
SEED_TYPES = {"dev_gid": 0, "host_mt": 1, "ext_dev": 2, "ext_host": 3}

# state dtype and per-state shape of each generator (include/clo_rng/clo_rng_device.hpp)
STATE_LAYOUT = {"lcg": (np.uint64, ()), "xorshift64": (np.uint64, ()), "xorshift128": (np.uint32, (4,)),
                "mwc64x": (np.uint32, (2,)), "parkmiller": (np.int32, ()), "tauslcg": (np.uint32, (4,))}


def rng_names():
    """The generators, in CLO_RNG_IMPLS order, as clo_rng_infos lists them."""
    p = lib.clo_rng_get_infos()
    out, i = [], 0
    while p[i].name:
        out.append(p[i].name.decode())
        i += 1
    return out


def rng_infos():
    """[(name, src, seed_size)] of clo_rng_infos."""
    p = lib.clo_rng_get_infos()
    out, i = [], 0
    while p[i].name:
        out.append((p[i].name.decode(), p[i].src.decode(), p[i].seed_size))
        i += 1
    return out


def _seed_type(t):
    return SEED_TYPES[t] if isinstance(t, str) else int(t)


class Rng:
    """CloRng. seed_type: 'dev_gid' (hash applies), 'host_mt', 'ext_host' (seeds: a numpy array of the seed
    bytes) or 'ext_dev' (seeds: a Buffer the caller keeps and frees)."""

    def __init__(self, type, ctx, queue, seed_type="dev_gid", seeds=None, seeds_count=1 << 16, main_seed=0, hash=None):
        st = _seed_type(seed_type)
        self._keep = None
        if seeds is None:
            sp = None
        elif isinstance(seeds, Buffer):
            sp = seeds.h
        else:
            self._keep = np.ascontiguousarray(seeds)
            sp = self._keep.ctypes.data_as(vp)
        err = _Err()
        self.h = lib.clo_rng_new(_b(type), st, sp, seeds_count, main_seed, _b(hash), ctx.h if ctx else None,
                                 queue.h if queue else None, err.ref)
        err.raise_if_set()
        if not self.h:
            raise CloError("clo", CLO_ERROR_LIBRARY, "clo_rng_new returned NULL")
        self._keep = None   # EXT_HOST seeds were copied by clo_rng_new
        self.type, self.ctx, self.seeds_count = type, ctx, seeds_count

    @property
    def source(self):
        return lib.clo_rng_get_source(self.h).decode()

    @property
    def size(self):
        return lib.clo_rng_get_size(self.h)

    @property
    def device_seeds(self):
        """The CCLBuffer* of the states (a raw handle)."""
        return lib.clo_rng_get_device_seeds(self.h)

    def fill(self, queue, out, numel, bits=32, maxint=0):
        """clo_rng_fill into `out`: a Buffer, a torch tensor on the device, or a raw device pointer (int) to at least
        numel uint32 values. Returns the event."""
        wrap = None
        if isinstance(out, Buffer):
            bh = out.h
        elif out is None:
            bh = None
        else:
            ptr = out.data_ptr() if hasattr(out, "data_ptr") else int(out)
            nbytes = out.numel() * out.element_size() if hasattr(out, "numel") else numel * 4
            wrap = Buffer(self.ctx, nbytes, device_ptr=ptr)
            bh = wrap.h
        try:
            err = _Err()
            evt = lib.clo_rng_fill(self.h, queue.h if queue else None, bh, numel, bits, maxint, err.ref)
            err.raise_if_set()
            return evt
        finally:
            if wrap is not None:
                wrap.close()   # (a wrapper only: the memory is the caller's)

    def states(self, queue):
        """The generator states now, as numpy: (seeds_count,) or (seeds_count, k) of the state's dtype."""
        dt, shape = STATE_LAYOUT[self.type]
        n = self.size // np.dtype(dt).itemsize
        out = np.empty(n, dtype=dt)
        err = _Err()
        lib.ccl_buffer_enqueue_read(self.device_seeds, queue.h, 1, 0, out.nbytes, out.ctypes.data_as(vp), None, err.ref)
        err.raise_if_set()
        return out.reshape((self.seeds_count,) + shape)

    def close(self):
        if self.h:
            lib.clo_rng_destroy(self.h)
            self.h = None
