"""CloSearch (include/clo_search.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the getters answer, every refusal comes back as CLO_ERROR_ARGS through an offline context before
anything touches a device (err == NULL included) and leaves pos_out alone, a call without needles succeeds without a
device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among them
clo_hip_search_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/search_host/search_host_test.c. The reference model the GPU tests compare against (search_model.py) is checked
here against a linear count over Python integers."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from search_model import search, sort_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_search_new", "clo_search_destroy", "clo_search_with_device_data", "clo_search_with_host_data",
          "clo_search_get_context", "clo_search_get_key_type", "clo_search_get_key_size")
THIN = ("clo_hip_search", "clo_hip_search_workspace_bytes", "clo_hip_search_tile", "clo_hip_search_lds_keys", "clo_hip_search_pivots")
KEY_TYPES = ("char", "uchar", "short", "ushort", "int", "uint", "long", "ulong", "half", "float", "double")
UPPER, SORTED = 1, 2


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_search.h")).read()
    for n in PUBLIC + ("CLO_SEARCH_UPPER", "CLO_SEARCH_NEEDLES_SORTED"):
        assert n + "(" in text or "#define " + n in text, n
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_search.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Search", "search_tile", "search_lds_keys", "search_pivots"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_getters():
    for ks in (1, 2, 4, 8):
        T, L, P = clo.search_tile(ks), clo.search_lds_keys(ks), clo.search_pivots(ks)
        assert T >= 64 and T % 64 == 0, (ks, T)
        assert 2 <= P <= L and P & (P - 1) == 0, (ks, P, L)               # the table is halved log2 P times
    for ks in (0, 3, 5, 16, -4):
        assert clo.search_tile(ks) == clo.search_lds_keys(ks) == clo.search_pivots(ks) == 0, ks
    ws = clo.api.lib.clo_hip_search_workspace_bytes
    for flags in range(4):
        for nh in (0, 1, 1 << 20):
            assert ws(nh, 0, flags) == 0
            sizes = [ws(nh, n, flags) for n in (0, 1, 63, 5000, 1 << 20, 1 << 24, (1 << 32) - 1)]
            assert sizes == sorted(sizes) and sizes[-1] < (64 << 20), (flags, nh, sizes)   # monotone, and small next to the data
            assert all(x % 256 == 0 for x in sizes)
    assert ws(1 << 20, 1 << 20, SORTED) > 0                                # the sorted form keeps its ranges there


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for opt in ("descending", "upper", " "):
            assert "options" in _refused(lambda: clo.Search(ctx, "uint", options=opt))
            assert not lib.clo_search_new(opt.encode(), ctx.h, 5, None)     # err NULL
        assert not lib.clo_search_new(None, ctx.h, 11, None)
        assert not lib.clo_search_new(None, ctx.h, -1, None)
        for kt in KEY_TYPES:                                                # every key type, both spellings of no options
            for opt in (None, ""):
                s = clo.Search(ctx, kt, options=opt)
                assert (s.key_type, s.key_size) == (clo.CLO_TYPES[kt], np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize)
                s.close()

        s = clo.Search(ctx, "uint")
        hay, ndl = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        pos = np.arange(100, 132, dtype=np.uint32)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(h, nh, x, nx, flags, out, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_search_with_host_data(s.h, None, None, p(h), nh, p(x), nx, flags, p(out), err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args):
            assert word in host(*args), args
            host(*args, with_err=False)

        for flags in (4, 8, 7, 1 << 31, 0xFFFFFFFC):
            both("flags", hay, 16, ndl, 16, flags, pos)
        both("numel_h", hay, 1 << 32, ndl, 16, 0, pos)
        both("numel_h", hay, 1 << 63, ndl, 16, SORTED, pos)
        both("numel_n", hay, 16, ndl, 1 << 32, UPPER, pos)
        both("numel_n", hay, 16, ndl, (1 << 64) - 1, 0, pos)
        both("haystack", None, 16, ndl, 16, 0, pos)
        both("needles", hay, 16, None, 16, UPPER | SORTED, pos)
        both("needles", None, 0, None, 16, 0, pos)
        both("pos_out", hay, 16, ndl, 16, 0, None)
        both("pos_out", None, 0, ndl, 16, SORTED, None)

        # overlap: pos_out on an input, inside it, across its end, or sharing one element
        one = np.zeros(160, np.uint32)
        O = "overlaps"
        both(O, hay, 16, ndl, 16, 0, hay)                                   # on the haystack
        both(O, hay, 16, ndl, 16, UPPER, ndl)                               # on the needles
        both(O, one[0:64], 64, ndl, 16, 0, one[8:24])                       # inside the haystack
        both(O, hay, 16, one[0:64], 64, 0, one[40:104])                     # inside the needles, to their end
        both(O, one[0:16], 16, ndl, 16, SORTED, one[8:24])                  # across the haystack's end
        both(O, hay, 16, one[32:48], 16, 0, one[40:56])                     # across the needles' end
        both(O, one[0:16], 16, ndl, 16, 0, one[15:31])                      # one shared element with the haystack's end
        both(O, hay, 16, one[32:48], 16, 0, one[17:33])                     # one shared element with the needles' start
        both(O, one[8:24], 16, ndl, 16, 0, one[0:16].view(np.uint32))       # the haystack starts inside pos_out
        h8 = np.zeros(16, np.uint64)
        s8 = clo.Search(ctx, "ulong")
        err = clo.api._Err()                                                # 8-byte keys: the haystack's second half counts
        assert not lib.clo_search_with_host_data(s8.h, None, None, p(h8), 16, p(np.zeros(4, np.uint64)), 4, 0, p(h8) + 120, err.ref)
        assert O in _refused(err.raise_if_set)
        s8.close()
        assert np.array_equal(pos, np.arange(100, 132)) and not one.any() and not hay.any() and not ndl.any()   # nothing was written

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS
        for args in ((one[0:16], 16, one[16:32], 16, 0, one[32:48]),
                     (one[16:32], 16, one[32:48], 16, UPPER | SORTED, one[0:16]),
                     (one[0:16], 16, one[32:48], 16, SORTED, one[16:32])):
            err = clo.api._Err()
            h, nh, x, nx, flags, out = args
            assert not lib.clo_search_with_host_data(s.h, None, None, p(h), nh, p(x), nx, flags, p(out), err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark"
        assert not one.any()

        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            s.with_host_data(np.zeros(4, np.uint16), np.zeros(4, np.uint16))
        with pytest.raises(ValueError):
            s.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.float32))
        s.close()
    finally:
        ctx.close()


def test_no_needles_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for kt in ("float", "uchar", "ulong"):
            dt = clo.api.CLO_TYPE_NP[kt]
            s = clo.Search(ctx, kt)
            for flags in range(4):
                got = s.with_host_data(np.zeros(9, dt), np.zeros(0, dt), upper=bool(flags & UPPER), needles_sorted=bool(flags & SORTED))
                assert got.size == 0 and got.dtype == np.uint32
                # raw: a pos_out that exists is not touched, the inputs may be NULL
                out = np.full(4, 7, np.uint32)
                err = clo.api._Err()
                assert lib.clo_search_with_host_data(s.h, None, None, None, 0, None, 0, flags, out.ctypes.data, err.ref)
                err.raise_if_set()
                assert lib.clo_search_with_host_data(s.h, None, None, None, 0, None, 0, flags, None, None)
                assert (out == 7).all()
            s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "search_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "search_host", "search_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("search host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


_FMT = {"float16": "<e", "float32": "<f", "float64": "<d"}


def _py_order(keys):
    """The order key of every element as a Python integer, from the definition: unsigned by bits, signed by value,
    IEEE by sign and magnitude (negative numbers descend with their magnitude bits)."""
    dt = keys.dtype
    if dt.kind == "u" or dt.kind == "i":
        return [int(x) for x in keys.tolist()]
    bits = 8 * dt.itemsize
    out = []
    for raw in keys.view("u%d" % dt.itemsize).tolist():
        mag = raw & ((1 << (bits - 1)) - 1)
        out.append(-(mag + 1) if raw >> (bits - 1) else mag)     # -0 -> -1 below +0 -> 0
    return out


def _count(haystack, needles, upper):
    """The definition: for every needle a linear count over the haystack, in Python integers."""
    oh, on = _py_order(haystack), _py_order(needles)
    return np.array([sum(1 for h in oh if (h <= x if upper else h < x)) for x in on], dtype=np.uint32)


def _specials(dt):
    """-NaNs (two payloads), -inf, -1, -0, +0, +1, +inf, +NaNs (two payloads), as bits of dtype dt."""
    dt = np.dtype(dt)
    bits = 8 * dt.itemsize
    mant = {16: 10, 32: 23, 64: 52}[bits]
    exp_all = ((1 << (bits - 1)) - 1) ^ ((1 << mant) - 1)
    sign = 1 << (bits - 1)
    one = struct.unpack({16: "<H", 32: "<I", 64: "<Q"}[bits], struct.pack(_FMT[dt.name], 1.0))[0]
    pos = [0, one, exp_all, exp_all | 1, exp_all | (1 << (mant - 1)) | 5]
    return np.array([x | sign for x in pos] + pos, dtype="u%d" % dt.itemsize).view(dt)


def test_the_reference_model():
    rng = np.random.default_rng(12)
    for kt in KEY_TYPES:
        dt = np.dtype(clo.api.CLO_TYPE_NP[kt])
        if dt.kind == "f":
            pool = np.concatenate((_specials(dt), np.array([-2.5, -1e-3, 3.0, 0.5, 7.0], dtype=dt)))
        else:
            info = np.iinfo(dt)
            pool = np.array([info.min, info.max, 0, 1, 5, 6] + ([-1, -2, -7] if dt.kind == "i" else [info.max - 3]), dtype=dt)
        for nh, nn in ((0, 0), (0, 9), (9, 0), (1, 1), (50, 70), (300, 40)):
            hay = sort_keys(pool[rng.integers(0, pool.size, nh)])         # few distinct keys: ties in the haystack and with the needles
            ndl = pool[rng.integers(0, pool.size, nn)]
            for upper in (False, True):
                got = search(hay, ndl, upper)
                assert got.dtype == np.uint32 and got.shape == (nn,)
                assert np.array_equal(got, _count(hay, ndl, upper)), (kt, nh, nn, upper)
            if nh:
                assert (search(hay, ndl, True) >= search(hay, ndl, False)).all()
        # every key of the pool as a needle in the pool itself: upper - lower is the number of matches, 1 each
        ubits = pool.view("u%d" % dt.itemsize)
        hay = sort_keys(pool[np.unique(ubits, return_index=True)[1]])     # (unsigned pools name 0 twice)
        assert np.array_equal(search(hay, hay, False), np.arange(hay.size)) and np.array_equal(search(hay, hay, True), np.arange(hay.size) + 1)
    # equal iff the bits are equal: -0.0 lies below +0.0, NaNs of both signs at the ends, payloads ordered
    for dt in (np.float16, np.float32, np.float64):
        s = _specials(dt)
        hay = sort_keys(s)
        assert np.array_equal(hay.view(np.uint8), np.concatenate((s[:5][::-1], s[5:])).view(np.uint8)), dt
        z = np.array([-0.0, 0.0], dtype=dt)
        assert search(z, z, False).tolist() == [0, 1] and search(z, z, True).tolist() == [1, 2]
        assert search(z[1:], z[:1], True).tolist() == [0] and search(z[:1], z[1:], False).tolist() == [1]
        nan_neg, nan_pos = s[3:4], s[8:9]
        assert search(hay, nan_neg, False).tolist() == [1] and search(hay, nan_neg, True).tolist() == [2]   # below it: the other -NaN only
        assert search(hay, nan_pos, False).tolist() == [8] and search(hay, nan_pos, True).tolist() == [9]
