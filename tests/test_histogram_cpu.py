"""CloHistogram (include/clo_histogram.h) on the CPU: the library exports the new public and thin-ABI entry points and
the headers declare them, the tile and LDS-bin getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves hist_out alone, numel 0 works
without a device in both modes, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c,
among them clo_hip_hist_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/hist_host/hist_host_test.c. The reference model the GPU tests compare against (hist_model.py) is checked here
against np.bincount and against a loop over Python integers."""
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from hist_model import histogram

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_histogram_new", "clo_histogram_destroy", "clo_histogram_with_device_data", "clo_histogram_with_host_data",
          "clo_histogram_get_context", "clo_histogram_get_key_type", "clo_histogram_get_key_size",
          "clo_histogram_get_value_type", "clo_histogram_get_value_size", "clo_histogram_get_sum_type",
          "clo_histogram_get_sum_size", "clo_histogram_get_accumulate")
THIN = ("clo_hip_histogram", "clo_hip_histogram_workspace_bytes", "clo_hip_histogram_tile", "clo_hip_histogram_lds_bins")
INT_KEYS = ("char", "uchar", "short", "ushort", "int", "uint", "long", "ulong")
PAIRS = (("int", "int"), ("int", "uint"), ("uint", "int"), ("uint", "uint"), ("int", "long"), ("int", "ulong"),
         ("uint", "long"), ("uint", "ulong"), ("long", "long"), ("long", "ulong"), ("ulong", "long"), ("ulong", "ulong"))


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_histogram.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_histogram.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Histogram", "histogram_tile", "histogram_lds_bins"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_tile_and_lds_bins_getters():
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.histogram_tile(ks, vs)
            assert t >= 64 and t % 64 == 0, (ks, vs, t)
    assert clo.histogram_tile(3, 4) == 0 and clo.histogram_tile(4, 2) == 0 and clo.histogram_tile(0) == 0
    l4, l8 = clo.histogram_lds_bins(4), clo.histogram_lds_bins(8)
    assert l4 >= 256 and l8 >= 256 and l4 * 4 <= 160 * 1024 and l8 * 8 <= 160 * 1024   # inside a CU's LDS
    assert clo.histogram_lds_bins(2) == 0 and clo.histogram_lds_bins(0) == 0 and clo.histogram_lds_bins(16) == 0
    assert clo.api.lib.clo_hip_histogram_workspace_bytes(1 << 20, 256) < (64 << 20)


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        # at construction: float / half keys, value or sum types outside the four, a sum narrower than the values, options
        for kt in ("float", "double", "half"):
            assert "integers" in _refused(lambda: clo.Histogram(ctx, kt))
            assert not lib.clo_histogram_new(None, ctx.h, clo.clo_type(kt), 5, 5, None)   # err NULL
        assert not lib.clo_histogram_new(None, ctx.h, 11, 5, 5, None)
        for vt, st in (("float", "float"), ("uint", "float"), ("uint", "double"), ("half", "uint"), ("double", "ulong"),
                       ("ushort", "uint"), ("short", "int"), ("uchar", "uint"), ("char", "long"), ("uint", "ushort"),
                       ("ulong", "uint"), ("long", "int")):
            _refused(lambda: clo.Histogram(ctx, "uint", vt, st))
            assert not lib.clo_histogram_new(None, ctx.h, 5, clo.clo_type(vt), clo.clo_type(st), None)
        for opt in ("tile=1", "Accumulate", "accumulate ", "accumulate,accumulate"):
            assert "options" in _refused(lambda: clo.Histogram(ctx, "uint", options=opt))
            assert not lib.clo_histogram_new(opt.encode(), ctx.h, 5, 5, 5, None)
        # what is offered: every integer key type, every value -> sum pair, both modes
        for kt in INT_KEYS:
            for opt, acc in ((None, False), ("", False), ("accumulate", True)):
                h = clo.Histogram(ctx, kt, options=opt)
                assert h.accumulate is acc and h.key_size == np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize
                h.close()
        for vt, st in PAIRS:
            h = clo.Histogram(ctx, "short", vt, st)
            assert (h.key_size, h.value_size, h.sum_size) == (2, np.dtype(clo.api.CLO_TYPE_NP[vt]).itemsize,
                                                              np.dtype(clo.api.CLO_TYPE_NP[st]).itemsize)
            h.close()

        # per call, through the host-data form (nothing is copied before the checks)
        h = clo.Histogram(ctx, "uint", "uint", "uint")
        h8 = clo.Histogram(ctx, "uchar", "uint", "ulong", options="accumulate")
        k, v = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        k8 = np.zeros(16, np.uint8)
        out = np.arange(100, 116, dtype=np.uint32)
        out8 = np.arange(100, 116, dtype=np.uint64)
        p = lambda a: a.ctypes.data if a is not None else None

        def host(obj, kin, vin, o, n, shift, nb, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_histogram_with_host_data(obj.h, None, None, p(kin), p(vin), p(o), n, None, shift, nb,
                                                  err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(obj, kin, vin, o, n, shift, nb, word):
            assert word in host(obj, kin, vin, o, n, shift, nb)
            host(obj, kin, vin, o, n, shift, nb, with_err=False)

        both(h, k, v, out, 1 << 32, 0, 16, "numel")
        both(h, k, v, out, 16, 0, 0, "num_bins")
        both(h, k, v, out, 16, 0, 1 << 32, "num_bins")
        both(h, k, v, out, 16, 32, 16, "shift")
        both(h, k, v, out, 16, 40, 16, "shift")
        both(h8, k8, v, out8, 16, 8, 16, "shift")
        both(h, None, v, out, 16, 0, 16, "keys_in")
        both(h, k, v, None, 16, 0, 16, "hist_out")
        # overlap: hist_out on, inside, or across the end of an input
        both(h, k, v, k, 16, 0, 16, "overlaps")
        both(h, k, v, v, 16, 0, 16, "overlaps")
        one = np.zeros(40, np.uint32)
        both(h, one[:16], v, one[15:31], 16, 0, 16, "overlaps")        # one shared element
        both(h, one[8:24], v, one[0:16], 16, 0, 16, "overlaps")        # ends inside the keys
        both(h, k, one[16:32], one[17:33], 16, 0, 16, "overlaps")
        both(h, k, one[16:32], one[10:20], 16, 0, 10, "overlaps")      # num_bins, not numel, sizes the output range
        assert np.array_equal(out, np.arange(100, 116)) and np.array_equal(out8, np.arange(100, 116))   # nothing was written
        assert not one.any() and not k.any() and not v.any()
        # what is next to an input without touching it is accepted as far as the checks go: the call then fails for
        # want of a device, not with CLO_ERROR_ARGS
        err = clo.api._Err()
        assert not lib.clo_histogram_with_host_data(h.h, None, None, p(one[:16]), None, p(one[16:32]), 16, None, 31, 16, err.ref)
        with pytest.raises(clo.CloError) as e:
            err.raise_if_set()
        assert e.value.domain == "ccl-hip-error-quark"
        with pytest.raises(ValueError):   # the Python view checks the element sizes
            h.with_host_data(np.zeros(4, np.uint16), num_bins=4)
        with pytest.raises(ValueError):
            h.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint64), num_bins=4)
        with pytest.raises(ValueError):
            h.with_host_data(np.zeros(4, np.uint32), num_bins=4, out=np.zeros(4, np.uint64))
        h.close()
        h8.close()
    finally:
        ctx.close()


def test_numel_0_without_a_device():
    ctx = clo.Context(offline=True)
    try:
        for st, dt in (("uint", np.uint32), ("long", np.int64)):
            h = clo.Histogram(ctx, "int", "int", st)
            out = np.arange(7, 20, dtype=dt)
            got = h.with_host_data(np.zeros(0, np.int32), num_bins=13, out=out, lower=-5, shift=3)
            assert got is out and not out.any()                      # zeroed
            assert not h.with_host_data(np.zeros(0, np.int32), np.zeros(0, np.int32), num_bins=3).any()
            h.close()
            h = clo.Histogram(ctx, "int", "int", st, options="accumulate")
            out = np.arange(7, 20, dtype=dt)
            h.with_host_data(np.zeros(0, np.int32), num_bins=13, out=out)
            assert np.array_equal(out, np.arange(7, 20))             # left alone
            h.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "hist_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "hist_host", "hist_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("hist host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(keys, values, sum_dtype, lower, shift, num_bins):
    """The definition, element by element, on Python integers."""
    bits = 8 * np.dtype(sum_dtype).itemsize
    h = [0] * num_bins
    for i, k in enumerate(keys.tolist()):
        d = k - lower
        if d >= 0 and (d >> shift) < num_bins:
            h[d >> shift] += 1 if values is None else int(values[i])
    return np.array([x % (1 << bits) for x in h], dtype=np.dtype("u%d" % (bits // 8))).view(sum_dtype)


def test_the_reference_model():
    rng = np.random.default_rng(5)
    # unsigned keys against np.bincount (weights: exact in float64 below 2^53)
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
        keys = rng.integers(0, 200, 5000).astype(dt)
        vals = rng.integers(0, 1 << 20, 5000, dtype=np.uint32)
        assert np.array_equal(histogram(keys, None, np.uint32, 0, 0, 200), np.bincount(keys.astype(np.int64), minlength=200).astype(np.uint32))
        w = np.bincount(keys.astype(np.int64), weights=vals.astype(np.float64), minlength=200)
        assert np.array_equal(histogram(keys, vals, np.uint64, 0, 0, 200), w.astype(np.uint64))
        # a lower bound, a shift and fewer bins than keys: bincount of the shifted keys, cut
        sel = (keys >= 10) & (((keys.astype(np.int64) - 10) >> 2) < 30)
        want = np.bincount((keys[sel].astype(np.int64) - 10) >> 2, minlength=30).astype(np.uint64)
        assert np.array_equal(histogram(keys, None, np.uint64, 10, 2, 30), want)
    # 32-bit sums wrap, 64-bit ones do not; int -> long sign-extends, uint -> long zero-extends
    keys = rng.integers(0, 4, 3000, dtype=np.uint32)
    big = rng.integers((1 << 32) - 1000, 1 << 32, 3000, dtype=np.uint32)
    assert np.array_equal(histogram(keys, big, np.uint32, 0, 0, 4), _loop(keys, big, np.uint32, 0, 0, 4))
    h64 = histogram(keys, big, np.uint64, 0, 0, 4)
    assert np.array_equal(h64, _loop(keys, big, np.uint64, 0, 0, 4)) and (h64 > np.uint64(1 << 32)).all()
    neg = big.view(np.int32)
    assert (neg < 0).all()
    assert np.array_equal(histogram(keys, neg, np.int64, 0, 0, 4), _loop(keys, neg, np.int64, 0, 0, 4))
    assert (histogram(keys, neg, np.int64, 0, 0, 4) < 0).all() and (histogram(keys, big, np.int64, 0, 0, 4) > 0).all()
    # an accumulating call adds onto what is there
    onto = np.array([5, 6, 7, 8], np.uint32)
    assert np.array_equal(histogram(keys, None, np.uint32, 0, 0, 4, onto=onto), onto + np.bincount(keys, minlength=4).astype(np.uint32))
    # signed keys with a negative lower, and lower at the type's minimum, against the loop
    for dt in (np.int8, np.int16, np.int32, np.int64):
        info = np.iinfo(dt)
        keys = rng.integers(-100, 100, 4000).astype(dt)
        vals = rng.integers(-1 << 31, 1 << 31, 4000).astype(np.int32)
        for lower, shift, nb in ((-50, 0, 70), (-100, 3, 25), (-7, 1, 3), (info.min, 0, 60), (info.min, info.bits - 1, 2), (info.min, info.bits - 1, 1)):
            k = keys if lower != info.min or shift else (keys.astype(np.int64) % 80 + info.min).astype(dt)
            assert np.array_equal(histogram(k, None, np.uint32, lower, shift, nb), _loop(k, None, np.uint32, lower, shift, nb)), (dt, lower, shift, nb)
            assert np.array_equal(histogram(k, vals, np.int64, lower, shift, nb), _loop(k, vals, np.int64, lower, shift, nb)), (dt, lower, shift, nb)
    # the wrap trap: lower + (num_bins << shift) runs past the type's maximum; keys below lower, whose difference
    # modulo 2^B would fall inside the range, are not counted
    for dt, lower in ((np.uint8, 250), (np.int32, (1 << 31) - 100), (np.uint64, (1 << 64) - 100), (np.int64, (1 << 63) - 100), (np.uint16, 65500)):
        info = np.iinfo(dt)
        nb = 256
        below = (np.arange(200) % 120 + (info.min if dt != np.uint8 else 0)).astype(dt)           # wrapped differences 6 .. 255 or 100 ..
        inside = np.array([lower, info.max, lower + 1], dtype=object).astype(dt)
        keys = np.concatenate((below, inside, below))
        got = histogram(keys, None, np.uint32, lower, 0, nb)
        assert np.array_equal(got, _loop(keys, None, np.uint32, lower, 0, nb)) and got.sum() == 3, (dt, got.sum())
        wrapped = (keys.astype(object) - lower) % (1 << info.bits)
        assert sum(1 for x in wrapped if x < nb) > 3           # without the test key >= lower more would be counted
    # nothing counted
    assert not histogram(np.full(100, 5, np.uint32), None, np.uint32, 6, 0, 10).any()
    assert not histogram(np.zeros(0, np.uint32), None, np.uint64, 0, 0, 10).any()
