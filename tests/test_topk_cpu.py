"""CloTopK (include/clo_topk.h) on the CPU: the library exports the new public and thin-ABI entry points and the headers
declare them, the tile, workspace and sorted-cap getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs alone, numel == 0 and
k == 0 succeed without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c,
among them clo_hip_topk_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/topk_host/topk_host_test.c. The reference model the GPU tests compare against (topk_model.py) is checked here
against a plain Python loop over Python integers, for every key type on its special values, both directions, and k
cutting inside a tie run."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from cl_ops_amd.topk import TOPK_WHICH, TOPK_ORDERS, TOPK_SCAN_TRIP
from topk_model import WHICH, ORDERS, topk
from test_merge_cpu import KEY_TYPES, _py_order, _specials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_topk_new", "clo_topk_destroy", "clo_topk_with_device_data", "clo_topk_with_host_data",
          "clo_topk_get_context", "clo_topk_get_key_type", "clo_topk_get_key_size", "clo_topk_get_value_size",
          "clo_topk_get_which", "clo_topk_get_order")
THIN = ("clo_hip_topk", "clo_hip_topk_workspace_bytes", "clo_hip_topk_tile", "clo_hip_topk_sweep_groups", "clo_hip_topk_sorted_max")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_topk.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_TOPK_WHICH "smallest, largest"' in text
    assert '#define CLO_TOPK_ORDERS "input, sorted"' in text
    assert ", ".join(TOPK_WHICH) == "smallest, largest" == ", ".join(WHICH)
    assert ", ".join(TOPK_ORDERS) == "input, sorted" == ", ".join(ORDERS)
    assert clo.TOPK_WHICH is TOPK_WHICH and clo.TOPK_ORDERS is TOPK_ORDERS
    assert "clo_select.h" in text and "out of scope" in text.lower()          # refers to select's out-of-scope line; says what stays out
    assert "top-k" in open(os.path.join(ROOT, "include", "clo_select.h")).read()
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(TOPK_WHICH):                                          # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_TOPK_%s %d\n" % (n.upper().ljust(8), i) in text, n
    for i, n in enumerate(TOPK_ORDERS):
        assert "#define CLO_HIP_TOPK_%s %d\n" % (n.upper().ljust(6), i) in text, n
    assert "#define CLO_HIP_TOPK_SCAN_TRIP %d\n" % TOPK_SCAN_TRIP in text
    assert '#include "clo_topk.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("TopK", "topk_tile", "topk_sweep_groups", "topk_sorted_max", "TOPK_WHICH", "TOPK_ORDERS"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_tile_workspace_and_sorted_max_getters():
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.topk_tile(ks, vs)
            assert t >= 1024 and t % 1024 == 0, (ks, vs, t)                   # whole rows of 256 lanes x 4 elements
            assert clo.topk_sorted_max(ks, vs) >= 1024, (ks, vs)
    for ks, vs in ((3, 0), (0, 0), (16, 4), (4, 2), (4, 1), (8, 16), (4, -4)):
        assert clo.topk_tile(ks, vs) == 0 and clo.topk_sorted_max(ks, vs) == 0, (ks, vs)
    ws = clo.api.lib.clo_hip_topk_workspace_bytes
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            assert ws(0, ks, vs) == 0
            sizes = [ws(n, ks, vs) for n in (0, 1, 63, 5000, 8192, 8193, 1 << 20, 1 << 24, (1 << 32) - 1)]
            assert sizes == sorted(sizes) and sizes[1] > 0 and sizes[-1] < (16 << 20), (ks, vs, sizes)   # monotone, small next to the data
            assert sizes[7] < (1 << 24) * ks // 64, (ks, vs, sizes)
            assert all(s % 256 == 0 for s in sizes)
            t = clo.topk_tile(ks, vs)
            for n in (1, t, t + 1, 100 * t + 5):                            # room for two counts per tile and the totals
                assert ws(n, ks, vs) >= 8 * (-(-n // t) + 1), (ks, vs, n)
    assert ws(1000, 3, 0) == 0 and ws(1000, 4, 2) == 0                      # sizes not built


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        # at construction: which, order, value sizes, options, key types
        for which in ("", "least", "Smallest", "smallest ", "min", None):
            assert "top-k which" in _refused(lambda: clo.TopK(which, "input", ctx, "uint", 0))
            assert not lib.clo_topk_new(which.encode() if which is not None else None, b"input", None, ctx.h, 5, 0, None)   # err NULL
        for order in ("", "index", "Sorted", "sort", "descending", None):
            assert "top-k order" in _refused(lambda: clo.TopK("smallest", order, ctx, "uint", 0))
            assert not lib.clo_topk_new(b"smallest", order.encode() if order is not None else None, None, ctx.h, 5, 0, None)
        for vs in (1, 2, 3, 5, 12, 16):
            assert "value_size" in _refused(lambda: clo.TopK("smallest", "input", ctx, "uint", vs))
            assert not lib.clo_topk_new(b"smallest", b"input", None, ctx.h, 5, vs, None)
        for opt in ("descending", "k=5", " "):
            assert "options" in _refused(lambda: clo.TopK("smallest", "input", ctx, "uint", 0, options=opt))
            assert not lib.clo_topk_new(b"smallest", b"input", opt.encode(), ctx.h, 5, 0, None)
        assert not lib.clo_topk_new(b"smallest", b"input", None, ctx.h, 11, 0, None)
        for which in WHICH:                                                  # every direction, order, key type, value size, both spellings of no options
            for order in ORDERS:
                for kt in KEY_TYPES:
                    for vs, opt in ((0, None), (4, ""), (8, None)):
                        s = clo.TopK(which, order, ctx, kt, vs, options=opt)
                        assert (s.which, s.order, s.key_type, s.key_size, s.value_size) == \
                            (which, order, clo.CLO_TYPES[kt], np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize, vs)
                        s.close()

        s0, s4, s8 = clo.TopK("smallest", "input", ctx, "uint", 0), clo.TopK("largest", "input", ctx, "uint", 4), clo.TopK("smallest", "input", ctx, "uint", 8)
        so = clo.TopK("largest", "sorted", ctx, "uint", 4)
        cap = clo.topk_sorted_max(4, 4)
        a, va = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        va8 = np.zeros(16, np.uint64)
        ko, vo = np.arange(100, 116, dtype=np.uint32), np.arange(200, 216, dtype=np.uint32)
        vo8 = np.arange(300, 316, dtype=np.uint64)
        kth = np.full(2, 777, np.uint32)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(obj, keys, vals, out_k, out_v, out_kth=None, n=16, k=8, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_topk_with_host_data(obj.h, None, None, p(keys), p(vals), p(out_k), p(out_v), p(out_kth), n, k, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), args
            host(*args, with_err=False, **kw)

        both("2^32", s0, a, None, ko, None, n=1 << 32)
        both("2^32", s4, a, va, ko, vo, kth, n=(1 << 32) + 5, k=1)
        both("2^32", s8, a, va8, ko, vo8, n=1 << 63)
        both("keys_in", s0, None, None, ko, None)
        both("keys_in", s4, None, None, None, vo)                            # ... in the arg form without keys_out too
        both("keys_in", s0, None, None, None, None, kth)                     # ... and for the k-th key alone
        both("value_size 0", s0, a, va, ko, None)                            # values with value_size 0
        both("value_size 0", s0, a, None, ko, vo)
        both("values_out", s4, a, va, ko, None)                              # values_out NULL with value_size > 0
        both("values_out", s4, a, None, ko, None, kth)
        both("value_size of 4", s8, a, None, ko, vo8)                        # NULL values with value_size 8
        both("both NULL", s0, a, None, None, None)                           # both outputs NULL and no kth_out
        both("aligned", s0, a, None, ko, None, kth.view(np.uint8)[1:5])      # kth_out misaligned
        both("aligned", s0, a, None, None, None, kth.view(np.uint8)[2:6])
        both("cap", so, a, va, ko, vo, n=cap + 100, k=cap + 1)               # "sorted" with m above the cap (nothing is read)
        both("cap", so, a, None, ko, vo, kth, n=1 << 20, k=1 << 20)

        # overlap: an output (sized by m = min(k, numel) rows) on, inside, across the end of an input or another output
        one = np.zeros(160, np.uint32)
        O = "overlap"
        both(O, s0, a, None, a, None)                                                        # in place
        both(O, s0, one[0:16], None, one[15:31], None)                                       # one shared element with keys_in's end
        both(O, s0, one[8:24], None, one[1:32], None)                                        # keys_out's row m - 1 = 7 on keys_in's first
        both(O, s4, a, one[0:16], ko, one[8:24])                                             # values_out across the end of values_in
        both(O, s4, a, va, one[0:16], one[7:23])                                             # the two outputs share row m - 1
        both(O, s4, a, va, one[0:16], one[0:16])                                             # the two outputs on each other
        both(O, s4, a, None, one[0:16], one[4:20])                                           # the arg form: the same rule
        both(O, s0, a, None, one[0:16], None, one[7:8])                                      # kth_out on keys_out's last row
        both(O, s0, one[0:16], None, ko, None, one[15:16])                                   # kth_out on keys_in's last element
        both(O, s4, a, one[16:32], ko, vo, one[16:17])                                       # kth_out on values_in's first
        both(O, s4, a, va, ko, one[0:16], one[0:1])                                          # kth_out on values_out's first
        both(O, s0, one[20:36], None, one[10:30], None, n=16, k=100)                         # k above numel: m = 16 rows reach keys_in, 8 would not
        assert np.array_equal(ko, np.arange(100, 116)) and np.array_equal(vo, np.arange(200, 216))   # nothing was written
        assert np.array_equal(vo8, np.arange(300, 316)) and not one.any() and not a.any() and not va.any() and (kth == 777).all()

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS. Row m of an output is not part of it.
        for obj, args in ((s0, (one[0:16], None, one[16:24], None, one[24:25])),
                          (s4, (one[0:16], one[16:32], one[32:40], one[40:48], one[48:49])),
                          (s4, (one[0:16], None, None, one[16:24], None)),
                          (s0, (one[8:24], None, one[0:16], None, None)),            # keys_out's rows 8.. would overlap; m = 8 rows do not
                          (s0, (one[0:16], None, None, None, one[16:17]))):
            err = clo.api._Err()
            keys, vals, out_k, out_v, out_kth = args
            assert not lib.clo_topk_with_host_data(obj.h, None, None, p(keys), p(vals), p(out_k), p(out_v), p(out_kth), 16, 8, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.which, obj.order, e.value)
        assert not one.any()

        # (what only the device form can see — an output of m - 1 rows, an input below numel rows, kth_out below one key —
        # needs buffers, which an offline context does not make: tests/topk_host/topk_host_test.c refuses those over
        # the host stubs, and accepts an output of exactly m rows)
        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            s4.with_host_data(np.zeros(4, np.uint16), 3)
        with pytest.raises(ValueError):
            s4.with_host_data(np.zeros(4, np.uint32), 3, np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            s0.with_host_data(np.zeros(4, np.uint32), 3, np.zeros(4, np.uint32))
        for s in (s0, s4, s8, so):
            s.close()
    finally:
        ctx.close()


def test_numel_zero_and_k_zero_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        empty, some = np.zeros(0, np.float32), np.arange(5, dtype=np.float32)
        for which in WHICH:
            for order in ORDERS:
                for vs in (0, 4, 8):
                    s = clo.TopK(which, order, ctx, "float", vs)
                    for keys, k in ((empty, 3), (some, 0), (empty, 0)):
                        vals = np.zeros(keys.size, np.uint64) if vs == 8 else None    # (NULL values are the arg form: value_size 4 only)
                        ko, vo, kth = s.with_host_data(keys, k, vals)
                        assert ko.size == 0 and ko.dtype == np.float32 and (vo is None if vs == 0 else vo.size == 0) and kth is None
                        # raw: outputs that exist are not touched, the inputs of numel 0 may be NULL
                        out_k, out_v, out_kth = np.full(4, 7, np.uint32), np.full(4, 9, np.uint64), np.full(1, 5, np.uint32)
                        err = clo.api._Err()
                        assert lib.clo_topk_with_host_data(s.h, None, None, keys.ctypes.data if keys.size else None,
                                                           vals.ctypes.data if vals is not None and (keys.size or vs == 8) else None,
                                                           out_k.ctypes.data, out_v.ctypes.data if vs else None, out_kth.ctypes.data, keys.size, k, err.ref)
                        err.raise_if_set()
                        assert (out_k == 7).all() and (out_v == 9).all() and out_kth[0] == 5
                    s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "topk_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "topk_host", "topk_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("topk host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _pool(dt):
    """The specials of the type: +-0, +-1, +-inf, NaNs of both signs and two payloads; the integers' ends and zero's
    neighbours."""
    if dt.kind == "f":
        return np.concatenate((_specials(dt), np.array([-2.5, -1e-3, 3.0, 0.5, 7.0], dtype=dt)))
    info = np.iinfo(dt)
    return np.array([info.min, info.min + 1, info.max, info.max - 1, 0, 1, 5, 6] + ([-1, -2, -7] if dt.kind == "i" else [info.max // 2, info.max // 2 + 1]), dtype=dt)


def test_the_model_against_a_plain_loop():
    """For all eleven key types on their specials, both directions, both orders and every k from 0 to past numel (so
    that k cuts inside every tie run): the model's rows are the first m of Python's sort of (order key, index) tuples —
    the order of test_merge_cpu._py_order, from the definition, negated for "largest" — and the k-th key is the last of
    them."""
    rng = np.random.default_rng(17)
    for kt in KEY_TYPES:
        dt = np.dtype(clo.api.CLO_TYPE_NP[kt])
        pool = _pool(dt)
        keys = np.concatenate((pool, pool[rng.integers(0, pool.size, 30)]))
        order = _py_order(keys)
        raw = keys.view("u%d" % dt.itemsize)
        for which in WHICH:
            ranked = sorted(range(keys.size), key=lambda i: (order[i] if which == "smallest" else -order[i], i))
            for k in list(range(0, keys.size + 2)) + [10 * keys.size]:
                m = min(k, keys.size)
                what = (kt, which, k)
                p, kth = topk(which, "sorted", keys, k)
                assert p.dtype == np.uint32 and p.tolist() == ranked[:m], what
                assert kth.dtype == dt and kth.size == (1 if m else 0), what
                if m:
                    assert int(kth.view(raw.dtype)[0]) == int(raw[ranked[m - 1]]), what
                p2, kth2 = topk(which, "input", keys, k)
                assert p2.tolist() == sorted(ranked[:m]) and kth2.tobytes() == kth.tobytes(), what


def test_the_model_cuts_ties_by_index_and_keeps_bits_apart():
    """Among equal keys the lowest indices are taken, in both directions; -0 is not +0 (and lies below it), NaNs lie at
    the ends by sign."""
    keys = np.array([5, 3, 5, 3, 5, 3, 9], np.uint32)
    assert topk("smallest", "sorted", keys, 2)[0].tolist() == [1, 3] and topk("smallest", "input", keys, 4)[0].tolist() == [0, 1, 3, 5]
    assert topk("largest", "sorted", keys, 3)[0].tolist() == [6, 0, 2] and topk("largest", "input", keys, 3)[0].tolist() == [0, 2, 6]
    assert topk("largest", "sorted", keys, 3)[1][0] == 5 and topk("smallest", "sorted", keys, 3)[1][0] == 3
    for dt in (np.float16, np.float32, np.float64):
        z = np.array([0.0, -0.0, 0.0, -0.0], dtype=dt)
        assert topk("smallest", "sorted", z, 3)[0].tolist() == [1, 3, 0] and topk("largest", "sorted", z, 3)[0].tolist() == [0, 2, 1]
        assert np.signbit(topk("smallest", "sorted", z, 2)[1][0]) and not np.signbit(topk("smallest", "sorted", z, 3)[1][0])
        s = _specials(dt)                # -NaN a, -NaN b, -inf, -1, -0 | +0, +1, +inf, +NaN a, +NaN b  as indices 3 4 2 1 0 | 5 6 7 8 9
        assert sorted(topk("smallest", "input", s, 2)[0].tolist()) == [3, 4]       # the negative NaNs are the smallest
        assert sorted(topk("largest", "input", s, 2)[0].tolist()) == [8, 9]        # the positive NaNs the largest
        assert topk("largest", "sorted", s, 3)[0].tolist()[2] == 7                 # then +inf
