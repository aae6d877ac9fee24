"""CloSelect (include/clo_select.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs alone, numel == 0
succeeds without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among
them clo_hip_select_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/select_host/select_host_test.c. The reference model the GPU tests compare against (select_model.py) is checked
here against a plain Python loop over Python integers, for every key type on its special values and every pred."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from cl_ops_amd.select import SELECT_OPS, SELECT_PREDS, SELECT_SCAN_TRIP
from select_model import OPS, PREDS, keep_mask, select
from test_merge_cpu import KEY_TYPES, _py_order, _specials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_select_new", "clo_select_destroy", "clo_select_with_device_data", "clo_select_with_host_data",
          "clo_select_get_context", "clo_select_get_key_type", "clo_select_get_key_size", "clo_select_get_value_size",
          "clo_select_get_op", "clo_select_get_pred")
THIN = ("clo_hip_select", "clo_hip_select_workspace_bytes", "clo_hip_select_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_select.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SELECT_OPS "select, partition"' in text
    assert '#define CLO_SELECT_PREDS "flagged, lt, le, gt, ge, eq, ne"' in text
    assert ", ".join(SELECT_OPS) == "select, partition" == ", ".join(OPS)
    assert ", ".join(SELECT_PREDS) == "flagged, lt, le, gt, ge, eq, ne" == ", ".join(PREDS)
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(SELECT_OPS):                                       # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_SELECT_%s %d\n" % (n.upper().ljust(9), i) in text, n
    for i, n in enumerate(SELECT_PREDS):
        assert "#define CLO_HIP_SELECT_%s %d\n" % (n.upper().ljust(7), i) in text, n
    assert "#define CLO_HIP_SELECT_SCAN_TRIP %d\n" % SELECT_SCAN_TRIP in text
    assert '#include "clo_select.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Select", "select_tile"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_tile_and_workspace_getters():
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.select_tile(ks, vs)
            assert t >= 1024 and t % 1024 == 0, (ks, vs, t)                   # whole rows of 256 lanes x 4 elements
    for ks, vs in ((3, 0), (0, 0), (16, 4), (4, 2), (4, 1), (8, 16), (4, -4)):
        assert clo.select_tile(ks, vs) == 0, (ks, vs)
    ws = clo.api.lib.clo_hip_select_workspace_bytes
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            assert ws(0, ks, vs) == 0
            sizes = [ws(n, ks, vs) for n in (0, 1, 63, 5000, 8192, 8193, 1 << 20, 1 << 24, (1 << 32) - 1)]
            assert sizes == sorted(sizes) and sizes[1] > 0 and sizes[-1] < (8 << 20), (ks, vs, sizes)   # monotone, small next to the data
            assert all(s % 256 == 0 for s in sizes)
            t = clo.select_tile(ks, vs)
            for n in (1, t, t + 1, 100 * t + 5):                            # room for one count per tile and the total
                assert ws(n, ks, vs) >= 4 * (-(-n // t) + 1), (ks, vs, n)
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
        # at construction: ops, preds, value sizes, options, key types
        for op in ("", "filter", "Select", "selects", "partition ", None):
            assert "selection op" in _refused(lambda: clo.Select(op, "lt", ctx, "uint", 0))
            assert not lib.clo_select_new(op.encode() if op is not None else None, b"lt", None, ctx.h, 5, 0, None)   # err NULL
        for pred in ("", "less", "LT", "l", "flag", "==", None):
            assert "selection pred" in _refused(lambda: clo.Select("select", pred, ctx, "uint", 0))
            assert not lib.clo_select_new(b"select", pred.encode() if pred is not None else None, None, ctx.h, 5, 0, None)
        for vs in (1, 2, 3, 5, 12, 16):
            assert "value_size" in _refused(lambda: clo.Select("select", "lt", ctx, "uint", vs))
            assert not lib.clo_select_new(b"select", b"lt", None, ctx.h, 5, vs, None)
        for opt in ("descending", "tile=8192", " "):
            assert "options" in _refused(lambda: clo.Select("select", "lt", ctx, "uint", 0, options=opt))
            assert not lib.clo_select_new(b"select", b"lt", opt.encode(), ctx.h, 5, 0, None)
        assert not lib.clo_select_new(b"select", b"lt", None, ctx.h, 11, 0, None)
        for op in OPS:                                                       # every op, pred, key type, value size, both spellings of no options
            for pred in PREDS:
                for kt in KEY_TYPES:
                    for vs, opt in ((0, None), (4, ""), (8, None)):
                        s = clo.Select(op, pred, ctx, kt, vs, options=opt)
                        assert (s.op, s.pred, s.key_type, s.key_size, s.value_size) == \
                            (op, pred, clo.CLO_TYPES[kt], np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize, vs)
                        s.close()

        s0, s4, p8 = clo.Select("select", "lt", ctx, "uint", 0), clo.Select("select", "ge", ctx, "uint", 4), clo.Select("partition", "eq", ctx, "uint", 8)
        f0, f4 = clo.Select("select", "flagged", ctx, "uint", 0), clo.Select("partition", "flagged", ctx, "uint", 4)
        a, va = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        va8 = np.zeros(16, np.uint64)
        fl, t = np.zeros(16, np.uint8), np.array([5], np.uint32)
        ko, vo = np.arange(100, 116, dtype=np.uint32), np.arange(200, 216, dtype=np.uint32)
        vo8 = np.arange(300, 316, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(obj, keys, vals, fot, out_k, out_v, n=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_select_with_host_data(obj.h, None, None, p(keys), p(vals), p(fot), p(out_k), p(out_v), n,
                                               C.cast(p(out_n), C.POINTER(C.c_size_t)), err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), args
            host(*args, with_err=False, **kw)

        both("2^32", s0, a, None, t, ko, None, n=1 << 32)
        both("2^32", f4, a, va, fl, ko, vo, n=(1 << 32) + 5)
        both("2^32", p8, a, va8, t, ko, vo8, n=1 << 63)
        both("keys_in", s0, None, None, t, ko, None)                         # a comparison reads the keys
        both("keys_in", s4, None, None, t, None, vo)                         # ... in the arg form without keys_out too
        both("keys_in", f0, None, None, fl, ko, None)                        # flagged, but keys_out wants them
        both("keys_in", f4, None, None, fl, ko, vo)
        both("the threshold", s0, a, None, None, ko, None)                       # NULL flags_or_threshold
        both("the flags", f0, a, None, None, ko, None)
        both("the flags", f4, None, None, None, None, vo)
        both("num_out", s0, a, None, t, ko, None, out_n=None)                # num_out is required
        both("num_out", f4, a, va, fl, ko, vo, out_n=None)
        both("value_size 0", s0, a, va, t, ko, None)                         # values with value_size 0
        both("value_size 0", f0, a, None, fl, ko, vo)
        both("values_out", s4, a, va, t, ko, None)                           # values_out NULL with value_size > 0
        both("values_out", f4, a, None, fl, ko, None)
        both("value_size of 4", p8, a, None, t, ko, vo8)                     # NULL values with value_size 8
        both("both NULL", s0, a, None, t, None, None)                        # both outputs NULL
        both("both NULL", f4, a, va, fl, None, None)

        # overlap: an output (sized by numel rows, not by k: all keys are 0 and the threshold 5, so "lt" keeps all and
        # "ge" / "eq" none) on, inside, across the end of an input, the flags, the threshold or another output
        one = np.zeros(160, np.uint32)
        one8 = one.view(np.uint8)
        O = "overlap"
        both(O, s0, a, None, t, a, None)                                                     # in place
        both(O, s0, one[0:16], None, t, one[15:31], None)                                    # one shared element with keys_in's end
        both(O, s0, one[8:24], None, t, one[0:32], None, n=16)                               # keys_in inside a larger keys_out allocation
        both(O, s4, one[31:47], va, t, one[16:32], vo)                                        # "ge" keeps nothing: row numel - 1 still counts
        both(O, s4, a, va, one[31:32], one[16:32], vo)                                       # keys_out's last row on the threshold
        both(O, p8, a, va8, one[16:17], ko, one[0:32].view(np.uint64))                       # values_out's 16 x 8 bytes across the threshold
        both(O, f0, a, None, one8[64:80], one[19:35], None)                                  # keys_out's first row on the flags' last bytes
        both(O, f4, a, va, one8[64:80], ko, one[0:17][1:])                                   # values_out's last row on the flags' first bytes
        both(O, s4, a, one[0:16], t, ko, one[8:24])                                          # values_out across the end of values_in
        both(O, s4, a, va, t, one[0:16], one[15:31])                                         # the two outputs share one row
        both(O, s4, a, va, t, one[0:16], one[0:16])                                          # the two outputs on each other
        both(O, s4, a, None, t, one[0:16], one[8:24])                                        # the arg form: the same rule
        both(O, s0, a, None, t, one[0:16], None, out_n=one[14:16].view(np.uint64))           # num_out on keys_out's last rows
        both(O, s0, one[0:16], None, t, ko, None, out_n=one[14:16].view(np.uint64))          # num_out on keys_in's
        both(O, s0, a, None, one[20:21], ko, None, out_n=one[20:22].view(np.uint64))         # num_out on the threshold
        both(O, f4, a, va, one8[80:96], ko, vo, out_n=one[22:24].view(np.uint64))            # num_out on the flags
        both(O, s4, a, va, t, ko, one[0:16], out_n=one[0:2].view(np.uint64))                 # num_out on values_out's first
        assert np.array_equal(ko, np.arange(100, 116)) and np.array_equal(vo, np.arange(200, 216))   # nothing was written
        assert np.array_equal(vo8, np.arange(300, 316)) and not one.any() and not a.any() and not va.any() and (num == 777).all()
        assert t[0] == 5 and not fl.any()

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS
        n8 = one[150:152].view(np.uint64)
        for obj, args in ((s0, (one[0:16], None, one[16:17], one[17:33], None)),
                          (s4, (one[0:16], one[16:32], one[32:33], one[33:49], one[49:65])),
                          (s4, (one[0:16], None, one[16:17], None, one[17:33])),
                          (f0, (one[0:16], None, one8[64:80], one[20:36], None)),
                          (f4, (None, None, one8[64:80], None, one[20:36]))):
            err = clo.api._Err()
            keys, vals, fot, out_k, out_v = args
            assert not lib.clo_select_with_host_data(obj.h, None, None, p(keys), p(vals), p(fot), p(out_k), p(out_v), 16,
                                                     C.cast(p(n8), C.POINTER(C.c_size_t)), err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.op, obj.pred, e.value)
        assert not one[:150].any()

        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            s4.with_host_data(np.zeros(4, np.uint16), 3)
        with pytest.raises(ValueError):
            s4.with_host_data(np.zeros(4, np.uint32), 3, np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            s0.with_host_data(np.zeros(4, np.uint32), 3, np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            f4.with_host_data(np.zeros(4, np.uint32), np.zeros(3, np.uint8))
        with pytest.raises(ValueError):
            s0.with_host_data(None, 3)
        for s in (s0, s4, p8, f0, f4):
            s.close()
    finally:
        ctx.close()


def test_numel_zero_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        empty = np.zeros(0, np.float32)
        for op in OPS:
            for pred in ("flagged", "lt", "ne"):
                for vs in (0, 4, 8):
                    s = clo.Select(op, pred, ctx, "float", vs)
                    fot = np.zeros(0, np.uint8) if pred == "flagged" else np.float32(1.5)
                    vals = np.zeros(0, np.uint64) if vs == 8 else None      # (NULL values are the arg form: value_size 4 only)
                    ko, vo, k = s.with_host_data(empty, fot, vals)
                    assert k == 0 and ko.size == 0 and ko.dtype == np.float32 and (vo is None if vs == 0 else vo.size == 0)
                    # raw: num_out becomes 0, outputs that exist are not touched, inputs may be NULL (the flags too)
                    out_k, out_v, num = np.full(4, 7, np.uint32), np.full(4, 9, np.uint64), C.c_size_t(55)
                    thr = np.array([1.5], np.float32)
                    err = clo.api._Err()
                    assert lib.clo_select_with_host_data(s.h, None, None, None, thr.ctypes.data if vs == 8 else None,
                                                         None if pred == "flagged" else thr.ctypes.data,
                                                         out_k.ctypes.data, out_v.ctypes.data if vs else None, 0, C.byref(num), err.ref)
                    err.raise_if_set()
                    assert num.value == 0 and (out_k == 7).all() and (out_v == 9).all()
                    s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "select_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "select_host", "select_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("select host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _pool(dt):
    """The specials of the type: +-0, +-1, +-inf, NaNs of both signs and two payloads; the integers' ends and zero's
    neighbours."""
    if dt.kind == "f":
        return np.concatenate((_specials(dt), np.array([-2.5, -1e-3, 3.0, 0.5, 7.0], dtype=dt)))
    info = np.iinfo(dt)
    return np.array([info.min, info.min + 1, info.max, info.max - 1, 0, 1, 5, 6] + ([-1, -2, -7] if dt.kind == "i" else [info.max // 2, info.max // 2 + 1]), dtype=dt)


_PY = {"lt": lambda x, t: x < t, "le": lambda x, t: x <= t, "gt": lambda x, t: x > t, "ge": lambda x, t: x >= t,
       "eq": lambda x, t: x == t, "ne": lambda x, t: x != t}


def test_the_model_against_a_plain_loop():
    """For all eleven key types on their specials, every pred, every threshold of the pool: the model's rows are what a
    loop over Python integers (the order of test_merge_cpu._py_order, from the definition) keeps, in its order."""
    rng = np.random.default_rng(16)
    for kt in KEY_TYPES:
        dt = np.dtype(clo.api.CLO_TYPE_NP[kt])
        pool = _pool(dt)
        keys = np.concatenate((pool, pool[rng.integers(0, pool.size, 40)]))
        order = _py_order(keys)
        flags = rng.integers(0, 4, keys.size).astype(np.uint8) * np.uint8(85)      # 0, 85, 170, 255
        for pred in PREDS:
            for ti in range(pool.size if pred != "flagged" else 1):
                thr = pool[ti]
                if pred == "flagged":
                    kept = [i for i in range(keys.size) if flags[i] != 0]
                else:
                    t = _py_order(pool[ti:ti + 1])[0]
                    kept = [i for i in range(keys.size) if _PY[pred](order[i], t)]
                rest = [i for i in range(keys.size) if i not in set(kept)]
                fot = flags if pred == "flagged" else thr
                what = (kt, pred, ti)
                assert keep_mask(pred, keys, fot).tolist() == [i in set(kept) for i in range(keys.size)], what
                p, k = select("select", pred, keys, fot)
                assert p.dtype == np.uint32 and k == len(kept) and p.tolist() == kept, what
                p, k = select("partition", pred, keys, fot)
                assert k == len(kept) and p.tolist() == kept + rest, what


def test_the_model_keeps_bits_apart():
    """The order is total: "eq" is equality of bits. -0 is not +0 (and lies below it), NaNs compare by payload, and
    negative NaNs lie below -inf."""
    for dt in (np.float16, np.float32, np.float64):
        z = np.array([-0.0, 0.0], dtype=dt)
        assert select("select", "eq", z, z[0])[0].tolist() == [0] and select("select", "eq", z, z[1])[0].tolist() == [1]
        assert select("select", "lt", z, z[1])[0].tolist() == [0] and select("select", "ge", z, z[1])[0].tolist() == [1]
        s = _specials(dt)                # -NaN a, -NaN b, -inf, -1, -0 | +0, +1, +inf, +NaN a, +NaN b  as indices 3 4 2 1 0 | 5 6 7 8 9
        assert select("select", "eq", s, s[3])[0].tolist() == [3] and select("select", "ne", s, s[8])[1] == 9
        assert sorted(select("select", "lt", s, s[2])[0].tolist()) == [3, 4]       # only the negative NaNs are below -inf
        assert sorted(select("select", "gt", s, s[7])[0].tolist()) == [8, 9]       # only the positive NaNs are above +inf
        assert select("partition", "le", s, s[0])[0].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]   # the negative half, then the rest
