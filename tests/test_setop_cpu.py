"""CloSetOp (include/clo_setop.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile, workspace and capacity getters answer, every refusal comes back as CLO_ERROR_ARGS
through an offline context before anything touches a device (err == NULL included) and leaves the outputs alone, two
empty inputs succeed without a device, and the C driver runs over the host stubs of the thin C-ABI
(tests/hoststub/*stub*.c, among them clo_hip_setop_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone
program tests/setop_host/setop_host_test.c. The reference model the GPU tests compare against (setop_model.py) is
checked here against std::set_* restated as a two-pointer loop over Python integers, against collections.Counter's
multiset arithmetic, and on duplicate-free inputs against numpy's set routines."""
import collections
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from merge_model import merge, order_key, sort_keys
from setop_model import OPS, capacity, setop
from test_merge_cpu import KEY_TYPES, _py_order, _specials

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_setop_new", "clo_setop_destroy", "clo_setop_with_device_data", "clo_setop_with_host_data",
          "clo_setop_get_context", "clo_setop_get_key_type", "clo_setop_get_key_size", "clo_setop_get_value_size",
          "clo_setop_get_op", "clo_setop_get_max_numel_out")
THIN = ("clo_hip_setop", "clo_hip_setop_workspace_bytes", "clo_hip_setop_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_setop.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SETOP_OPS "union, intersection, difference, symmetric_difference"' in text
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_setop.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("SetOp", "setop_tile"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_tile_workspace_and_capacity_getters():
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.setop_tile(ks, vs)
            assert t >= 64 and t % 64 == 0, (ks, vs, t)
    for ks, vs in ((3, 0), (0, 0), (16, 4), (4, 2), (4, 1), (8, 16), (4, -4)):
        assert clo.setop_tile(ks, vs) == 0, (ks, vs)
    ws = clo.api.lib.clo_hip_setop_workspace_bytes
    assert ws(0, 0) == 0
    sizes = [ws(n, n // 3) for n in (0, 1, 63, 5000, 1 << 20, 1 << 24, 3 << 29)]
    assert sizes == sorted(sizes) and sizes[-1] < (64 << 20)                 # monotone, and small next to the data
    assert ws(1000, 24) == ws(24, 1000) == ws(1024, 0)                       # a function of n
    ctx = clo.Context(offline=True)
    try:
        for op in OPS:
            s = clo.SetOp(op, ctx, "uint", 4)
            assert s.op == op
            for na, nb in ((0, 0), (0, 9), (9, 0), (5, 9), (9, 5), (1 << 31, 1 << 30)):
                assert s.max_numel_out(na, nb) == capacity(op, na, nb), (op, na, nb)
            s.close()
    finally:
        ctx.close()


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        # at construction: ops, value sizes, options, key types
        for op in ("", "xor", "Union", "unions", "symmetric difference", None):
            assert "set operation" in _refused(lambda: clo.SetOp(op, ctx, "uint", 0))
            assert not lib.clo_setop_new(op.encode() if op is not None else None, None, ctx.h, 5, 0, None)   # err NULL
        for vs in (1, 2, 3, 5, 12, 16):
            assert "value_size" in _refused(lambda: clo.SetOp("union", ctx, "uint", vs))
            assert not lib.clo_setop_new(b"union", None, ctx.h, 5, vs, None)
        for opt in ("descending", "tile=2304", " "):
            assert "options" in _refused(lambda: clo.SetOp("union", ctx, "uint", 0, options=opt))
            assert not lib.clo_setop_new(b"union", opt.encode(), ctx.h, 5, 0, None)
        assert not lib.clo_setop_new(b"union", None, ctx.h, 11, 0, None)
        for op in OPS:                                                           # every op, key type, value size, both spellings of no options
            for kt in KEY_TYPES:
                for vs in (0, 4, 8):
                    for opt in (None, ""):
                        s = clo.SetOp(op, ctx, kt, vs, options=opt)
                        assert (s.op, s.key_type, s.key_size, s.value_size) == (op, clo.CLO_TYPES[kt], np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize, vs)
                        s.close()

        u0, u4, x8 = clo.SetOp("union", ctx, "uint", 0), clo.SetOp("union", ctx, "uint", 4), clo.SetOp("symmetric_difference", ctx, "uint", 8)
        i0, i4, d4 = clo.SetOp("intersection", ctx, "uint", 0), clo.SetOp("intersection", ctx, "uint", 4), clo.SetOp("difference", ctx, "uint", 4)
        a, b, va, vb = (np.zeros(16, np.uint32) for _ in range(4))
        va8, vb8 = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
        ko, vo = np.arange(100, 132, dtype=np.uint32), np.arange(200, 232, dtype=np.uint32)
        vo8 = np.arange(300, 332, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(obj, ka, xa, na, kb, xb, nb, out_k, out_v, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_setop_with_host_data(obj.h, None, None, p(ka), p(xa), na, p(kb), p(xb), nb, p(out_k), p(out_v),
                                              C.cast(p(out_n), C.POINTER(C.c_size_t)), err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), args
            host(*args, with_err=False, **kw)

        both("2^32", u4, a, va, (1 << 32) - 16, b, vb, 16, ko, vo)
        both("2^32", u0, a, None, 1 << 32, b, None, 0, ko, None)
        both("2^32", i0, a, None, 1 << 63, b, None, 1 << 63, ko, None)       # the sum wraps to 0
        both("keys_a", u0, None, None, 16, b, None, 16, ko, None)
        both("keys_b", i0, a, None, 16, None, None, 16, ko, None)
        both("num_out", u0, a, None, 16, b, None, 16, ko, None, out_n=None)  # num_out is required
        both("num_out", i4, a, va, 16, b, vb, 16, ko, vo, out_n=None)
        both("both be given", u4, a, va, 16, b, None, 16, ko, vo)            # exactly one values array NULL where both are looked at
        both("both be given", u4, a, None, 16, b, vb, 16, ko, vo)
        both("value_size 0", u0, a, va, 16, b, vb, 16, ko, None)             # values with value_size 0
        both("value_size 0", i0, a, None, 16, b, None, 16, ko, vo)
        both("values_out", u4, a, va, 16, b, vb, 16, ko, None)               # values_out NULL with value_size > 0
        both("values_out", d4, a, None, 16, b, None, 16, ko, None)
        both("value_size of 4", x8, a, None, 16, b, None, 16, ko, vo8)       # NULL values with value_size 8
        both("value_size of 4", x8, a, None, 16, b, None, 0, ko, vo8)
        both("both NULL", u0, a, None, 16, b, None, 16, None, None)          # both outputs NULL
        both("both NULL", i4, a, va, 16, b, vb, 16, None, None)

        # overlap: an output (sized by the capacity) on, inside, across the end of an input or of another output
        one = np.zeros(160, np.uint32)
        O = "overlap"
        both(O, u0, a, None, 16, b, None, 16, a, None)                                       # on keys_a (and too small: never looked at)
        both(O, u0, one[0:16], None, 16, one[40:56], None, 16, one[40:72], None)             # starts on keys_b
        both(O, u0, one[8:24], None, 16, b, None, 16, one[0:32], None)                       # keys_a inside keys_out
        both(O, u0, one[0:16], None, 16, b, None, 16, one[15:47], None)                      # one shared element with keys_a's end
        both(O, u0, a, None, 16, one[32:48], None, 16, one[1:33], None)                      # one shared element with keys_b's start
        both(O, i0, one[0:16], None, 16, b, None, 16, one[15:31], None)                      # an intersection's 16 rows reach keys_a's end too
        both(O, u4, a, one[0:16], 16, b, vb, 16, ko, one[8:40])                              # values_out across the end of values_a
        both(O, u4, a, va, 16, b, one[40:56], 16, one[30:62], vo)                            # keys_out over values_b
        both(O, u4, a, va, 16, b, vb, 16, one[0:32], one[31:63])                             # the two outputs share one element
        both(O, u4, a, va, 16, b, vb, 16, one[0:32], one[0:32])                              # the two outputs on each other
        both(O, u4, a, None, 16, b, None, 16, one[0:32], one[16:48])                         # the arg form: the same rule
        both(O, x8, a, va8, 16, b, vb8, 16, vo8[0:32].view(np.uint32)[0:32], vo8)            # keys_out inside values_out
        both(O, u0, a, None, 16, b, None, 16, one[0:32], None, out_n=one[30:32].view(np.uint64))   # num_out on keys_out's last elements
        both(O, u0, one[0:16], None, 16, b, None, 16, ko, None, out_n=one[14:16].view(np.uint64))  # num_out on keys_a's
        both(O, u4, a, va, 16, b, vb, 16, ko, one[0:32], out_n=one[0:2].view(np.uint64))           # num_out on values_out's first
        assert np.array_equal(ko, np.arange(100, 132)) and np.array_equal(vo, np.arange(200, 232))   # nothing was written
        assert np.array_equal(vo8, np.arange(300, 332)) and not one.any() and not a.any() and not va.any() and (num == 777).all()

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS. An intersection's outputs end after min(numel_a, numel_b) rows,
        # a difference's after numel_a, and neither looks at values_b: NULL, or on an output.
        n8 = one[150:152].view(np.uint64)
        for obj, args in ((u0, (one[0:16], None, 16, one[16:32], None, 16, one[32:64], None)),
                          (u4, (one[0:16], one[64:80], 16, one[16:32], one[80:96], 16, one[32:64], one[96:128])),
                          (u4, (one[0:16], None, 16, one[16:32], None, 16, None, one[32:64])),
                          (i0, (one[0:16], None, 16, one[16:24], None, 8, one[24:32], None)),             # capacity 8: ends where the next view begins
                          (i4, (one[0:16], one[64:80], 16, one[16:32], None, 16, one[32:48], one[48:64])),
                          (d4, (one[0:16], one[64:80], 16, one[16:48], one[96:128], 32, one[48:64], one[96:112]))):
            err = clo.api._Err()
            ka, xa, na, kb, xb, nb, out_k, out_v = args
            assert not lib.clo_setop_with_host_data(obj.h, None, None, p(ka), p(xa), na, p(kb), p(xb), nb, p(out_k), p(out_v),
                                                    C.cast(p(n8), C.POINTER(C.c_size_t)), err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.op, e.value)
        assert not one[:150].any()

        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            u4.with_host_data(np.zeros(4, np.uint16), np.zeros(4, np.uint16))
        with pytest.raises(ValueError):
            u4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint64), np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            u0.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            u4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(3, np.uint32), np.zeros(4, np.uint32))
        for s in (u0, u4, x8, i0, i4, d4):
            s.close()
    finally:
        ctx.close()


def test_both_inputs_empty_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        empty = np.zeros(0, np.float32)
        for op in OPS:
            for vs in (0, 4, 8):
                s = clo.SetOp(op, ctx, "float", vs)
                ko, vo = s.with_host_data(empty, empty)
                assert ko.size == 0 and ko.dtype == np.float32 and (vo is None if vs == 0 else vo.size == 0)
                # raw: num_out becomes 0, outputs that exist are not touched, inputs may be NULL
                out_k, out_v, k = np.full(4, 7, np.uint32), np.full(4, 9, np.uint64), C.c_size_t(55)
                err = clo.api._Err()
                assert lib.clo_setop_with_host_data(s.h, None, None, None, None, 0, None, None, 0, out_k.ctypes.data,
                                                    out_v.ctypes.data if vs else None, C.byref(k), err.ref)
                err.raise_if_set()
                assert k.value == 0 and (out_k == 7).all() and (out_v == 9).all()
                s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "setop_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "setop_host", "setop_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("setop host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(op, keys_a, keys_b):
    """std::set_union / set_intersection / set_difference / set_symmetric_difference, restated: two pointers over
    Python integers. Returns the indices into A || B of what the algorithm copies, in its order."""
    oa, ob = _py_order(keys_a), _py_order(keys_b)
    na, nb = len(oa), len(ob)
    i = j = 0
    p = []
    while i < na and j < nb:
        if oa[i] < ob[j]:
            if op != "intersection":
                p.append(i)
            i += 1
        elif ob[j] < oa[i]:
            if op in ("union", "symmetric_difference"):
                p.append(na + j)
            j += 1
        else:
            if op in ("union", "intersection"):
                p.append(i)
            i += 1
            j += 1
    if op != "intersection":
        p.extend(range(i, na))
    if op in ("union", "symmetric_difference"):
        p.extend(range(na + j, na + nb))
    return np.array(p, dtype=np.uint32)


def _pool(dt, rng):
    if dt.kind == "f":
        return np.concatenate((_specials(dt), np.array([-2.5, -1e-3, 3.0, 0.5, 7.0], dtype=dt)))
    info = np.iinfo(dt)
    return np.array([info.min, info.max, 0, 1, 5, 6] + ([-1, -2, -7] if dt.kind == "i" else [info.max - 3]), dtype=dt)


SIZES = ((0, 0), (0, 9), (9, 0), (1, 1), (50, 70), (300, 11))


def _inputs():
    rng = np.random.default_rng(12)
    for kt in KEY_TYPES:
        dt = np.dtype(clo.api.CLO_TYPE_NP[kt])
        pool = _pool(dt, rng)
        for na, nb in SIZES:
            a = sort_keys(pool[rng.integers(0, pool.size, na)])          # few distinct keys: runs in A and in B
            b = sort_keys(pool[rng.integers(0, pool.size, nb)])
            yield kt, dt, a, b


def test_the_model_against_a_two_pointer_loop():
    """std::set_* take an element of A wherever they may take either, and so does the table: the indices agree, not
    only the keys. (For the symmetric difference and the union the loop copies the SURPLUS of a run, the table keeps
    the elements of rank >= the other count: the same elements, because the loop pairs off equal keys from the front.)"""
    for kt, dt, a, b in _inputs():
        for op in OPS:
            keys_out, p = setop(op, a, b)
            what = (kt, op, a.size, b.size)
            assert keys_out.dtype == dt and p.dtype == np.uint32
            assert p.size <= capacity(op, a.size, b.size), what
            assert np.array_equal(p, _loop(op, a, b)), what
            cat = np.concatenate((a, b))
            assert np.array_equal(keys_out.view(np.uint8), cat[p].view(np.uint8)), what
            # a subsequence of the merge: ascending, and among equal keys the indices ascend (A before B, input order)
            ok = order_key(cat)[p]
            assert (ok[1:] >= ok[:-1]).all() and (p[1:][ok[1:] == ok[:-1]] > p[:-1][ok[1:] == ok[:-1]]).all(), what
            merged_p = merge(a, b)[1]
            assert np.array_equal(merged_p[np.isin(merged_p, p)], p), what


def test_the_model_against_counter_arithmetic():
    for kt, dt, a, b in _inputs():
        ca, cb = collections.Counter(_py_order(a)), collections.Counter(_py_order(b))
        want = {"union": ca | cb, "intersection": ca & cb, "difference": ca - cb, "symmetric_difference": (ca - cb) + (cb - ca)}
        for op in OPS:
            keys_out, p = setop(op, a, b)
            assert collections.Counter(_py_order(keys_out)) == want[op], (kt, op, a.size, b.size)
            assert sum(want[op].values()) == p.size
            if op in ("intersection", "difference"):
                assert (p < a.size).all()                                 # indices into A


def test_the_model_on_duplicate_free_inputs():
    """Without duplicates the multiset operations are the set operations: numpy's, on the order keys (np.union1d and
    friends sort by value, which for floats is not the total order and merges -0 with +0)."""
    for kt, dt, a, b in _inputs():
        ua, ub = a[np.unique(order_key(a), return_index=True)[1]], b[np.unique(order_key(b), return_index=True)[1]]
        oa, ob = order_key(ua), order_key(ub)
        want = {"union": np.union1d(oa, ob), "intersection": np.intersect1d(oa, ob, assume_unique=True),
                "difference": np.setdiff1d(oa, ob, assume_unique=True), "symmetric_difference": np.setxor1d(oa, ob, assume_unique=True)}
        for op in OPS:
            keys_out, p = setop(op, ua, ub)
            assert np.array_equal(order_key(keys_out), want[op]), (kt, op, ua.size, ub.size)


def test_the_model_keeps_bits_apart():
    """Equal iff the bits are equal: -0 and +0 are different keys, NaNs are equal by payload."""
    for dt in (np.float16, np.float32, np.float64):
        z = np.array([-0.0, 0.0], dtype=dt)
        assert setop("intersection", z[:1], z[1:])[1].size == 0
        assert setop("union", z[1:], z[:1])[1].tolist() == [1, 0]         # B's -0 sorts below A's +0
        assert setop("difference", z, z[1:])[1].tolist() == [0]
        s = _specials(dt)
        nans = sort_keys(s[[3, 4, 8, 9]])                                 # two negative and two positive payloads
        assert setop("intersection", nans, nans[1:3])[1].tolist() == [1, 2]
        assert setop("symmetric_difference", nans[:2], nans[1:])[1].tolist() == [0, 3, 4]
