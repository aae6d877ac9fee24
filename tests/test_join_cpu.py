"""CloJoin (include/clo_join.h) on the CPU: the library exports the new public and thin-ABI entry points and the headers
declare them, the tile, workspace and upper-bound getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs alone, two empty inputs
succeed without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among
them clo_hip_join_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/join_host/join_host_test.c. The reference model the GPU tests compare against (join_model.py) is checked here
against a plain two-pointer loop over Python integers and, for inner joins of duplicate-free inputs, against
np.intersect1d(..., return_indices=True)."""
import ctypes as C
import glob
import itertools
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from join_model import KINDS, NONE, join, max_rows
from merge_model import order_key, sort_keys
from test_merge_cpu import KEY_TYPES, _py_order, _specials
from test_setop_cpu import SIZES, _pool

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_join_new", "clo_join_destroy", "clo_join_with_device_data", "clo_join_with_host_data",
          "clo_join_get_context", "clo_join_get_key_type", "clo_join_get_key_size", "clo_join_get_kind",
          "clo_join_get_max_numel_out")
THIN = ("clo_hip_join", "clo_hip_join_workspace_bytes", "clo_hip_join_tile", "clo_hip_join_out_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_join.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_JOIN_KINDS "inner, left, right, full"' in text and "#define CLO_JOIN_NONE 0xFFFFFFFFu" in text
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_join.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Join", "join_tile", "JOIN_KINDS", "JOIN_NONE"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert clo.JOIN_KINDS == KINDS and clo.JOIN_NONE == NONE == 0xFFFFFFFF


def test_tile_workspace_and_upper_bound_getters():
    for ks in (1, 2, 4, 8):
        t = clo.join_tile(ks)
        assert t >= 64 and t % 64 == 0, (ks, t)
    for ks in (3, 0, 16, -4):
        assert clo.join_tile(ks) == 0, ks
    assert clo.join_out_tile() >= 64 and clo.join_out_tile() % 64 == 0
    ws = clo.api.lib.clo_hip_join_workspace_bytes
    for kind in range(4):
        assert ws(kind, 0, 0) == 0
        sizes = [ws(kind, n, n // 3) for n in (0, 1, 63, 5000, 1 << 20, 1 << 24, 3 << 29)]
        assert sizes == sorted(sizes) and all(s % 256 == 0 for s in sizes) and sizes[1] > 0    # monotone
        assert sizes[-1] < 17 * ((3 << 29) + (1 << 29)) + (8 << 20)                           # 16 bytes per input element, and little else
        for na, nb in ((7, 0), (0, 7), (100, 100), (5000, 1)):                              # monotone in either argument alone
            assert ws(kind, na, nb) <= ws(kind, na + 1, nb) and ws(kind, na, nb) <= ws(kind, na, nb + 1)
    assert ws(-1, 100, 100) == 0 and ws(4, 100, 100) == 0
    ctx = clo.Context(offline=True)
    try:
        for kind in KINDS:
            j = clo.Join(kind, ctx, "uint")
            assert j.kind == kind
            for na, nb in ((0, 0), (0, 9), (9, 0), (5, 9), (9, 5), (1, 1), (2, 1), (1 << 31, 1 << 30)):
                assert j.max_numel_out(na, nb) == max_rows(kind, na, nb), (kind, na, nb)
            assert j.max_numel_out(1 << 40, 1 << 40) == (1 << 64) - 1                        # saturates
            j.close()
    finally:
        ctx.close()


def test_the_upper_bound_is_reached_and_never_exceeded():
    """max_rows by brute force: every pair of sorted arrays over three keys with at most three rows a side."""
    arrays = [np.array(c, np.uint8) for n in range(4) for c in itertools.combinations_with_replacement(range(3), n)]
    for kind in KINDS:
        best = {}
        for a in arrays:
            for b in arrays:
                K = join(kind, a, b, capacity=0)[3]
                best[(a.size, b.size)] = max(best.get((a.size, b.size), 0), K)
        for (na, nb), K in best.items():
            assert K == max_rows(kind, na, nb), (kind, na, nb, K)


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for kind in ("", "outer", "Inner", "inners", "full outer", None):
            assert "join kind" in _refused(lambda: clo.Join(kind, ctx, "uint"))
            assert not lib.clo_join_new(kind.encode() if kind is not None else None, None, ctx.h, 5, None)   # err NULL
        for opt in ("descending", "tile=2304", " "):
            assert "options" in _refused(lambda: clo.Join("inner", ctx, "uint", options=opt))
            assert not lib.clo_join_new(b"inner", opt.encode(), ctx.h, 5, None)
        assert not lib.clo_join_new(b"inner", None, ctx.h, 11, None)
        for kind in KINDS:                                                       # every kind, key type, both spellings of no options
            for kt in KEY_TYPES:
                for opt in (None, ""):
                    j = clo.Join(kind, ctx, kt, options=opt)
                    assert (j.kind, j.key_type, j.key_size) == (kind, clo.CLO_TYPES[kt], np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize)
                    j.close()

        jn, jf, j8 = clo.Join("inner", ctx, "uint"), clo.Join("full", ctx, "uint"), clo.Join("left", ctx, "double")
        a, b = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        ia, ib, ko = np.arange(100, 132, dtype=np.uint32), np.arange(200, 232, dtype=np.uint32), np.arange(300, 332, dtype=np.uint32)
        num = np.full(2, 777, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(obj, ka, na, kb, nb, out_a, out_b, out_k, cap=32, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_join_with_host_data(obj.h, None, None, p(ka), na, p(kb), nb, p(out_a), p(out_b), p(out_k), cap,
                                             C.cast(p(out_n), C.POINTER(C.c_size_t)), err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), args
            host(*args, with_err=False, **kw)

        both("2^32", jn, a, (1 << 32) - 16, b, 16, ia, ib, ko)
        both("2^32", jf, a, 1 << 32, b, 0, ia, ib, ko)
        both("2^32", jn, a, 1 << 63, b, 1 << 63, ia, ib, ko)                 # the sum wraps to 0
        both("capacity", jn, a, 16, b, 16, ia, ib, ko, cap=1 << 32)
        both("capacity", jf, a, 16, b, 16, ia, None, None, cap=1 << 40)
        both("keys_a", jn, None, 16, b, 16, ia, ib, ko)
        both("keys_b", jf, a, 16, None, 16, ia, ib, ko)
        both("num_out", jn, a, 16, b, 16, ia, ib, ko, out_n=None)            # num_out is required
        both("num_out", jf, a, 16, b, 16, None, None, None, cap=0, out_n=None)   # ... in the count form too
        both("all NULL", jn, a, 16, b, 16, None, None, None)                 # a capacity and nothing to hold it
        both("all NULL", jf, a, 16, b, 0, None, None, None, cap=1)

        # overlap: an output (sized by the capacity) on, inside, across the end of an input or of another output
        one = np.zeros(200, np.uint32)
        O = "overlap"
        both(O, jn, a, 16, b, 16, a, ib, ko, cap=16)                                             # idx_a_out on keys_a
        both(O, jn, one[0:16], 16, one[40:56], 16, one[40:72], ib, ko)                           # starts on keys_b
        both(O, jn, one[8:24], 16, b, 16, ia, one[0:32], ko)                                     # keys_a inside idx_b_out
        both(O, jn, one[0:16], 16, b, 16, ia, ib, one[15:47])                                    # one shared element with keys_a's end
        both(O, jn, a, 16, one[32:48], 16, one[1:33], None, None)                                # one shared element with keys_b's start
        both(O, jn, a, 16, b, 16, one[0:32], one[31:63], ko)                                     # the index outputs share one element
        both(O, jn, a, 16, b, 16, one[0:32], one[0:32], None)                                    # ... or lie on each other
        both(O, jn, a, 16, b, 16, None, one[0:32], one[16:48])                                   # keys_out inside idx_b_out
        both(O, j8, one[0:32].view(np.float64), 16, one[32:64].view(np.float64), 16, ia, ib, one[62:126].view(np.float64))   # 8-byte keys: keys_out is twice as long
        both(O, jn, a, 16, b, 16, one[0:32], ib, ko, out_n=one[30:32].view(np.uint64))           # num_out on idx_a_out's last elements
        both(O, jn, one[0:16], 16, b, 16, ia, ib, ko, out_n=one[14:16].view(np.uint64))          # num_out on keys_a's
        both(O, jn, a, 16, b, 16, None, None, one[0:32], out_n=one[0:2].view(np.uint64))         # num_out on keys_out's first
        assert np.array_equal(ia, np.arange(100, 132)) and np.array_equal(ib, np.arange(200, 232)) and np.array_equal(ko, np.arange(300, 332))
        assert not one.any() and not a.any() and (num == 777).all()                             # nothing was written

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS. An output ends after `capacity` rows; with capacity 0 it has no
        # bytes at all.
        n8 = one[190:192].view(np.uint64)
        for obj, args, cap in ((jn, (one[0:16], 16, one[16:32], 16, one[32:64], one[64:96], one[96:128]), 32),
                               (jf, (one[0:16], 16, one[16:32], 16, one[32:40], None, one[40:48]), 8),
                               (jn, (one[0:16], 16, one[16:32], 16, None, None, None), 0),
                               (jf, (one[0:16], 16, one[16:32], 16, one[0:16], one[0:16], None), 0),
                               (jn, (one[0:16], 16, None, 0, one[32:64], None, None), 32)):
            err = clo.api._Err()
            ka, na, kb, nb, out_a, out_b, out_k = args
            assert not lib.clo_join_with_host_data(obj.h, None, None, p(ka), na, p(kb), nb, p(out_a), p(out_b), p(out_k), cap,
                                                   C.cast(p(n8), C.POINTER(C.c_size_t)), err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.kind, e.value)
        assert not one[:190].any()

        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            jn.with_host_data(np.zeros(4, np.uint16), np.zeros(4, np.uint16), capacity=4)
        with pytest.raises(ValueError):
            jn.count(np.zeros(4, np.uint32), np.zeros(4, np.int32))
        for j in (jn, jf, j8):
            j.close()
    finally:
        ctx.close()


def test_both_inputs_empty_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        empty = np.zeros(0, np.float32)
        for kind in KINDS:
            j = clo.Join(kind, ctx, "float")
            assert j.count(empty, empty) == 0
            ia, ib, ko, K = j.with_host_data(empty, empty, keys_out=True)
            assert K == 0 and ia.size == 0 and ib.size == 0 and ko.size == 0 and ko.dtype == np.float32
            # raw: num_out becomes 0, outputs that exist are not touched, inputs may be NULL
            out_a, out_k, k = np.full(4, 7, np.uint32), np.full(4, 9, np.uint32), C.c_size_t(55)
            err = clo.api._Err()
            assert lib.clo_join_with_host_data(j.h, None, None, None, 0, None, 0, out_a.ctypes.data, None, out_k.ctypes.data, 4, C.byref(k), err.ref)
            err.raise_if_set()
            assert k.value == 0 and (out_a == 7).all() and (out_k == 9).all()
            j.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "join_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "join_host", "join_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("join host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(kind, keys_a, keys_b):
    """The join from its definition: two pointers over Python integers, group by group."""
    oa, ob = _py_order(keys_a), _py_order(keys_b)
    na, nb = len(oa), len(ob)
    emits_a, emits_b = kind in ("left", "full"), kind in ("right", "full")
    i = j = 0
    rows = []
    while i < na or j < nb:
        x = oa[i] if j >= nb else ob[j] if i >= na else min(oa[i], ob[j])
        m = n = 0
        while i + m < na and oa[i + m] == x:
            m += 1
        while j + n < nb and ob[j + n] == x:
            n += 1
        if m and n:
            rows += [(i + r, j + s, True) for r in range(m) for s in range(n)]
        elif m:
            rows += [(i + r, NONE, True) for r in range(m)] if emits_a else []
        else:
            rows += [(NONE, j + s, False) for s in range(n)] if emits_b else []
        i += m
        j += n
    return rows


def _inputs():
    rng = np.random.default_rng(12)
    for kt in KEY_TYPES:
        dt = np.dtype(clo.api.CLO_TYPE_NP[kt])
        pool = _pool(dt, rng)
        for na, nb in SIZES:
            a = sort_keys(pool[rng.integers(0, pool.size, na)])          # few distinct keys: runs in A and in B
            b = sort_keys(pool[rng.integers(0, pool.size, nb)])
            yield kt, dt, a, b


def test_model_sizes():
    assert SIZES == ((0, 0), (0, 9), (9, 0), (1, 1), (50, 70), (300, 11))


def test_the_model_against_a_two_pointer_loop():
    for kt, dt, a, b in _inputs():
        for kind in KINDS:
            rows = _loop(kind, a, b)
            ia, ib, keys, K = join(kind, a, b)
            what = (kt, kind, a.size, b.size)
            assert K == len(rows) <= max_rows(kind, a.size, b.size), what
            assert ia.dtype == np.uint32 and ib.dtype == np.uint32 and keys.dtype == dt
            assert ia.tolist() == [r[0] for r in rows] and ib.tolist() == [r[1] for r in rows], what
            want_keys = np.array([a[r[0]] if r[2] else b[r[1]] for r in rows], dtype=dt) if rows else np.zeros(0, dt)
            assert np.array_equal(keys.view(np.uint8), want_keys.view(np.uint8)), what
            assert (np.diff(order_key(keys).astype(object)) >= 0).all(), what            # sorted by key
            for cap in (0, 1, K // 2, K, K + 5):                                          # a capacity cuts the rows, not K
                ca, cb, ck, cK = join(kind, a, b, capacity=cap)
                assert cK == K and ca.tolist() == ia[:cap].tolist() and cb.tolist() == ib[:cap].tolist(), (what, cap)
                assert np.array_equal(ck.view(np.uint8), keys[:cap].view(np.uint8)), (what, cap)


def test_the_model_on_duplicate_free_inputs():
    """Without duplicates the inner join is the intersection with its indices: numpy's, on the order keys."""
    for kt, dt, a, b in _inputs():
        ua, ub = a[np.unique(order_key(a), return_index=True)[1]], b[np.unique(order_key(b), return_index=True)[1]]
        common, wa, wb = np.intersect1d(order_key(ua), order_key(ub), assume_unique=True, return_indices=True)
        ia, ib, keys, K = join("inner", ua, ub)
        assert K == common.size and np.array_equal(ia, wa) and np.array_equal(ib, wb) and np.array_equal(order_key(keys), common), (kt, ua.size, ub.size)
        assert join("left", ua, ub)[3] == ua.size and join("right", ua, ub)[3] == ub.size
        assert join("full", ua, ub)[3] == ua.size + ub.size - common.size


def test_the_model_keeps_bits_apart():
    """Equal iff the bits are equal: -0 and +0 are different keys, NaNs are equal by payload; integer extremes join."""
    for dt in (np.float16, np.float32, np.float64):
        z = np.array([-0.0, 0.0], dtype=dt)
        assert join("inner", z[:1], z[1:])[3] == 0
        ia, ib, keys, K = join("full", z[1:], z[:1])                     # B's -0 sorts below A's +0
        assert (ia.tolist(), ib.tolist(), K) == ([NONE, 0], [0, NONE], 2) and np.signbit(keys[0]) and not np.signbit(keys[1])
        s = _specials(dt)
        nans = sort_keys(s[[3, 4, 8, 9]])                                 # two negative and two positive payloads
        ia, ib, _, K = join("inner", nans, nans[1:3])
        assert (ia.tolist(), ib.tolist()) == ([1, 2], [0, 1])
    for dt in (np.int8, np.uint8, np.int16, np.uint16, np.int32, np.uint32, np.int64, np.uint64):
        info = np.iinfo(dt)
        a = np.array([info.min, info.min, 5, info.max], dtype=dt)
        b = np.array([info.min, info.max, info.max], dtype=dt)
        ia, ib, keys, K = join("inner", a, b)
        assert (ia.tolist(), ib.tolist()) == ([0, 1, 3, 3], [0, 0, 1, 2]) and keys.tolist() == [info.min, info.min, info.max, info.max]
