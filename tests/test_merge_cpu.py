"""CloMerge (include/clo_merge.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile getter answers, every refusal comes back as CLO_ERROR_ARGS through an offline context
before anything touches a device (err == NULL included) and leaves the outputs alone, two empty inputs succeed without a
device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among them
clo_hip_merge_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/merge_host/merge_host_test.c. The reference model the GPU tests compare against (merge_model.py) is checked here
against a two-pointer loop over Python integers and against np.sort(kind="stable")."""
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from merge_model import merge, order_key, sort_keys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_merge_new", "clo_merge_destroy", "clo_merge_with_device_data", "clo_merge_with_host_data",
          "clo_merge_get_context", "clo_merge_get_key_type", "clo_merge_get_key_size", "clo_merge_get_value_size")
THIN = ("clo_hip_merge", "clo_hip_merge_workspace_bytes", "clo_hip_merge_tile")
KEY_TYPES = ("char", "uchar", "short", "ushort", "int", "uint", "long", "ulong", "half", "float", "double")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_merge.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_merge.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Merge", "merge_tile"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_merge_tile_and_workspace_getters():
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.merge_tile(ks, vs)
            assert t >= 64 and t % 64 == 0, (ks, vs, t)
    for ks, vs in ((3, 0), (0, 0), (16, 4), (4, 2), (4, 1), (8, 16), (4, -4)):
        assert clo.merge_tile(ks, vs) == 0, (ks, vs)
    ws = clo.api.lib.clo_hip_merge_workspace_bytes
    assert ws(0, 0) == 0
    sizes = [ws(n, n // 3) for n in (0, 1, 63, 5000, 1 << 20, 1 << 24, 3 << 29)]
    assert sizes == sorted(sizes) and sizes[-1] < (64 << 20)                 # monotone, and small next to the data
    assert ws(1000, 24) == ws(24, 1000) == ws(1024, 0)                       # a function of n


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        # at construction: value sizes, options, key types
        for vs in (1, 2, 3, 5, 12, 16):
            assert "value_size" in _refused(lambda: clo.Merge(ctx, "uint", vs))
            assert not lib.clo_merge_new(None, ctx.h, 5, vs, None)           # err NULL
        for opt in ("descending", "tile=2304", " "):
            assert "options" in _refused(lambda: clo.Merge(ctx, "uint", 0, options=opt))
            assert not lib.clo_merge_new(opt.encode(), ctx.h, 5, 0, None)
        assert not lib.clo_merge_new(None, ctx.h, 11, 0, None)
        for kt in KEY_TYPES:                                                 # every key type, every value size, both spellings of no options
            for vs in (0, 4, 8):
                for opt in (None, ""):
                    m = clo.Merge(ctx, kt, vs, options=opt)
                    assert (m.key_type, m.key_size, m.value_size) == (clo.CLO_TYPES[kt], np.dtype(clo.api.CLO_TYPE_NP[kt]).itemsize, vs)
                    m.close()

        m0, m4, m8 = clo.Merge(ctx, "uint", 0), clo.Merge(ctx, "uint", 4), clo.Merge(ctx, "uint", 8)
        a, b, va, vb = (np.zeros(16, np.uint32) for _ in range(4))
        va8, vb8 = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
        ko, vo = np.arange(100, 132, dtype=np.uint32), np.arange(200, 232, dtype=np.uint32)
        vo8 = np.arange(300, 332, dtype=np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(obj, ka, xa, na, kb, xb, nb, out_k, out_v, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_merge_with_host_data(obj.h, None, None, p(ka), p(xa), na, p(kb), p(xb), nb, p(out_k), p(out_v),
                                              err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args):
            assert word in host(*args), args
            host(*args, with_err=False)

        both("2^32", m4, a, va, (1 << 32) - 16, b, vb, 16, ko, vo)
        both("2^32", m0, a, None, 1 << 32, b, None, 0, ko, None)
        both("2^32", m0, a, None, 1 << 63, b, None, 1 << 63, ko, None)       # the sum wraps to 0
        both("keys_a", m0, None, None, 16, b, None, 16, ko, None)
        both("keys_b", m0, a, None, 16, None, None, 16, ko, None)
        both("both be given", m4, a, va, 16, b, None, 16, ko, vo)            # exactly one values array NULL
        both("both be given", m4, a, None, 16, b, vb, 16, ko, vo)
        both("value_size 0", m0, a, va, 16, b, vb, 16, ko, None)             # values with value_size 0
        both("value_size 0", m0, a, None, 16, b, None, 16, ko, vo)
        both("values_out", m4, a, va, 16, b, vb, 16, ko, None)               # values_out NULL with value_size > 0
        both("values_out", m4, a, None, 16, b, None, 16, ko, None)
        both("value_size of 4", m8, a, None, 16, b, None, 16, ko, vo8)       # NULL values with value_size 8
        both("value_size of 4", m8, a, None, 16, b, None, 0, ko, vo8)
        both("both NULL", m0, a, None, 16, b, None, 16, None, None)          # both outputs NULL
        both("both NULL", m4, a, va, 16, b, vb, 16, None, None)

        # overlap: an output on, inside, across the end of an input or of the other output, or sharing one element
        one = np.zeros(160, np.uint32)
        O = "overlaps"
        both(O, m0, a, None, 16, b, None, 16, a, None)                                       # on keys_a (and too small: never looked at)
        both(O, m0, one[0:16], None, 16, one[40:56], None, 16, one[40:72], None)             # starts on keys_b
        both(O, m0, one[8:24], None, 16, b, None, 16, one[0:32], None)                       # keys_a inside keys_out
        both(O, m0, one[0:16], None, 16, b, None, 16, one[15:47], None)                      # one shared element with keys_a's end
        both(O, m0, a, None, 16, one[32:48], None, 16, one[1:33], None)                      # one shared element with keys_b's start
        both(O, m4, a, one[0:16], 16, b, vb, 16, ko, one[8:40])                              # values_out across the end of values_a
        both(O, m4, a, va, 16, b, one[40:56], 16, one[30:62], vo)                            # keys_out over values_b
        both(O, m4, a, va, 16, b, vb, 16, one[0:32], one[31:63])                             # the two outputs share one element
        both(O, m4, a, va, 16, b, vb, 16, one[0:32], one[0:32])                              # the two outputs on each other
        both(O, m4, a, None, 16, b, None, 16, one[0:32], one[16:48])                         # argmerge: the same rule
        both(O, m8, a, va8, 16, b, vb8, 16, vo8[0:32].view(np.uint32)[0:32], vo8)            # keys_out inside values_out
        assert np.array_equal(ko, np.arange(100, 132)) and np.array_equal(vo, np.arange(200, 232))   # nothing was written
        assert np.array_equal(vo8, np.arange(300, 332)) and not one.any() and not a.any() and not va.any()

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS
        for obj, args in ((m0, (one[0:16], None, 16, one[16:32], None, 16, one[32:64], None)),
                          (m4, (one[0:16], one[64:80], 16, one[16:32], one[80:96], 16, one[32:64], one[96:128])),
                          (m4, (one[0:16], None, 16, one[16:32], None, 16, None, one[32:64]))):
            err = clo.api._Err()
            ka, xa, na, kb, xb, nb, out_k, out_v = args
            assert not lib.clo_merge_with_host_data(obj.h, None, None, p(ka), p(xa), na, p(kb), p(xb), nb, p(out_k), p(out_v), err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark"
        assert not one.any()

        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            m4.with_host_data(np.zeros(4, np.uint16), np.zeros(4, np.uint16))
        with pytest.raises(ValueError):
            m4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint64), np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            m0.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            m4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(3, np.uint32), np.zeros(4, np.uint32))
        for m in (m0, m4, m8):
            m.close()
    finally:
        ctx.close()


def test_both_inputs_empty_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        empty = np.zeros(0, np.float32)
        for vs in (0, 4, 8):
            m = clo.Merge(ctx, "float", vs)
            ko, vo = m.with_host_data(empty, empty)
            assert ko.size == 0 and ko.dtype == np.float32 and (vo is None if vs == 0 else vo.size == 0)
            # raw: outputs that exist are not touched, inputs may be NULL
            out_k, out_v = np.full(4, 7, np.uint32), np.full(4, 9, np.uint64)
            err = clo.api._Err()
            assert lib.clo_merge_with_host_data(m.h, None, None, None, None, 0, None, None, 0, out_k.ctypes.data,
                                                out_v.ctypes.data if vs else None, err.ref)
            err.raise_if_set()
            assert (out_k == 7).all() and (out_v == 9).all()
            m.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "merge_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "merge_host", "merge_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("merge host ok") == 1, out[-4000:]
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


def _loop(keys_a, keys_b):
    """The definition, two pointers over Python integers: from A while a <= b."""
    oa, ob = _py_order(keys_a), _py_order(keys_b)
    i = j = 0
    p = []
    while i < len(oa) or j < len(ob):
        if j >= len(ob) or (i < len(oa) and oa[i] <= ob[j]):
            p.append(i)
            i += 1
        else:
            p.append(len(oa) + j)
            j += 1
    return np.array(p, dtype=np.uint32)


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
    rng = np.random.default_rng(11)
    for kt in KEY_TYPES:
        dt = np.dtype(clo.api.CLO_TYPE_NP[kt])
        if dt.kind == "f":
            pool = np.concatenate((_specials(dt), np.array([-2.5, -1e-3, 3.0, 0.5, 7.0], dtype=dt)))
        else:
            info = np.iinfo(dt)
            pool = np.array([info.min, info.max, 0, 1, 5, 6] + ([-1, -2, -7] if dt.kind == "i" else [info.max - 3]), dtype=dt)
        for na, nb in ((0, 0), (0, 9), (9, 0), (1, 1), (50, 70), (300, 11)):
            a = sort_keys(pool[rng.integers(0, pool.size, na)])          # few distinct keys: ties inside and across A and B
            b = sort_keys(pool[rng.integers(0, pool.size, nb)])
            keys_out, p = merge(a, b)
            assert keys_out.dtype == dt and p.dtype == np.uint32
            assert np.array_equal(p, _loop(a, b)), (kt, na, nb)
            cat = np.concatenate((a, b))
            assert np.array_equal(keys_out.view(np.uint8), cat[p].view(np.uint8))
            # against np.sort(kind="stable") of the order keys, and of (order key, index) pairs: the permutation is the stable one
            ok = order_key(cat)
            assert np.array_equal(order_key(keys_out), np.sort(ok, kind="stable"))
            assert np.array_equal(ok[p], np.sort(ok, kind="stable")) and np.array_equal(np.sort(p), np.arange(na + nb))
            same = ok[p][1:] == ok[p][:-1]
            assert (p[1:][same] > p[:-1][same]).all()                     # equal keys: A before B, input order kept
            if dt.kind != "f" and na + nb:
                assert np.array_equal(keys_out, np.sort(cat, kind="stable"))
    # equal iff the bits are equal: -0.0 sorts below +0.0, NaNs of both signs at the ends, payloads ordered
    for dt in (np.float16, np.float32, np.float64):
        s = _specials(dt)
        got = sort_keys(s[::-1].copy())
        neg, pos = s[:5], s[5:]
        want = np.concatenate((neg[::-1], pos))
        assert np.array_equal(got.view(np.uint8), want.view(np.uint8)), dt
        z = np.array([0.0, -0.0], dtype=dt)
        keys_out, p = merge(z[:1], z[1:])                                 # A = [+0], B = [-0]: B's element comes first
        assert p.tolist() == [1, 0] and np.signbit(keys_out[0]) and not np.signbit(keys_out[1])
        keys_out, p = merge(z[1:], z[:1])
        assert p.tolist() == [0, 1]
        n1 = s[3:4]                                                       # one -NaN in A, the same bits in B: a tie, A first
        assert merge(n1, n1)[1].tolist() == [0, 1]
