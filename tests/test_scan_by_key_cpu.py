"""CloScanByKey (include/clo_scan_by_key.h) on the CPU: the library exports the new public and thin-ABI entry points
and the headers declare them, every refusal comes back as CLO_ERROR_ARGS through an offline context before anything
touches a device (err == NULL included), the in-place rule lets exactly `out == values_in` of equal widths through,
and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among them
clo_hip_sbk_stub.c) under AddressSanitizer + UBSan, driven by tests/sbk_host/sbk_host_test.c. The reference model
the GPU tests compare against (sbk_model.py) is checked here against a plain Python loop and, on sorted keys,
against per-key np.cumsum."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from sbk_model import sbk, sbk_loop, identity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_scan_by_key_new", "clo_scan_by_key_destroy", "clo_scan_by_key_with_device_data",
          "clo_scan_by_key_with_host_data", "clo_scan_by_key_get_context", "clo_scan_by_key_get_key_type",
          "clo_scan_by_key_get_key_size", "clo_scan_by_key_get_value_type", "clo_scan_by_key_get_value_size",
          "clo_scan_by_key_get_sum_type", "clo_scan_by_key_get_sum_size", "clo_scan_by_key_get_op",
          "clo_scan_by_key_get_inclusive")
THIN = ("clo_hip_scan_by_key", "clo_hip_scan_by_key_workspace_bytes", "clo_hip_scan_by_key_tile")
PAIRS = (("int", "int"), ("int", "uint"), ("uint", "int"), ("uint", "uint"), ("int", "long"), ("int", "ulong"),
         ("uint", "long"), ("uint", "ulong"), ("long", "long"), ("long", "ulong"), ("ulong", "long"), ("ulong", "ulong"))


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_scan_by_key.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert "CLO_SCAN_BY_KEY_OPS" in text
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_scan_by_key.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    assert clo.ScanByKey is not None and "ScanByKey" in clo.__all__ and "scan_by_key_tile" in clo.__all__
    assert os.path.exists(os.path.join(ROOT, "tests", "hoststub", "clo_hip_sbk_stub.c"))


def test_tile_getter_and_workspace_size():
    lib = clo.api.lib
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = lib.clo_hip_scan_by_key_tile(ks, vs)
            assert t >= 1024 and t % 1024 == 0, (ks, vs, t)
            assert clo.scan_by_key_tile(ks, vs) == t
    assert lib.clo_hip_scan_by_key_tile(3, 4) == 0 and lib.clo_hip_scan_by_key_tile(4, 2) == 0
    sizes = [lib.clo_hip_scan_by_key_workspace_bytes(n) for n in (0, 1, 1 << 20, 1 << 24, (1 << 32) - 1)]
    assert sizes == sorted(sizes) and sizes[0] > 0 and sizes[-1] < (64 << 20)


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        # at construction: floating-point values or sums, values narrower than 4 bytes, a sum narrower than the
        # values, an unknown op, bad options
        for vt, st in (("float", "float"), ("uint", "float"), ("uint", "double"), ("half", "uint"), ("double", "ulong"),
                       ("ushort", "uint"), ("short", "int"), ("uchar", "uint"), ("char", "long"), ("uint", "ushort"),
                       ("ulong", "uint"), ("long", "int")):
            _refused(lambda: clo.ScanByKey(ctx, "uint", vt, st))
            assert not lib.clo_scan_by_key_new(b"sum", None, ctx.h, 5, clo.clo_type(vt), clo.clo_type(st), None)   # err NULL
        for op in ("mean", "", "SUM", "count"):
            assert "operation" in _refused(lambda: clo.ScanByKey(ctx, "uint", "uint", "uint", op=op))
            assert not lib.clo_scan_by_key_new(op.encode(), None, ctx.h, 5, 5, 5, None)
        assert not lib.clo_scan_by_key_new(None, None, ctx.h, 5, 5, 5, None)
        for options in ("inclusive=2", "tile=1", "inclusive", "inclusive=", "inclusive=1,tile=1", "inclusive=yes", "Inclusive=1"):
            err = clo.api._Err()
            assert not lib.clo_scan_by_key_new(b"sum", options.encode(), ctx.h, 5, 5, 5, err.ref)
            assert "options" in _refused(err.raise_if_set), options
            assert not lib.clo_scan_by_key_new(b"sum", options.encode(), ctx.h, 5, 5, 5, None)
        for options, want in ((None, False), ("", False), ("inclusive=0", False), ("inclusive=1", True)):
            err = clo.api._Err()
            h = lib.clo_scan_by_key_new(b"sum", options.encode() if options is not None else None, ctx.h, 5, 5, 5, err.ref)
            err.raise_if_set()
            assert h and bool(lib.clo_scan_by_key_get_inclusive(h)) == want, options
            lib.clo_scan_by_key_destroy(h)
        for flag in (False, True):
            x = clo.ScanByKey(ctx, "uint", inclusive=flag)
            assert x.inclusive is flag
            x.close()
        # every key type, every value -> sum pair that is offered
        for kt in clo.CLO_TYPES:
            clo.ScanByKey(ctx, kt).close()
        for vt, st in PAIRS:
            for op in ("sum", "min", "max"):
                r = clo.ScanByKey(ctx, "float", vt, st, op=op, inclusive=(op == "min"))
                assert (r.op, r.key_size, r.value_size, r.sum_size, r.inclusive) == (
                    op, 4, np.dtype(clo.api.CLO_TYPE_NP[vt]).itemsize, np.dtype(clo.api.CLO_TYPE_NP[st]).itemsize, op == "min")
                assert (r.key_type, r.value_type, r.sum_type) == (clo.clo_type("float"), clo.clo_type(vt), clo.clo_type(st))
                r.close()

        # per call, through the host-data form (nothing is copied before the checks)
        r = clo.ScanByKey(ctx, "uint", "uint", "uint")
        rw = clo.ScanByKey(ctx, "uint", "uint", "ulong")
        rmin = clo.ScanByKey(ctx, "uint", "uint", "uint", op="min")
        rmax = clo.ScanByKey(ctx, "uint", "uint", "uint", op="max", inclusive=True)
        k, v, o = np.zeros(16, np.uint32), np.zeros(17, np.uint32), np.full(16, 7, np.uint32)
        p = lambda a: a.ctypes.data if a is not None else None

        def host(obj, kin, vin, out, n, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_scan_by_key_with_host_data(obj.h, None, None, p(kin), p(vin), p(out), n, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        assert "2^32" in host(r, k, v, o, 1 << 32)
        host(r, k, v, o, 1 << 32, with_err=False)
        assert "keys_in" in host(r, None, v, o, 16)
        host(r, None, v, o, 16, with_err=False)
        assert "data_out" in host(r, k, v, None, 16)
        host(r, k, v, None, 16, with_err=False)
        for obj in (rmin, rmax):
            assert "min / max" in host(obj, k, None, o, 16)
            host(obj, k, None, o, 16, with_err=False)
        # overlap: out on the keys, across their end, shifted by one element over the values (either way), and on
        # the values with a wider sum type
        assert "keys_in" in host(r, k, v, k, 16)
        host(r, k, v, k, 16, with_err=False)
        both = np.zeros(40, np.uint32)
        assert "keys_in" in host(r, both[:16], v, both[15:31], 16)            # one shared element
        assert "values_in" in host(r, k, v[:16], v[1:17], 16)                 # shifted up by one element
        host(r, k, v[:16], v[1:17], 16, with_err=False)
        assert "values_in" in host(r, k, v[1:17], v[:16], 16)                 # shifted down by one element
        assert "values_in" in host(r, k, both[8:24], both[23:39], 16)         # one shared element
        assert "values_in" in host(rw, k[:8], v[:8], v, 8)                    # the same address, a wider sum type
        host(rw, k[:8], v[:8], v, 8, with_err=False)
        assert (o == 7).all() and not v.any()   # a refused call wrote nothing
        # what passes the checks fails for want of a device, not with CLO_ERROR_ARGS: exactly in place with equal
        # widths, and an output next to an input without touching it
        for vin, out, obj in ((v[:16], v[:16], r), (both[:16], both[16:32], r), (None, both[16:32], r), (v[:8], both[8:24].view(np.uint64), rw)):
            err = clo.api._Err()
            assert not lib.clo_scan_by_key_with_host_data(obj.h, None, None, p(k), p(vin), p(out), out.size, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", e.value
        # numel 0: nothing to do, no device
        err = clo.api._Err()
        assert lib.clo_scan_by_key_with_host_data(r.h, None, None, None, None, p(o), 0, err.ref)
        err.raise_if_set()
        assert lib.clo_scan_by_key_with_host_data(r.h, None, None, None, None, None, 0, None)
        assert r.with_host_data(k[:0], v[:0]).size == 0
        assert (o == 7).all()
        with pytest.raises(ValueError):   # the Python view checks the element sizes
            r.with_host_data(np.zeros(4, np.uint16))
        with pytest.raises(ValueError):
            r.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            rw.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), out=np.zeros(4, np.uint32))
        for x in (r, rw, rmin, rmax):
            x.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "sbk_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "sbk_host", "sbk_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("sbk host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _runs(n, mean, rng):
    heads = rng.random(n) < 1.0 / mean
    return np.cumsum(heads)


@pytest.mark.parametrize("mean", [1, 3, 50, 5000])
def test_the_model_against_a_plain_loop(mean):
    """Every value -> sum pair, op and both kinds; values over the full range, so 32-bit sums wrap."""
    rng = np.random.default_rng(mean)
    n = 3000
    keys = (_runs(n, mean, rng) % 7).astype(np.uint16)    # few distinct keys: equal keys in separate runs too
    raw = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    np_of = clo.api.CLO_TYPE_NP
    for vt, st in PAIRS:
        values = raw.astype({4: np.uint32, 8: np.uint64}[np.dtype(np_of[vt]).itemsize]).view(np_of[vt])
        for op in ("sum", "min", "max"):
            for inclusive in (False, True):
                got = sbk(keys, values, op, np_of[st], inclusive)
                want = sbk_loop(keys, values, op, np_of[st], inclusive)
                assert got.dtype == np.dtype(np_of[st]) and np.array_equal(got, want), (vt, st, op, inclusive)
    for st in ("uint", "int", "ulong", "long"):
        for inclusive in (False, True):
            assert np.array_equal(sbk(keys, None, "sum", np_of[st], inclusive), sbk_loop(keys, None, "sum", np_of[st], inclusive))


def test_the_model_on_sorted_keys_and_special_keys():
    """Against per-key np.cumsum / np.minimum.accumulate on sorted keys; float keys by their bits; the identities."""
    rng = np.random.default_rng(5)
    keys = np.sort(rng.integers(0, 50, 5000, dtype=np.uint32))
    vals = rng.integers(0, 1 << 32, 5000, dtype=np.uint32)
    incl32, incl64 = sbk(keys, vals, "sum", np.uint32, True), sbk(keys, vals, "sum", np.uint64, True)
    excl64 = sbk(keys, vals, "sum", np.uint64, False)
    rank = sbk(keys, None, "sum", np.uint32)
    mn, mx = sbk(keys, vals.view(np.int32), "min", np.int64, True), sbk(keys, vals.view(np.int32), "max", np.int32, True)
    for u in np.unique(keys):
        m = keys == u
        c = np.cumsum(vals[m], dtype=np.uint64)
        assert np.array_equal(incl64[m], c) and np.array_equal(incl32[m], c.astype(np.uint32))   # wrapped, not widened
        assert np.array_equal(excl64[m], c - vals[m]) and excl64[m][0] == 0
        assert np.array_equal(rank[m], np.arange(m.sum(), dtype=np.uint32))
        assert np.array_equal(mn[m], np.minimum.accumulate(vals.view(np.int32)[m]).astype(np.int64))
        assert np.array_equal(mx[m], np.maximum.accumulate(vals.view(np.int32)[m]))
    assert (incl64 > np.uint64(1 << 32)).any() and (incl32 < vals).any()
    # unsorted: one run per stretch; float keys by their bits
    k = np.array([1.0, 1.0, -0.0, 0.0, 0.0, np.nan, np.nan, 1.0], dtype=np.float32)
    k[6] = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
    assert list(sbk(k, None, "sum", np.uint32)) == [0, 1, 0, 0, 1, 0, 0, 0]
    assert list(sbk(k, None, "sum", np.uint64, True)) == [1, 2, 1, 1, 2, 1, 1, 1]
    v = np.array([5, -3, 7, 2, 9, -1, 4, 6], np.int32)
    assert list(sbk(k, v, "min", np.int32)) == [2**31 - 1, 5, 2**31 - 1, 2**31 - 1, 2, 2**31 - 1, 2**31 - 1, 2**31 - 1]
    assert list(sbk(k, v, "max", np.int64)) == [-2**63, 5, -2**63, -2**63, 2, -2**63, -2**63, -2**63]
    assert list(sbk(k, v.view(np.uint32), "max", np.uint32, True)) == [5, 2**32 - 3, 7, 2, 9, 2**32 - 1, 4, 6]
    assert identity("min", np.uint64) == np.uint64(2**64 - 1) and identity("max", np.uint32) == 0 and identity("sum", np.int32) == 0
    assert sbk(k[:0], None, "sum", np.uint64).size == 0
