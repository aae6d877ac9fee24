"""CloReduceByKey (include/clo_reduce.h) on the CPU: the library exports the new public and thin-ABI entry points and
the headers declare them, every refusal comes back as CLO_ERROR_ARGS through an offline context before anything
touches a device (err == NULL included), and the C driver runs over the host stubs of the thin C-ABI
(tests/hoststub/*stub*.c, among them clo_hip_rbk_stub.c) under AddressSanitizer + UBSan, driven by
tests/rbk_host/rbk_host_test.c. The reference model the GPU tests compare against (rbk_model.py) is checked here
against per-key sums and np.unique."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from rbk_model import rbk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_reduce_by_key_new", "clo_reduce_by_key_destroy", "clo_reduce_by_key_with_device_data",
          "clo_reduce_by_key_with_host_data", "clo_reduce_by_key_get_context", "clo_reduce_by_key_get_key_type",
          "clo_reduce_by_key_get_key_size", "clo_reduce_by_key_get_value_type", "clo_reduce_by_key_get_value_size",
          "clo_reduce_by_key_get_sum_type", "clo_reduce_by_key_get_sum_size", "clo_reduce_by_key_get_op")
THIN = ("clo_hip_reduce_by_key", "clo_hip_reduce_by_key_workspace_bytes", "clo_hip_reduce_by_key_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_reduce.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert '#include "clo_reduce.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    assert clo.ReduceByKey is not None and "ReduceByKey" in clo.__all__


def test_tile_getter_and_workspace_size():
    lib = clo.api.lib
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = lib.clo_hip_reduce_by_key_tile(ks, vs)
            assert t >= 1024 and t % 1024 == 0, (ks, vs, t)
    assert lib.clo_hip_reduce_by_key_tile(3, 4) == 0 and lib.clo_hip_reduce_by_key_tile(4, 2) == 0
    sizes = [lib.clo_hip_reduce_by_key_workspace_bytes(n) for n in (0, 1, 1 << 20, 1 << 24, (1 << 32) - 1)]
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
        # values, an unknown op, options
        for vt, st in (("float", "float"), ("uint", "float"), ("uint", "double"), ("half", "uint"), ("double", "ulong"),
                       ("ushort", "uint"), ("short", "int"), ("uchar", "uint"), ("char", "long"), ("uint", "ushort"),
                       ("ulong", "uint"), ("long", "int")):
            _refused(lambda: clo.ReduceByKey(ctx, "uint", vt, st))
            assert not lib.clo_reduce_by_key_new(b"sum", None, ctx.h, 5, clo.clo_type(vt), clo.clo_type(st), None)   # err NULL
        for op in ("mean", "", "SUM", "count"):
            assert "operation" in _refused(lambda: clo.ReduceByKey(ctx, "uint", "uint", "uint", op=op))
            assert not lib.clo_reduce_by_key_new(op.encode(), None, ctx.h, 5, 5, 5, None)
        assert not lib.clo_reduce_by_key_new(None, None, ctx.h, 5, 5, 5, None)
        assert "options" in _refused(lambda: clo.ReduceByKey(ctx, "uint", "uint", "uint", options="tile=1"))
        clo.ReduceByKey(ctx, "uint", "uint", "uint", options="").close()
        # every key type, every value -> sum pair that is offered
        for kt in clo.CLO_TYPES:
            clo.ReduceByKey(ctx, kt).close()
        for vt, st in (("int", "int"), ("int", "uint"), ("uint", "int"), ("uint", "uint"), ("int", "long"), ("int", "ulong"),
                       ("uint", "long"), ("uint", "ulong"), ("long", "long"), ("long", "ulong"), ("ulong", "long"), ("ulong", "ulong")):
            for op in ("sum", "min", "max"):
                r = clo.ReduceByKey(ctx, "float", vt, st, op=op)
                assert (r.op, r.key_size, r.value_size, r.sum_size) == (op, 4, np.dtype(clo.api.CLO_TYPE_NP[vt]).itemsize,
                                                                      np.dtype(clo.api.CLO_TYPE_NP[st]).itemsize)
                r.close()

        # per call, through the host-data form (nothing is copied before the checks)
        r = clo.ReduceByKey(ctx, "uint", "uint", "uint")
        rmin = clo.ReduceByKey(ctx, "uint", "uint", "uint", op="min")
        k, v = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        ko, ao = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        m = C.c_size_t(7)
        p = lambda a: a.ctypes.data if a is not None else None

        def host(obj, kin, vin, kout, aout, count, n, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_reduce_by_key_with_host_data(obj.h, None, None, p(kin), p(vin), p(kout), p(aout), count, n,
                                                      err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        cnt = C.byref(m)
        assert "2^32" in host(r, k, v, ko, ao, cnt, 1 << 32)
        host(r, k, v, ko, ao, cnt, 1 << 32, with_err=False)
        assert "both" in host(r, k, v, None, None, cnt, 16)
        host(r, k, v, None, None, cnt, 16, with_err=False)
        assert "min / max" in host(rmin, k, None, ko, ao, cnt, 16)
        host(rmin, k, None, ko, ao, cnt, 16, with_err=False)
        assert "keys_in" in host(r, None, v, ko, ao, cnt, 16)
        assert "run count" in host(r, k, v, ko, ao, None, 16)
        # overlap: an output on, inside, or across the end of an input
        assert "overlaps" in host(r, k, v, k, ao, cnt, 16)
        host(r, k, v, k, ao, cnt, 16, with_err=False)
        assert "overlaps" in host(r, k, v, ko, v, cnt, 16)
        assert "overlaps" in host(r, k, v, v, ao, cnt, 16)
        both = np.zeros(40, np.uint32)
        assert "overlaps" in host(r, both[:16], v, both[15:31], ao, cnt, 16)     # one shared element
        assert "overlaps" in host(r, both[8:24], v, ko, both[0:16], cnt, 16)     # ends inside the keys
        assert "overlaps" in host(r, both[:16], both[16:32], both[17:33], ao, cnt, 16)
        assert m.value == 7   # a refused call wrote nothing
        # what is next to an input without touching it is accepted as far as the checks go: the call then fails for
        # want of a device, not with CLO_ERROR_ARGS
        err = clo.api._Err()
        assert not lib.clo_reduce_by_key_with_host_data(r.h, None, None, p(both[:16]), None, p(both[16:32]), p(ao), cnt, 16, err.ref)
        with pytest.raises(clo.CloError) as e:
            err.raise_if_set()
        assert e.value.domain == "ccl-hip-error-quark"
        # numel 0: no runs, no device
        err = clo.api._Err()
        assert lib.clo_reduce_by_key_with_host_data(r.h, None, None, None, None, p(ko), p(ao), cnt, 0, err.ref)
        err.raise_if_set()
        assert m.value == 0
        with pytest.raises(ValueError):   # the Python view checks the element sizes
            r.with_host_data(np.zeros(4, np.uint16))
        with pytest.raises(ValueError):
            r.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint64))
        r.close()
        rmin.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rbk_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "rbk_host", "rbk_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("rbk host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def test_the_reference_model():
    """rbk() against per-key sums and np.unique on sorted keys, and against a run-by-run loop on unsorted ones."""
    rng = np.random.default_rng(5)
    keys = np.sort(rng.integers(0, 50, 5000, dtype=np.uint32))
    vals = rng.integers(0, 1 << 32, 5000, dtype=np.uint32)
    uk, counts = np.unique(keys, return_counts=True)
    ko, ao, m = rbk(keys, None, "sum", np.uint32)
    assert m == uk.size and np.array_equal(ko, uk) and np.array_equal(ao, counts.astype(np.uint32))
    ko, ao, m = rbk(keys, vals, "sum", np.uint32)
    want = np.zeros(50, np.uint32)
    with np.errstate(over="ignore"):
        np.add.at(want, keys, vals)
    assert ao.dtype == np.uint32 and np.array_equal(ao, want[uk])            # wrapped modulo 2^32, not widened
    ko, ao, m = rbk(keys, vals, "sum", np.uint64)
    want = np.zeros(50, np.uint64)
    np.add.at(want, keys, vals.astype(np.uint64))
    assert np.array_equal(ao, want[uk]) and (ao > np.uint64(1 << 32)).any()
    sv = vals.view(np.int32)
    for op, f in (("min", min), ("max", max)):
        ko, ao, m = rbk(keys, sv, op, np.int64)
        assert np.array_equal(ao, np.array([f(int(x) for x in sv[keys == u]) for u in uk], dtype=np.int64))
    # unsorted: one row per stretch; float keys by their bits
    k = np.array([1.0, 1.0, -0.0, 0.0, 0.0, np.nan, np.nan, 1.0], dtype=np.float32)
    k[6] = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
    ko, ao, m = rbk(k, None, "sum", np.uint32)
    assert m == 6 and list(ao) == [2, 1, 2, 1, 1, 1] and np.array_equal(ko.view(np.uint32), k.view(np.uint32)[[0, 2, 3, 5, 6, 7]])
    assert rbk(k[:0], None, "sum", np.uint64)[2] == 0
