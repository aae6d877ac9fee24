"""Sorting by key (clo_sort_by_key_with_device_data / _with_host_data, include/clo_sort.h) on the CPU: the library
exports the new entry points, refusals come back through an offline context before anything touches a device, and
the satradix driver's by-key path runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among them
clo_hip_kv_stub.c) under AddressSanitizer + UBSan, driven by tests/kv_host/kv_host_test.c: every key type, a key
field inside the element, values given and NULL, keys_out given and NULL, in place, host data, every refusal.
(A run-time compiled get_key needs hiprtc, which the stubs do not have: that refusal is checked on the GPU.)"""
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exports():
    for n in ("clo_sort_by_key_with_device_data", "clo_sort_by_key_with_host_data", "clo_hip_radix_sort_kv",
              "clo_hip_radix_kv_workspace_bytes"):
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_sort.h")).read()
    assert "clo_sort_by_key_with_device_data" in text and "clo_sort_by_key_with_host_data" in text


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    try:
        for algo, dtype in (("sbitonic", np.uint32), ("abitonic", np.uint32), ("gselect", np.uint32), ("satradix", np.uint64)):
            s = clo.Sorter(algo, ctx, dtype)
            with pytest.raises(clo.CloError) as e:
                s.by_key_with_host_data(np.zeros(4, dtype=dtype))
            assert e.value.code == CLO_ERROR_ARGS, algo
            s.close()
        s = clo.Sorter("satradix", ctx, "uint")
        lib = clo.api.lib
        err = clo.api._Err()
        assert not lib.clo_sort_by_key_with_host_data(s.h, None, None, np.zeros(4, np.uint32).ctypes.data, None, None,
                                                      None, 4, 0, err.ref)   # values_out NULL
        with pytest.raises(clo.CloError) as e:
            err.raise_if_set()
        assert e.value.code == CLO_ERROR_ARGS and "values_out" in e.value.message
        assert not lib.clo_sort_by_key_with_host_data(s.h, None, None, np.zeros(4, np.uint32).ctypes.data, None, None,
                                                      np.zeros(4, np.uint32).ctypes.data, 1 << 32, 0, err.ref)
        with pytest.raises(clo.CloError) as e:
            err.raise_if_set()
        assert e.value.code == CLO_ERROR_ARGS and "2^32" in e.value.message
        assert not lib.clo_sort_by_key_with_host_data(s.h, None, None, None, None, None, None, 4, 0, None)   # err NULL
        with pytest.raises(ValueError):   # the Python view checks the element size
            s.by_key_with_host_data(np.zeros(4, dtype=np.uint16))
        s.close()
    finally:
        ctx.close()


def test_by_key_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "kv_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "kv_host", "kv_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "kv host ok" in r.stdout, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]
