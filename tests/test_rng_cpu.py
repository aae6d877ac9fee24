"""CloRng on the CPU: known-answer values pin the numpy model (tests/rng_model.py), the C boundary exports the new
interface, argument errors come back through an offline context, and the C driver (cl_ops_amd/csrc/clo_rng.c) runs
every seed type and error path over the host stub of the thin C-ABI under AddressSanitizer + UBSan."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd import _hip
from cl_ops_amd.api import CLO_ERROR_ARGS, CLO_ERROR_IMPL_NOT_FOUND
import rng_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_model_known_answers():
    # java.util.Random(seed).nextInt(): the lcg from the scrambled seed, top 32 of 48 bits
    for seed, exp in ((42, -1170105035), (0, -1155484576)):
        _, x = M.step("lcg", np.array([seed ^ 0x5DEECE66D], dtype=np.uint64))
        assert int(x.view(np.int32)[0]) == exp
    # Marsaglia's xor128 from its published state
    st = np.array([[123456789, 362436069, 521288629, 88675123]], dtype=np.uint32)
    got = []
    for _ in range(3):
        st, x = M.step("xorshift128", st)
        got.append(int(x[0]))
    assert got == [3701687786, 458299110, 2500872618]
    # Park & Miller's check: the 10 000th state from 1
    st = np.array([1], dtype=np.int32)
    for _ in range(10000):
        st, _ = M.step("parkmiller", st)
    assert int(st[0]) == 1043618065
    # MT19937 init_genrand(5489)
    assert int(M.host_mt_words(5489, 1)[0]) == 3499211612


def test_model_rules():
    # parkmiller's remainder truncates towards zero for negative states (C's %), as upstream's OpenCL
    s, x = M.step("parkmiller", np.array([-5, -2147483648, 2147483647], dtype=np.int32))
    assert list(s) == [-84035, int(np.fmod(-2147483648 * 16807, 2147483647)), 0]
    # zero states stay zero (xorshift64 / xorshift128 / parkmiller), upstream behaviour
    for name in ("xorshift64", "xorshift128", "parkmiller"):
        st = M.ulong2state(name, np.zeros(1, dtype=np.uint64))
        st, x = M.step(name, st)
        assert not np.any(st) and not np.any(x)
    # the fill's index rule: state i % S makes draw i // S
    states = M.dev_gid_states("lcg", 3, 10)
    out, fin = M.fill("lcg", states, 7)
    st = states.copy()
    exp = []
    for i in range(7):
        s1, x = M.step("lcg", st[i % 3:i % 3 + 1])
        st[i % 3] = s1[0]
        exp.append(int(x[0]))
    assert list(out) == exp and np.array_equal(fin, st)
    # mwc64x: the output is taken before the step, the seed's low word is x
    st = M.ulong2state("mwc64x", np.array([(7 << 32) | 5], dtype=np.uint64))
    assert list(st[0]) == [5, 7]
    _, x = M.step("mwc64x", st)
    assert int(x[0]) == 5 ^ 7
    assert list(M.ulong2state("tauslcg", np.array([(9 << 32) | 4], dtype=np.uint64))[0]) == [4, 9, 4, 9]


def test_boundary_exports_and_infos():
    for n in ("clo_rng_new", "clo_rng_destroy", "clo_rng_get_source", "clo_rng_get_device_seeds", "clo_rng_get_size",
              "clo_rng_fill", "clo_rng_get_infos", "clo_hip_rng_fill", "clo_hip_rng_init", "clo_hip_rng_init_jit",
              "clo_hip_rng_device_source"):
        assert hasattr(clo.api.lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", _hip.LIB_PATH], capture_output=True, text=True).stdout
    assert "clo_rng_infos" not in out     # a function and a macro, not a data symbol
    from cl_ops_amd.rng import rng_infos
    assert rng_infos() == [("lcg", "#define CLO_RNG_LCG 1\n", 8), ("xorshift64", "#define CLO_RNG_XORSHIFT64 1\n", 8),
                           ("xorshift128", "#define CLO_RNG_XORSHIFT128 1\n", 16), ("mwc64x", "#define CLO_RNG_MWC64X 1\n", 8),
                           ("parkmiller", "#define CLO_RNG_PARKMILLER 1\n", 4), ("tauslcg", "#define CLO_RNG_TAUSLCG 1\n", 16)]
    assert clo.rng_names() == M.NAMES
    text = open(os.path.join(ROOT, "include", "clo_rng.h")).read()
    assert '#define CLO_RNG_IMPLS "lcg, xorshift64, xorshift128, mwc64x, parkmiller, tauslcg"' in text
    assert "#define clo_rng_infos (clo_rng_get_infos())" in text
    assert '#include "clo_rng.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()


def test_device_source_is_the_header():
    src = clo.api.lib.clo_hip_rng_device_source
    src.restype = C.c_char_p
    assert src().decode() == open(os.path.join(ROOT, "include", "clo_rng", "clo_rng_device.hpp")).read()


def test_errors_through_an_offline_context():
    ctx = clo.Context(offline=True)
    try:
        for args, code in (
            (("mt19937", ctx, None), CLO_ERROR_IMPL_NOT_FOUND),
            (("", ctx, None), CLO_ERROR_IMPL_NOT_FOUND),
            (("lcg", ctx, None, "dev_gid", np.zeros(4, np.uint64), 4), CLO_ERROR_ARGS),
            (("lcg", ctx, None, "host_mt", np.zeros(4, np.uint64), 4), CLO_ERROR_ARGS),
            (("lcg", ctx, None, "ext_host", None, 4), CLO_ERROR_ARGS),
            (("lcg", ctx, None, "ext_dev", None, 4), CLO_ERROR_ARGS),
            (("lcg", ctx, None, "dev_gid", None, 0), CLO_ERROR_ARGS),
            (("lcg", ctx, None, 9, None, 4), CLO_ERROR_ARGS),
        ):
            with pytest.raises(clo.CloError) as e:
                clo.Rng(*args)
            assert e.value.code == code, args
        with pytest.raises(clo.CloError) as e:   # a seed type that needs a queue, without one
            clo.Rng("lcg", ctx, None, "dev_gid", None, 4)
        assert e.value.code == CLO_ERROR_ARGS
        lib = clo.api.lib
        err = clo.api._Err()
        assert not lib.clo_rng_fill(None, None, None, 4, 32, 0, err.ref)
        with pytest.raises(clo.CloError) as e:
            err.raise_if_set()
        assert e.value.code == CLO_ERROR_ARGS
        assert not lib.clo_rng_new(b"nosuch", 0, None, 4, 0, None, ctx.h, None, None)   # err == NULL is accepted
    finally:
        ctx.close()


def test_rng_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "rng_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "rng_host", "rng_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and "rng host ok" in r.stdout, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]
