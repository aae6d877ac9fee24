"""CloBucket (include/clo_bucket.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the header names what is out of scope, the tile and workspace getters answer, every refusal comes
back as CLO_ERROR_ARGS through an offline context before anything touches a device (err == NULL included) and leaves the
outputs alone, numel == 0 succeeds without a device, the driver stands on the shared host layer, the host stub answers
the thin ABI's status-code table, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c,
among them clo_hip_bucket_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/bucket_host/bucket_host_test.c. The reference model the GPU tests compare against (bucket_model.py) is checked
here against a plain Python loop over Python integers, and the strata of the GPU fuzz (bucket_strata.py) are shown to
reach what they are for."""
import ctypes as C
import glob
import os
import re
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from bucket_model import COUNT_NP, bin_or_rest, bucket
from bucket_strata import BIN_COUNTS, COUNT_TYPES, DISTS, KEY_TYPES, LOWERS, MODES, NP, SEED, SHIFTS, SIZES, STRATA, strata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_bucket_new", "clo_bucket_destroy", "clo_bucket_with_device_data", "clo_bucket_with_host_data", "clo_bucket_get_context",
          "clo_bucket_get_key_type", "clo_bucket_get_key_size", "clo_bucket_get_value_size", "clo_bucket_get_count_type", "clo_bucket_get_count_size")
THIN = ("clo_hip_bucket", "clo_hip_bucket_workspace_bytes", "clo_hip_bucket_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_bucket.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert "#define CLO_BUCKET_MAX_BINS 65535" in text and clo.BUCKET_MAX_BINS == 65535
    for word in ("more than 65 535 bins", "floating-point keys", "get_key or run-time", "numel >= 2^32", "values wider than 8 bytes",
                 "numel read from device memory", "dropping the rest", "large-bin histogram"):      # what the header says is out of scope
        assert word in " ".join(text.split()).replace(" * ", " "), word
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert "#define CLO_HIP_BUCKET_MAX_BINS 65535" in text
    assert "#define CLO_HIP_BUCKET_SCAN_GROUP %d\n" % clo.BUCKET_SCAN_GROUP in text and "#define CLO_HIP_BUCKET_SCAN_TRIP %d\n" % clo.BUCKET_SCAN_TRIP in text
    assert '#include "clo_bucket.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Bucket", "bucket_tile", "BUCKET_MAX_BINS"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert "bucket-partition" in clo.__doc__


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    text = open(os.path.join(ROOT, "cl_ops_amd", "csrc", "clo_bucket.c")).read()
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text and "clo_ranges_conflict(" in text


def test_tile_and_workspace_getters():
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.bucket_tile(ks, vs)
            assert t >= 1024 and t % 256 == 0 and t <= 65536, (ks, vs, t)
    assert clo.bucket_tile(4) == clo.bucket_tile(4, 0)
    ws = clo.api.lib.clo_hip_bucket_workspace_bytes
    for ks, vs in ((3, 4), (16, 0), (0, 0), (4, 2), (4, 16), (-1, 4), (4, -4)):
        assert clo.bucket_tile(ks, vs) == 0 and ws(1000, ks, vs, 10) == 0, (ks, vs)
    T = clo.bucket_tile(4, 4)
    sizes = (0, 1, 63, T - 1, T, T + 1, 17 * T, 1 << 20, (1 << 32) - 1)
    bins = (1, 2, 254, 255, 256, 257, 4096, 65535)
    for ks, vs in ((1, 0), (4, 4), (8, 8)):
        assert all(ws(0, ks, vs, b) == 0 for b in bins)
        for b in bins:
            col = [ws(n, ks, vs, b) for n in sizes]
            assert col == sorted(col) and all(x % 256 == 0 for x in col) and all(x > 0 for x in col[1:]), (ks, vs, b, col)   # monotone in numel
        for n in sizes[1:]:
            row = [ws(n, ks, vs, b) for b in bins]
            assert row == sorted(row), (ks, vs, n, row)                  # ... and in num_bins
            tiles = -(-n // T)
            assert ws(n, ks, vs, 255) >= 12 * 256 * tiles                # 4 bytes per counter and 8 per end
            assert ws(n, ks, vs, 256) >= ws(n, ks, vs, 255) + n * (ks + vs) + 4 * 256   # two passes: the rows between them, the histogram


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for kt in ("half", "float", "double"):
            assert "integers" in _refused(lambda: clo.Bucket(ctx, kt))
            assert not lib.clo_bucket_new(None, ctx.h, clo.CLO_TYPES[kt], 0, 5, None)                 # err NULL
        for vs in (1, 2, 3, 12, 16):
            assert "value_size" in _refused(lambda: clo.Bucket(ctx, "uint", vs))
            assert not lib.clo_bucket_new(None, ctx.h, 5, vs, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.Bucket(ctx, "uint", 0, ct))
            assert not lib.clo_bucket_new(None, ctx.h, 5, 0, clo.CLO_TYPES[ct], None)
        for opt in ("accumulate", "drop_rest=1", " ", "tile=4096"):
            assert "options" in _refused(lambda: clo.Bucket(ctx, "uint", options=opt)), opt
            assert not lib.clo_bucket_new(opt.encode(), ctx.h, 5, 0, 5, None)
        for kt in KEY_TYPES:                                                                          # every legal combination
            for vs in (0, 4, 8):
                for ct in COUNT_TYPES:
                    b = clo.Bucket(ctx, kt, vs, ct, options="" if vs else None)
                    assert (b.key_type, b.key_size, b.value_size, b.count_type, b.count_size) == \
                        (clo.CLO_TYPES[kt], np.dtype(NP[kt]).itemsize, vs, clo.CLO_TYPES[ct], np.dtype(COUNT_NP[ct]).itemsize)
                    b.close()

        b0, b4, b8, c0 = clo.Bucket(ctx, "uint"), clo.Bucket(ctx, "uint", 4), clo.Bucket(ctx, "uint", 8, "ulong"), clo.Bucket(ctx, "char")
        one = np.zeros(200, np.uint32)
        ki, vi = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        ko, vo = np.arange(100, 116, dtype=np.uint32), np.arange(200, 216, dtype=np.uint32)
        vo8 = np.arange(300, 316, dtype=np.uint64)
        of = np.arange(400, 409, dtype=np.uint32)
        p = lambda x: x.ctypes.data if x is not None else None

        def host(obj, k, v, k_out, v_out, off, n=16, shift=0, bins=8, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_bucket_with_host_data(obj.h, None, None, p(k), p(v), p(k_out), p(v_out), p(off), n, None, shift, bins, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel must", b0, ki, None, ko, None, of, n=1 << 32)
        both("num_bins must not be 0", b0, ki, None, ko, None, of, bins=0)
        both("65535", b0, ki, None, ko, None, of, bins=65536)
        both("65535", b0, ki, None, ko, None, of, bins=1 << 33)
        both("shift", b0, ki, None, ko, None, of, shift=32)
        both("shift", c0, ki, None, ko, None, of, shift=8)
        both("keys_in", b0, None, None, ko, None, of)
        both("keys_in", b4, None, None, None, vo, of)
        both("offsets_out", b0, ki, None, ko, None, None)
        both("offsets_out", b0, None, None, ko, None, None, n=0)                                      # even where nothing else is needed
        both("value_size 0", b0, ki, vi, ko, None, of)
        both("value_size 0", b0, ki, None, ko, vo, of)
        both("values_out", b4, ki, vi, ko, None, of)
        both("arg form", b8, ki, None, ko, vo8, of)
        both("keys_out", b0, ki, None, None, None, of)
        both("keys_out", b4, ki, vi, None, vo, of)
        both("keys_out", b8, ki, vo8, None, vo8, of)
        O = "overlap"
        both(O, b0, ki, None, ki, None, of)                                                           # in place
        both(O, b0, one[0:16], None, one[15:31], None, of)                                            # one shared element
        both(O, b0, one[8:24], None, one[0:16], None, of)
        both(O, b4, ki, one[0:16], ko, one[0:16], of)                                                 # values in place
        both(O, b4, ki, vi, one[0:16], one[15:31], of)                                                # values_out on keys_out's last row
        both(O, b8, ki, vo8, one[0:16], one[14:46].view(np.uint64), of)
        both(O, b0, ki, None, one[0:16], None, one[15:24])                                            # offsets_out on keys_out's last row
        both(O, b0, one[0:16], None, ko, None, one[15:24])                                            # ... on keys_in's
        both(O, b4, ki, one[0:16], ko, vo, one[8:17])                                                 # ... inside values_in
        both(O, b4, ki, vi, ko, one[20:36], one[12:21])                                               # its last entry (index num_bins) on values_out's first row
        assert np.array_equal(ko, np.arange(100, 116)) and np.array_equal(vo, np.arange(200, 216)) and np.array_equal(vo8, np.arange(300, 316))
        assert np.array_equal(of, np.arange(400, 409)) and not one.any() and not ki.any() and not vi.any()

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS
        for obj, args in ((b0, (one[0:16], None, one[16:32], None, one[32:41])),
                          (b4, (one[0:16], one[16:32], one[32:48], one[48:64], one[64:73])),
                          (b4, (one[0:16], None, None, one[16:32], one[32:41]))):
            err = clo.api._Err()
            assert not lib.clo_bucket_with_host_data(obj.h, None, None, *[p(x) for x in args], 16, None, 0, 8, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", e.value
        assert not one.any()
        # the Python view checks the element sizes
        with pytest.raises(ValueError):
            b0.with_host_data(np.zeros(4, np.uint64), num_bins=3)
        with pytest.raises(ValueError):
            b4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint64), num_bins=3)
        for s in (b0, b4, b8, c0):
            s.close()
    finally:
        ctx.close()


def test_no_rows_without_a_device():
    ctx = clo.Context(offline=True)
    try:
        for kt in ("char", "ulong"):
            for vs in (0, 4, 8):
                for ct in COUNT_TYPES:
                    for bins in (1, 255, 256, 65535):
                        b = clo.Bucket(ctx, kt, vs, ct)
                        ko, vo, off = b.with_host_data(np.zeros(0, NP[kt]), None if vs != 8 else np.zeros(0, np.uint64), -3 if kt == "char" else 3, 2, bins)
                        assert ko.size == 0 and (vo is None) == (vs == 0) and off.dtype == COUNT_NP[ct] and off.size == bins + 1 and not off.any()
                        # raw: bins + 1 zeros and not an entry more; the rows' arrays are not touched
                        raw, dummy = np.full(bins + 3, 7, COUNT_NP[ct]), np.full(8, 9, np.uint64)
                        err = clo.api._Err()
                        at = lambda x: x.ctypes.data
                        assert clo.api.lib.clo_bucket_with_host_data(b.h, None, None, None, at(dummy) if vs == 8 else None, at(dummy), at(dummy) if vs else None,
                                                                     at(raw), 0, None, 0, bins, err.ref)
                        err.raise_if_set()
                        assert not raw[:bins + 1].any() and (raw[bins + 1:] == 7).all() and (dummy == 9).all()
                        b.close()
    finally:
        ctx.close()


# ---- the thin ABI's status codes: the table tests/test_gpu_bucket.py asks of the device code, asked here of the stub ----

STATUS_SOURCE = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "clo_hip.h"
int main(void) {
	static uint32_t ki[16], vi[32], ko[16], vo[32];
	static uint64_t of[400];
	const size_t need = clo_hip_bucket_workspace_bytes(16, 4, 4, 300), need1 = clo_hip_bucket_workspace_bytes(16, 4, 4, 255);
	void* ws = aligned_alloc(256, need);
	char* odd = (char*) vi + 2;
#define ROW(name, call) printf("%s %d\n", name, (call))
	ROW("ok", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("ok_one_pass", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 1, 4, 8, 5, 3, 255, ws, need1, NULL));
	ROW("ok_arg_only", clo_hip_bucket(ki, NULL, NULL, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("ok_keys_8", clo_hip_bucket(of, NULL, of + 200, NULL, vo, 16, 8, 1, 0, 4, 0, 63, 3, ws, need, NULL));
	ROW("ok_empty", clo_hip_bucket(NULL, NULL, ko, NULL, of, 0, 4, 0, 0, 4, 0, 0, 7, NULL, 0, NULL));
	ROW("bins_0", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 0, ws, need, NULL));
	ROW("bins_65536", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 65536, ws, need, NULL));
	ROW("key_size", clo_hip_bucket(ki, vi, ko, vo, of, 16, 3, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("key_size_16", clo_hip_bucket(ki, vi, ko, vo, of, 4, 16, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("value_size", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 2, 4, 0, 0, 300, ws, need, NULL));
	ROW("count_size", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 2, 0, 0, 300, ws, need, NULL));
	ROW("shift", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 32, 300, ws, need, NULL));
	ROW("numel", clo_hip_bucket(ki, vi, ko, vo, of, (size_t) 1 << 32, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("offsets_null", clo_hip_bucket(ki, vi, ko, vo, NULL, 16, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("offsets_odd", clo_hip_bucket(ki, vi, ko, vo, (char*) of + 4, 16, 4, 0, 4, 8, 0, 0, 300, ws, need, NULL));
	ROW("keys_null", clo_hip_bucket(NULL, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("values_out_null", clo_hip_bucket(ki, vi, ko, NULL, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("keys_out_null", clo_hip_bucket(ki, vi, NULL, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("keys_out_null_0", clo_hip_bucket(ki, NULL, NULL, NULL, of, 16, 4, 0, 0, 4, 0, 0, 300, ws, need, NULL));
	ROW("arg_8", clo_hip_bucket(ki, NULL, ko, vo, of, 16, 4, 0, 8, 4, 0, 0, 300, ws, need, NULL));
	ROW("values_with_0", clo_hip_bucket(ki, vi, ko, NULL, of, 16, 4, 0, 0, 4, 0, 0, 300, ws, need, NULL));
	ROW("values_out_with_0", clo_hip_bucket(ki, NULL, ko, vo, of, 16, 4, 0, 0, 4, 0, 0, 300, ws, need, NULL));
	ROW("keys_odd", clo_hip_bucket((char*) ki + 2, vi, ko, vo, of, 15, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("values_odd", clo_hip_bucket(ki, odd, ko, vo, of, 15, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("keys_out_odd", clo_hip_bucket(ki, vi, (char*) ko + 2, vo, of, 15, 4, 0, 4, 4, 0, 0, 300, ws, need, NULL));
	ROW("values_out_odd", clo_hip_bucket(ki, vi, ko, (char*) vo + 4, of, 15, 4, 0, 8, 4, 0, 0, 300, ws, need, NULL));
	ROW("ws_null", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, NULL, need, NULL));
	ROW("ws_short", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need - 1, NULL));
	ROW("ws_one_pass_for_two", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, need1, NULL));
	ROW("ws_zero", clo_hip_bucket(ki, vi, ko, vo, of, 16, 4, 0, 4, 4, 0, 0, 300, ws, 0, NULL));
	ROW("tile_unbuilt", (int) (clo_hip_bucket_tile(3, 4) + clo_hip_bucket_tile(4, 2) + clo_hip_bucket_workspace_bytes(16, 3, 4, 300)));
	free(ws);
	return 0;
}
"""

# CLO_HIP_EARGS -1, CLO_HIP_EUNSUPPORTED -2, CLO_HIP_EWORKSPACE -3 (include/clo_hip.h); tests/test_gpu_bucket.py makes
# such calls on device memory and expects the same answers
STATUS_TABLE = (("ok", 0), ("ok_one_pass", 0), ("ok_arg_only", 0), ("ok_keys_8", 0), ("ok_empty", 0), ("bins_0", "EARGS"), ("bins_65536", "EARGS"),
                ("key_size", "EUNSUPPORTED"), ("key_size_16", "EUNSUPPORTED"), ("value_size", "EUNSUPPORTED"), ("count_size", "EUNSUPPORTED"),
                ("shift", "EARGS"), ("numel", "EARGS"), ("offsets_null", "EARGS"), ("offsets_odd", "EARGS"), ("keys_null", "EARGS"),
                ("values_out_null", "EARGS"), ("keys_out_null", "EARGS"), ("keys_out_null_0", "EARGS"), ("arg_8", "EARGS"), ("values_with_0", "EARGS"),
                ("values_out_with_0", "EARGS"), ("keys_odd", "EARGS"), ("values_odd", "EARGS"), ("keys_out_odd", "EARGS"), ("values_out_odd", "EARGS"),
                ("ws_null", "EARGS"), ("ws_short", "EWORKSPACE"), ("ws_one_pass_for_two", "EWORKSPACE"), ("ws_zero", "EWORKSPACE"), ("tile_unbuilt", 0))


def status_codes():
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    return {n: int(re.search(r"#define CLO_HIP_%s\s+\(?(-?\d+)\)?" % n, text).group(1)) for n in ("EARGS", "EUNSUPPORTED", "EWORKSPACE")}


def test_the_stub_answers_the_status_code_table(tmp_path):
    src = tmp_path / "status.c"
    src.write_text(STATUS_SOURCE)
    exe = str(tmp_path / "status")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-w", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), str(src), os.path.join(ROOT, "tests", "hoststub", "clo_hip_bucket_stub.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = [tuple(l.split()) for l in r.stdout.splitlines()]
    codes = status_codes()
    assert got == [(n, str(codes.get(c, c))) for n, c in STATUS_TABLE]
    # the stub's getters are the library's
    lib = clo.api.lib
    assert lib.clo_hip_bucket_workspace_bytes(16, 4, 4, 300) > lib.clo_hip_bucket_workspace_bytes(16, 4, 4, 255) > 0


def test_the_stub_and_the_library_size_the_workspace_alike(tmp_path):
    src = tmp_path / "sizes.c"
    cases = [(n, ks, vs, b) for n in (1, 4096, 4097, 1 << 20, (1 << 32) - 1) for ks, vs in ((1, 0), (4, 4), (8, 8), (2, 4)) for b in (1, 255, 256, 65535)]
    src.write_text('#include <stdio.h>\n#include "clo_hip.h"\nint main(void) {\n' +
                   "".join('printf("%%zu %%zu\\n", clo_hip_bucket_workspace_bytes(%dull, %d, %d, %d), clo_hip_bucket_tile(%d, %d));\n' % (c + c[1:3]) for c in cases) + "return 0; }\n")
    exe = str(tmp_path / "sizes")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-w", "-I" + os.path.join(ROOT, "include"), str(src),
                           os.path.join(ROOT, "tests", "hoststub", "clo_hip_bucket_stub.c"), "-o", exe])
    got = [tuple(int(x) for x in l.split()) for l in subprocess.run([exe], capture_output=True, text=True, timeout=60, check=True).stdout.splitlines()]
    lib = clo.api.lib
    assert got == [(lib.clo_hip_bucket_workspace_bytes(*c), lib.clo_hip_bucket_tile(c[1], c[2])) for c in cases]


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "bucket_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "bucket_host", "bucket_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("bucket host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(keys, values, lower, shift, num_bins):
    """The definition, over Python integers: d = key - lower, in range iff d >= 0 and (d >> shift) < num_bins; the rows
    bin by bin in input order, the rest last."""
    rows = [[] for _ in range(num_bins + 1)]
    for i, k in enumerate(keys.tolist()):
        d = int(k) - int(lower)
        rows[d >> shift if d >= 0 and (d >> shift) < num_bins else num_bins].append(i)
    perm = [i for r in rows for i in r]
    off = [0]
    for r in rows[:-1]:
        off.append(off[-1] + len(r))
    return perm, off


def test_the_model_against_a_plain_loop():
    """Every key type with keys at the type's limits and around lower; lower at the minimum, negative, zero, positive
    and near the maximum, so that lower + (num_bins << shift) lies past the type's maximum and the wrapped difference of
    a key below lower would land in range; shifts 0, small and B - 1; bin counts 1 to 65535; with and without values."""
    rng = np.random.default_rng(11)
    for kt in KEY_TYPES:
        info = np.iinfo(NP[kt])
        B = 8 * np.dtype(NP[kt]).itemsize
        edge = np.array([info.min, info.min + 1, info.max, info.max - 1, 0, 1, 5, info.max // 2, info.max // 2 + 1], dtype=NP[kt])
        for lower in sorted({info.min, info.min + 3, 0, 7, info.max - 50, info.max - 1, info.max, -5 if info.min < 0 else 5}):
            near = np.array([min(max(lower + x, info.min), info.max) for x in range(-20, 300, 7)], dtype=object).astype(NP[kt])
            keys = rng.permutation(np.concatenate((edge, near, rng.integers(info.min, info.max, 60, dtype=NP[kt], endpoint=True))))
            vals = rng.integers(0, 1 << 62, keys.size, dtype=np.uint64)
            for shift in (0, 1, 3, B - 1):
                for num_bins in (1, 2, 40, 255, 256, 65535):
                    if lower == info.max - 50 and B == 64:
                        assert lower + (num_bins << shift) > info.max or num_bins <= 50      # past the type's maximum
                    for ct in COUNT_TYPES:
                        k, v, perm, off = bucket(keys, vals, lower, shift, num_bins, ct)
                        want_perm, want_off = _loop(keys, vals, lower, shift, num_bins)
                        what = (kt, lower, shift, num_bins)
                        assert perm.dtype == np.uint32 and perm.tolist() == want_perm, what
                        assert off.dtype == COUNT_NP[ct] and off.tolist() == want_off, what
                        assert np.array_equal(k, keys[want_perm]) and np.array_equal(v, vals[want_perm]), what
                        b = bin_or_rest(keys, lower, shift, num_bins)
                        assert np.array_equal(b[perm], np.sort(b)) and off[-1] == (b < num_bins).sum(), what
    k, v, perm, off = bucket(np.zeros(0, np.int16), None, -4, 2, 9)
    assert k.size == 0 and v is None and perm.size == 0 and off.tolist() == [0] * 10


def test_the_fuzz_strata_reach_what_they_are_for():
    """What tests/test_gpu_bucket_fuzz.py runs, seen through the model alone: every value of every dimension is dealt; bin
    counts on both sides of the one-pass / two-pass border meet row counts on both sides of multiples of the tile; there
    are empty inputs, inputs with nothing in range and with nothing in the rest, empty bins, bins that take rows from
    every tile, rows below lower that the wrapped difference would put in range, and every form at both pass counts."""
    T = clo.bucket_tile(4, 0)
    ss = strata(T)
    assert len(ss) == STRATA >= 200 and SEED == 24101
    seen = {k: set() for k in ("key_type", "mode", "count_type", "num_bins", "size", "dist", "lower_kind", "shift_kind")}
    passes_by_size, forms_by_passes = set(), set()
    reach = dict(empty=0, nothing_in_range=0, nothing_in_rest=0, empty_bins=0, every_tile=0, wrapped=0, several_tiles=0, past_max=0)
    for s in ss:
        for k in seen:
            seen[k].add(s[k])
        keys, n, num_bins = s["keys"], s["n"], s["num_bins"]
        assert keys.dtype == NP[s["key_type"]] and keys.size == n <= 4 * T
        info = np.iinfo(keys.dtype)
        assert info.min <= s["lower"] <= info.max and 0 <= s["shift"] < 8 * keys.dtype.itemsize
        passes = 1 if num_bins + 1 <= 256 else 2
        passes_by_size.add((passes, s["size"]))
        forms_by_passes.add((passes, s["mode"]))
        b = bin_or_rest(keys, s["lower"], s["shift"], num_bins)
        counts = np.bincount(b, minlength=num_bins + 1)
        reach["empty"] += int(n == 0)
        reach["nothing_in_range"] += int(n > 0 and counts[num_bins] == n)
        reach["nothing_in_rest"] += int(n > 0 and counts[num_bins] == 0)
        reach["empty_bins"] += int(n > 0 and (counts[:num_bins] == 0).any() and (counts[:num_bins] > 0).any())
        reach["several_tiles"] += int(n > 2 * T)
        if n > 2 * T:
            tiles = -(-n // T)
            per = np.zeros((num_bins + 1, tiles), bool)
            per[b, np.arange(n) // T] = True
            reach["every_tile"] += int(per[:num_bins].all(axis=1).any())
        # a key below lower whose difference, wrapped to the key's width, is below num_bins << shift
        if s["lower"] + (num_bins << s["shift"]) > info.max:
            reach["past_max"] += 1
            below = [int(k) for k in keys.tolist() if int(k) < s["lower"]]
            bits = 8 * keys.dtype.itemsize
            reach["wrapped"] += int(any((((k - s["lower"]) % (1 << bits)) >> s["shift"]) < num_bins for k in below))
    assert seen == dict(key_type=set(KEY_TYPES), mode=set(MODES), count_type=set(COUNT_TYPES), num_bins=set(BIN_COUNTS), size=set(SIZES),
                        dist=set(DISTS), lower_kind=set(LOWERS), shift_kind=set(SHIFTS))
    assert {255, 256} <= set(BIN_COUNTS) and max(BIN_COUNTS) == clo.BUCKET_MAX_BINS
    assert passes_by_size == {(p, z) for p in (1, 2) for z in SIZES}, sorted(passes_by_size)
    assert forms_by_passes == {(p, m) for p in (1, 2) for m in MODES}
    assert all(v >= 1 for v in reach.values()), reach
