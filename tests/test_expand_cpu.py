"""CloExpand (include/clo_expand.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile, LDS-segment and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS
through an offline context before anything touches a device (err == NULL included) and leaves the outputs alone, m == 0
succeeds without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among
them clo_hip_expand_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/expand_host/expand_host_test.c. The reference model the GPU tests compare against (expand_model.py) is checked
here against a plain Python loop over Python integers."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from expand_model import FORMS, ends_of, expand

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_expand_new", "clo_expand_destroy", "clo_expand_with_device_data", "clo_expand_with_host_data",
          "clo_expand_get_context", "clo_expand_get_form", "clo_expand_get_value_type", "clo_expand_get_value_size",
          "clo_expand_get_count_type", "clo_expand_get_count_size")
THIN = ("clo_hip_expand", "clo_hip_expand_workspace_bytes", "clo_hip_expand_tile", "clo_hip_expand_lds_segments")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_expand.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_EXPAND_FORMS "counts, offsets"' in text
    assert ", ".join(clo.EXPAND_FORMS) == "counts, offsets" == ", ".join(FORMS)
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(FORMS):                                             # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_EXPAND_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_expand.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("Expand", "expand_tile", "expand_lds_segments"):
        assert getattr(clo, n) is not None and n in clo.__all__


def test_tile_lds_and_workspace_getters():
    for vs in (0, 1, 2, 4, 8):
        t = clo.expand_tile(vs)
        assert t >= 1024 and t % 1024 == 0, (vs, t)
    for vs in (3, 16, -1):
        assert clo.expand_tile(vs) == 0, vs
    assert clo.expand_lds_segments() > 0
    ws = clo.api.lib.clo_hip_expand_workspace_bytes
    T = clo.expand_tile(4)
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    assert ws(0, 0) == 0
    for a in sizes:
        col = [ws(a, c) for c in sizes]
        row = [ws(n, a) for n in sizes]
        assert col == sorted(col) and row == sorted(row), (a, col, row)       # monotone in both arguments
        assert all(s % 256 == 0 for s in col + row)
        for c in sizes:
            assert ws(a, c) >= 8 * a + 4 * -(-c // T), (a, c)                 # 8 bytes per segment plus 4 per tile


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for form in ("", "lengths", "Counts", "count", "offsets ", None):
            assert "form" in _refused(lambda: clo.Expand(form, ctx, "uint"))
            assert not lib.clo_expand_new(form.encode() if form is not None else None, None, ctx.h, 5, 5, None)   # err NULL
        for opt in ("tile=4096", "sorted", " "):
            assert "options" in _refused(lambda: clo.Expand("counts", ctx, "uint", options=opt))
            assert not lib.clo_expand_new(b"counts", opt.encode(), ctx.h, 5, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.Expand("counts", ctx, "uint", count_type=ct))
            assert not lib.clo_expand_new(b"offsets", None, ctx.h, 5, clo.CLO_TYPES[ct], None)
        for vt in (-1, 11, 100):
            assert "value_type" in _refused(lambda: clo.Expand("counts", ctx, vt))
            assert not lib.clo_expand_new(b"counts", None, ctx.h, vt, 5, None)
        for form in FORMS:                                                    # every form, value type, count type, both spellings of no options
            for vt, code in clo.CLO_TYPES.items():
                for ct, opt in (("uint", None), ("ulong", "")):
                    e = clo.Expand(form, ctx, vt, ct, options=opt)
                    assert (e.form, e.value_type, e.value_size, e.count_type, e.count_size) == \
                        (form, code, np.dtype(clo.api.CLO_TYPE_NP[vt]).itemsize, clo.CLO_TYPES[ct], 4 if ct == "uint" else 8)
                    e.close()

        c4, o4, c8 = clo.Expand("counts", ctx, "uint"), clo.Expand("offsets", ctx, "float"), clo.Expand("counts", ctx, "double", "ulong")
        cn, of = np.zeros(16, np.uint32), np.zeros(17, np.uint32)
        cn8 = np.zeros(16, np.uint64)
        vi, vi8 = np.zeros(16, np.uint32), np.zeros(16, np.uint64)
        vo, so, ro = (np.arange(b, b + 16, dtype=np.uint32) for b in (100, 200, 300))
        vo8 = np.arange(400, 416, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 16, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, vals, out_v, out_s, out_r, n=16, cap=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_expand_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_v), p(out_s), p(out_r), sp(out_n), n, cap,
                                               err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_in", c4, cn, None, None, None, so, None, n=1 << 32)
        both("numel_in", o4, of, nin, vi, vo, so, ro, n=(1 << 32) + 5)
        both("capacity", c4, cn, None, None, None, so, None, cap=1 << 32)
        both("capacity", c8, cn8, None, vi8, vo8, None, None, cap=1 << 63)
        both("the counts", c4, None, None, None, None, so, None)             # NULL counts_or_offsets
        both("the offsets", o4, None, None, None, None, so, None)
        both("the offsets", o4, None, None, None, None, so, None, n=0, cap=1)   # ... with numel_in 0 too where rows are asked for
        both("all NULL", c4, cn, None, None, None, None, None)
        both("all NULL", o4, of, nin, None, None, None, None)
        both("without values_out", c4, cn, None, vi, None, so, None)         # exactly one of values_in / values_out
        both("without values_in", c4, cn, None, None, vo, so, None)
        both("without values_in", c8, cn8, None, None, vo8, None, None)
        both("num_out", c4, cn, None, None, None, so, None, out_n=None)
        both("num_out", o4, of, nin, vi, vo, so, ro, out_n=None)

        # overlap: an output (sized by capacity rows, not by total: every count is 0) on, inside, across the end of,
        # sharing one element with an input or num_in, outputs on each other, num_out on each array
        one = np.zeros(160, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, None, None, cn, None)                                           # seg_out on the counts
        both(O, c4, one[0:32], None, None, None, one[8:24], None, n=32)                       # seg_out inside the counts
        both(O, c4, one[0:16], None, None, None, one[8:24], None)                             # seg_out across the counts' end
        both(O, c4, one[0:16], None, None, None, one[15:31], None)                            # one shared element
        both(O, o4, one[0:17], None, None, None, None, one[16:32])                            # rank_out on the 17th offset
        both(O, c4, cn, n8(40, 42), None, None, one[41:57], None)                             # seg_out on num_in's second half
        both(O, c4, cn, None, one[0:16], one[15:31], so, None)                                # values_out on values_in's last row
        both(O, c8, cn8, None, vi8, one[0:32].view(np.uint64), one[31:47], None)              # seg_out on values_out's last row (8-byte rows)
        both(O, c4, cn, None, None, None, one[0:16], one[15:31])                              # seg_out and rank_out share a row
        both(O, c4, cn, None, None, None, one[0:16], one[0:16])                               # ... lie on each other
        both(O, c4, cn, None, vi, one[0:16], None, one[8:24])                                 # values_out and rank_out
        both(O, c4, cn, None, None, None, one[0:16], None, out_n=n8(14, 16))                  # num_out on seg_out's last rows
        both(O, c4, cn, None, None, None, None, one[0:16], out_n=n8(0, 2))                    # num_out on rank_out's first
        both(O, c4, cn, None, vi, one[0:16], so, None, out_n=n8(6, 8))                        # num_out inside values_out
        both(O, c4, one[0:16], None, None, None, so, None, out_n=n8(14, 16))                  # num_out on the counts
        both(O, c4, cn, None, one[0:16], vo, so, None, out_n=n8(2, 4))                        # num_out on values_in
        both(O, c4, cn, n8(20, 22), None, None, so, None, out_n=n8(20, 22))                   # num_out on num_in
        assert np.array_equal(vo, np.arange(100, 116)) and np.array_equal(so, np.arange(200, 216)) and np.array_equal(ro, np.arange(300, 316))
        assert np.array_equal(vo8, np.arange(400, 416)) and not one.any() and not cn.any() and not of.any() and (num == 777).all() and nin[0] == 16

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS (the counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(150, 152)
        for obj, args in ((c4, (one[0:16], None, None, None, one[16:32], None)),
                          (c4, (one[0:16], n8(16, 18), one[18:34], one[34:50], one[50:66], one[66:82])),
                          (o4, (one[0:17], None, None, None, one[17:33], one[33:49])),
                          (o4, (one[0:17], n8(18, 20), one[20:36], one[36:52], None, None))):
            err = clo.api._Err()
            src, n_in, vals, out_v, out_s, out_r = args
            assert not lib.clo_expand_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_v), p(out_s), p(out_r), sp(out_n), 16, 16, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:150] == 1).all()

        # the Python view checks the element types
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint64), 8)
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), 8, values=np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), 8, values=np.zeros(5, np.uint32))
        with pytest.raises(ValueError):
            o4.with_host_data(np.zeros(0, np.uint32), 8)
        for e in (c4, o4, c8):
            e.close()
    finally:
        ctx.close()


def test_no_segments_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for form in FORMS:
            for ct, cdt in (("uint", np.uint32), ("ulong", np.uint64)):
                e = clo.Expand(form, ctx, "float", ct)
                src = np.zeros(1 if form == "offsets" else 0, cdt)
                v, s, r, total = e.with_host_data(src, 5, values=np.zeros(0, np.float32), rank=True)
                assert total == 0 and v.size == 0 and v.dtype == np.float32 and s.size == 0 and r.size == 0
                src = np.arange(1, 6, dtype=cdt)                              # four or five segments, of which num_in takes none
                v, s, r, total = e.with_host_data(src, 5, num_in=0)
                assert total == 0 and v is None and s.size == 0 and r is None
                # raw: num_out becomes 0, outputs that exist are not touched, the inputs of numel_in 0 may be NULL
                out_v, out_s, num = np.full(4, 7, np.float32), np.full(4, 9, np.uint32), C.c_size_t(55)
                vals = np.zeros(1, np.float32)
                err = clo.api._Err()
                assert lib.clo_expand_with_host_data(e.h, None, None, src.ctypes.data if form == "offsets" else None, None, vals.ctypes.data,
                                                     out_v.ctypes.data, out_s.ctypes.data, None, C.byref(num), 0, 4, err.ref)
                err.raise_if_set()
                assert num.value == 0 and (out_v == 7).all() and (out_s == 9).all()
                e.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "expand_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "expand_host", "expand_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("expand host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(form, src, capacity, num_in=None):
    """The definition, over Python integers: segment r owns c_r consecutive rows."""
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    seg, rank = [], []
    for r in range(m):
        for k in range(counts[r]):
            seg.append(r)
            rank.append(k)
    return seg[:capacity], rank[:capacity], len(seg)


def test_the_model_against_a_plain_loop():
    """Counts with zeros at the start, in the middle and at the end, consecutive zeros, all ones, a single segment; both
    forms (the offsets with a base that is not 0), num_in below, equal to and above numel_in, capacities around total."""
    cases = ([0, 0, 3, 1, 0, 2, 0, 0, 0, 5, 1, 0], [0, 4], [4, 0], [0, 0, 0], [1] * 9, [7], [0], [], [2, 0, 0, 0, 0, 3], [1, 0, 1, 0, 1, 0])
    for counts in cases:
        for form in FORMS:
            for cdt in (np.uint32, np.uint64):
                src = np.array(counts, cdt) if form == "counts" else (np.concatenate(([0], np.cumsum(counts))) + 12345).astype(cdt)
                for num_in in (None, 0, len(counts) // 2, len(counts), len(counts) + 3):
                    total = _loop(form, src, 1 << 30, num_in)[2]
                    for cap in sorted({0, 1, max(total - 1, 0), total, total + 4}):
                        seg, rank, t = expand(form, src, cap, num_in)
                        what = (counts, form, num_in, cap)
                        assert seg.dtype == np.uint32 and rank.dtype == np.uint32, what
                        assert (seg.tolist(), rank.tolist(), t) == _loop(form, src, cap, num_in), what
    ends, m = ends_of("counts", np.array([1 << 63, 1 << 63, 5], np.uint64))   # the sums are taken modulo 2^64
    assert m == 3 and ends.tolist() == [1 << 63, 0, 5]
