"""CloSegReduce (include/clo_segreduce.h) on the CPU: the library exports the new public and thin-ABI entry points and
the headers declare them, the tile and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs alone, m == 0 succeeds
without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among them
clo_hip_segreduce_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/segreduce_host/segreduce_host_test.c. The reference model the GPU tests compare against (segreduce_model.py) is
checked here against a plain Python loop over Python integers."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from segreduce_model import FORMS, NP, OPS, PAIRS, identity, segreduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_segreduce_new", "clo_segreduce_destroy", "clo_segreduce_with_device_data", "clo_segreduce_with_host_data",
          "clo_segreduce_get_context", "clo_segreduce_get_op", "clo_segreduce_get_form", "clo_segreduce_get_value_type",
          "clo_segreduce_get_value_size", "clo_segreduce_get_sum_type", "clo_segreduce_get_sum_size",
          "clo_segreduce_get_count_type", "clo_segreduce_get_count_size")
THIN = ("clo_hip_segreduce", "clo_hip_segreduce_workspace_bytes", "clo_hip_segreduce_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_segreduce.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SEGREDUCE_FORMS "counts, offsets"' in text
    assert ", ".join(clo.SEGREDUCE_FORMS) == "counts, offsets" == ", ".join(FORMS)
    assert clo.SEGREDUCE_OPS == ("sum", "min", "max") == OPS
    assert '#define CLO_REDUCE_BY_KEY_OPS "%s"' % ", ".join(OPS) in open(os.path.join(ROOT, "include", "clo_reduce.h")).read()
    for word in ("arg-min", "floating point", "several value columns", "numel >= 2^32"):   # what the header says is out of scope
        assert word in text, word
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(FORMS):                                             # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_SEGREDUCE_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_segreduce.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("SegReduce", "segreduce_tile", "SEGREDUCE_OPS"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert "segmented-reduction" in clo.__doc__


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    import re
    text = open(os.path.join(ROOT, "cl_ops_amd", "csrc", "clo_segreduce.c")).read()
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text


def test_tile_and_workspace_getters():
    for vs, ss in ((4, 4), (4, 8), (8, 8)):
        t = clo.segreduce_tile(vs, ss)
        assert t >= 1024 and t % 256 == 0, (vs, ss, t)
    assert clo.segreduce_tile(4) == clo.segreduce_tile(4, 4)
    for vs, ss in ((8, 4), (2, 4), (4, 2), (0, 4), (4, 0), (16, 16), (-1, 4)):
        assert clo.segreduce_tile(vs, ss) == 0, (vs, ss)
    ws = clo.api.lib.clo_hip_segreduce_workspace_bytes
    T = clo.segreduce_tile(4, 4)
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    assert ws(0, 0) == 0
    for a in sizes:
        col = [ws(a, c) for c in sizes]
        row = [ws(n, a) for n in sizes]
        assert col == sorted(col) and row == sorted(row), (a, col, row)       # monotone in both arguments
        assert all(s % 256 == 0 for s in col + row)
        for c in sizes:
            assert ws(a, c) >= 8 * a + 20 * -(-(a + c) // T), (a, c)          # 8 bytes per segment plus 20 per tile of merge steps


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for op in ("", "mean", "Sum", "sum ", "argmin", None):
            assert "reduction" in _refused(lambda: clo.SegReduce(op, "counts", ctx))
            assert not lib.clo_segreduce_new(op.encode() if op is not None else None, b"counts", None, ctx.h, 5, 5, 5, None)   # err NULL
        for form in ("", "lengths", "Counts", "count", "offsets ", None):
            assert "form" in _refused(lambda: clo.SegReduce("sum", form, ctx))
            assert not lib.clo_segreduce_new(b"sum", form.encode() if form is not None else None, None, ctx.h, 5, 5, 5, None)
        for opt in ("tile=4096", "sorted", " "):
            assert "options" in _refused(lambda: clo.SegReduce("sum", "counts", ctx, options=opt))
            assert not lib.clo_segreduce_new(b"sum", b"counts", opt.encode(), ctx.h, 5, 5, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.SegReduce("sum", "counts", ctx, count_type=ct))
            assert not lib.clo_segreduce_new(b"sum", b"offsets", None, ctx.h, 5, 5, clo.CLO_TYPES[ct], None)
        for vt in ("char", "uchar", "short", "ushort", "half", "float", "double"):   # neither as the value nor as the sum type
            assert "int, uint, long or ulong" in _refused(lambda: clo.SegReduce("sum", "counts", ctx, vt, "ulong"))
            assert "int, uint, long or ulong" in _refused(lambda: clo.SegReduce("max", "offsets", ctx, "uint", vt))
            assert not lib.clo_segreduce_new(b"sum", b"counts", None, ctx.h, clo.CLO_TYPES[vt], 7, 5, None)
        for vt, st in (("long", "int"), ("long", "uint"), ("ulong", "int"), ("ulong", "uint")):
            assert "narrower" in _refused(lambda: clo.SegReduce("min", "counts", ctx, vt, st))
            assert not lib.clo_segreduce_new(b"min", b"counts", None, ctx.h, clo.CLO_TYPES[vt], clo.CLO_TYPES[st], 5, None)
        for op in OPS:                                                        # every op, form, legal type pair, count type, both spellings of no options
            for form in FORMS:
                for vt, st in PAIRS:
                    for ct, opt in (("uint", None), ("ulong", "")):
                        s = clo.SegReduce(op, form, ctx, vt, st, ct, options=opt)
                        assert (s.op, s.form, s.value_type, s.value_size, s.sum_type, s.sum_size, s.count_type, s.count_size) == \
                            (op, form, clo.CLO_TYPES[vt], np.dtype(NP[vt]).itemsize, clo.CLO_TYPES[st], np.dtype(NP[st]).itemsize,
                             clo.CLO_TYPES[ct], 4 if ct == "uint" else 8)
                        s.close()
        assert len(PAIRS) == 12
        s = clo.SegReduce("sum", "counts", ctx, "long")                       # sum_type None: the value type
        assert s.sum_type == clo.CLO_TYPES["long"]
        s.close()

        c4, o4, c8 = clo.SegReduce("sum", "counts", ctx), clo.SegReduce("min", "offsets", ctx, "int"), clo.SegReduce("max", "counts", ctx, "int", "long", "ulong")
        cn, of = np.zeros(16, np.uint32), np.zeros(17, np.uint32)
        cn8 = np.zeros(16, np.uint64)
        vi = np.zeros(16, np.uint32)
        ao = np.arange(100, 116, dtype=np.uint32)
        ao8 = np.arange(400, 416, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 16, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, vals, out_a, m_h=16, n=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_segreduce_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_a), sp(out_n), m_h, n, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_seg", c4, cn, None, vi, ao, m_h=1 << 32)
        both("numel_seg", o4, of, nin, vi, ao, m_h=(1 << 32) + 5)
        both("numel must", c4, cn, None, vi, ao, n=1 << 32)
        both("numel must", c8, cn8, None, vi, ao8, n=1 << 63)
        both("the counts", c4, None, None, vi, ao)                            # NULL counts_or_offsets
        both("the offsets", o4, None, None, vi, ao)
        both("the offsets", o4, None, None, None, None, m_h=0, n=0)           # ... in the offsets form always
        both("values_in", c4, cn, None, None, ao)
        both("values_in", c4, None, None, None, None, m_h=0, n=3)             # ... even without a segment
        both("aggr_out", c4, cn, None, vi, None)
        both("aggr_out", c8, cn8, nin, vi, None, n=0)
        both("num_out", c4, cn, None, vi, ao, out_n=None)
        both("num_out", o4, of, nin, vi, ao, out_n=None)

        # overlap: aggr_out (sized by numel_seg rows) on, inside, across the end of, sharing one element with an input or
        # num_in; num_out on each array and on num_in
        one = np.zeros(160, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, vi, cn)                                                         # aggr_out on the counts
        both(O, c4, one[0:32], None, vi, one[8:24], m_h=32)                                   # aggr_out inside the counts
        both(O, c4, one[0:16], None, vi, one[8:24])                                           # aggr_out across the counts' end
        both(O, c4, one[0:16], None, vi, one[15:31])                                          # one shared element
        both(O, o4, one[0:17], None, vi, one[16:32])                                          # aggr_out on the 17th offset
        both(O, c4, cn, n8(40, 42), vi, one[41:57])                                           # aggr_out on num_in's second half
        both(O, c4, cn, None, one[0:16], one[15:31])                                          # aggr_out on values_in's last row
        both(O, c4, cn, None, one[0:64], one[63:79], n=64)                                    # ... sized by numel, not numel_seg
        both(O, c4, cn, None, one[0:16], one[0:16])                                           # aggr_out on values_in
        both(O, c8, cn8, None, vi, one[0:32].view(np.uint64), out_n=n8(30, 32))               # num_out on aggr_out's last row (8-byte rows)
        both(O, c4, cn, None, vi, one[0:16], out_n=n8(0, 2))                                  # num_out on aggr_out's first rows
        both(O, c4, one[0:16], None, vi, ao, out_n=n8(14, 16))                                # num_out on the counts
        both(O, c4, cn, None, one[0:16], ao, out_n=n8(2, 4))                                  # num_out on values_in
        both(O, c4, cn, n8(20, 22), vi, ao, out_n=n8(20, 22))                                 # num_out on num_in
        assert np.array_equal(ao, np.arange(100, 116)) and np.array_equal(ao8, np.arange(400, 416))
        assert not one.any() and not cn.any() and not of.any() and not vi.any() and (num == 777).all() and nin[0] == 16

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS (the counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(150, 152)
        for obj, args in ((c4, (one[0:16], None, one[16:32], one[32:48])),
                          (c4, (one[0:16], n8(16, 18), one[18:34], one[34:50])),
                          (o4, (one[0:17], None, one[17:33], one[33:49])),
                          (o4, (one[0:17], n8(18, 20), one[20:36], one[36:52]))):
            err = clo.api._Err()
            src, n_in, vals, out_a = args
            assert not lib.clo_segreduce_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_a), sp(out_n), 16, 16, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:150] == 1).all()

        # the Python view checks the element types
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint64), np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.int32))
        with pytest.raises(ValueError):
            o4.with_host_data(np.zeros(0, np.uint32), np.zeros(4, np.int32))
        for s in (c4, o4, c8):
            s.close()
    finally:
        ctx.close()


def test_no_segments_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for op in OPS:
            for form in FORMS:
                for ct, cdt in (("uint", np.uint32), ("ulong", np.uint64)):
                    s = clo.SegReduce(op, form, ctx, "int", "long", ct)
                    src = np.zeros(1 if form == "offsets" else 0, cdt)
                    a, total = s.with_host_data(src, np.arange(5, dtype=np.int32))     # rows, but no segment to put them in
                    assert total == 0 and a.size == 0 and a.dtype == np.int64
                    a, total = s.with_host_data(src, np.zeros(0, np.int32))
                    assert total == 0 and a.size == 0
                    src = np.arange(1, 6, dtype=cdt)                              # four or five segments, of which num_in takes none
                    a, total = s.with_host_data(src, np.arange(20, dtype=np.int32), num_in=0)
                    assert total == 0 and a.size == 0
                    # raw: num_out becomes 0, aggr_out is not touched
                    out_a, num = np.full(5, 7, np.int64), C.c_size_t(55)
                    zero = C.c_size_t(0)
                    vals = np.zeros(20, np.int32)
                    err = clo.api._Err()
                    assert lib.clo_segreduce_with_host_data(s.h, None, None, src.ctypes.data, C.byref(zero), vals.ctypes.data,
                                                            out_a.ctypes.data, C.byref(num), 4, 20, err.ref)
                    err.raise_if_set()
                    assert num.value == 0 and (out_a == 7).all()
                    s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segreduce_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "segreduce_host", "segreduce_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("segreduce host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(op, form, src, values, vt, st, num_in=None):
    """The definition, over Python integers: the C cast, then op over the rows the segment owns that exist."""
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    bits, signed = 8 * np.dtype(NP[st]).itemsize, np.dtype(NP[st]).kind == "i"
    wrap = lambda x: ((x + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1)) if signed else x % (1 << bits)
    vals = [wrap(int(x)) for x in values]                                     # int(x) of a numpy integer keeps its sign: C's cast
    out, at = [], 0
    for r in range(m):
        rows = [vals[i] for i in range(at, at + counts[r]) if i < len(vals)]
        at += counts[r]
        out.append(wrap(sum(rows)) if op == "sum" else int(identity(op, st)) if not rows else min(rows) if op == "min" else max(rows))
    return out, at


def test_the_model_against_a_plain_loop():
    """Counts with zeros at the start, in the middle and at the end, consecutive zeros, all ones, a single segment; both
    forms (the offsets with a base that is not 0), num_in below, equal to and above numel_seg, row counts around total
    (segments cut in the middle, segments beyond the rows), every type pair with values at the types' extremes."""
    cases = ([0, 0, 3, 1, 0, 2, 0, 0, 0, 5, 1, 0], [0, 4], [4, 0], [0, 0, 0], [1] * 9, [7], [0], [], [2, 0, 0, 0, 0, 3], [1, 0, 1, 0, 1, 0])
    rng = np.random.default_rng(7)
    for counts in cases:
        for form in FORMS:
            for cdt in (np.uint32, np.uint64):
                src = np.array(counts, cdt) if form == "counts" else (np.concatenate(([0], np.cumsum(counts))) + 12345).astype(cdt)
                for num_in in (None, 0, len(counts) // 2, len(counts), len(counts) + 3):
                    total = sum(counts[:num_in])
                    for n in sorted({0, 1, max(total - 1, 0), total, total + 4, sum(counts) // 2}):
                        for vt, st in PAIRS:
                            info = np.iinfo(NP[vt])
                            v = rng.choice(np.array([info.min, info.max, info.min + 1, info.max - 1, 0, 1, 5], dtype=NP[vt]), n)
                            for op in OPS:
                                a, t = segreduce(op, form, src, v, st, num_in)
                                what = (counts, form, num_in, n, vt, st, op)
                                assert a.dtype == NP[st], what
                                assert (a.tolist(), t) == _loop(op, form, src, v, vt, st, num_in), what
    a, t = segreduce("sum", "counts", np.array([1 << 63, 1 << 63, 5], np.uint64), np.arange(4, dtype=np.uint32), "uint")   # ends modulo 2^64
    assert t == 5 and a.size == 3                                             # (the ends do not ascend: the rows' contents are unspecified)
