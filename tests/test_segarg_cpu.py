"""CloSegArg (include/clo_segarg.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile, carry-trip and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS
through an offline context before anything touches a device (err == NULL included) and leaves the outputs alone, m == 0
succeeds without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among
them clo_hip_segarg_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/segarg_host/segarg_host_test.c. The reference model the GPU tests compare against (segarg_model.py) is checked here
against a plain Python loop over Python integers and struct-unpacked floats."""
import ctypes as C
import glob
import math
import os
import struct
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from segarg_model import FORMS, NONE, NP, OPS, TIES, none_value, segarg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_segarg_new", "clo_segarg_destroy", "clo_segarg_with_device_data", "clo_segarg_with_host_data",
          "clo_segarg_get_context", "clo_segarg_get_op", "clo_segarg_get_tie", "clo_segarg_get_form", "clo_segarg_get_value_type",
          "clo_segarg_get_value_size", "clo_segarg_get_count_type", "clo_segarg_get_count_size")
THIN = ("clo_hip_segarg", "clo_hip_segarg_workspace_bytes", "clo_hip_segarg_tile", "clo_hip_segarg_carry_tiles")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_segarg.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SEGARG_OPS  "argmin, argmax"' in text and '#define CLO_SEGARG_TIES "first, last"' in text
    assert "#define CLO_SEGARG_NONE 0xffffffffu" in text
    assert clo.SEGARG_OPS == ("argmin", "argmax") == OPS and clo.SEGARG_TIES == ("first", "last") == TIES
    assert clo.SEGARG_NONE == NONE == 0xffffffff
    assert FORMS == clo.SEGREDUCE_FORMS                                       # the forms are CloSegReduce's
    for word in ("half", "get_key", "several value columns", "segment-relative index", "k smallest per segment", "numel >= 2^32"):
        assert word in text[text.index("Out of scope"):], word                # what the header says is out of scope
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for names in (OPS, TIES, FORMS):                                          # the thin ABI's numbers are the names' positions
        for i, n in enumerate(names):
            assert "#define CLO_HIP_SEGARG_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_segarg.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("SegArg", "segarg_tile", "SEGARG_OPS", "SEGARG_TIES"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert "segmented-arg-min-max" in clo.__doc__


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    import re
    text = open(os.path.join(ROOT, "cl_ops_amd", "csrc", "clo_segarg.c")).read()
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text


def test_tile_and_workspace_getters():
    for vs in (4, 8):
        t = clo.segarg_tile(vs)
        assert t >= 1024 and t % 256 == 0, (vs, t)
    assert clo.segarg_tile() == clo.segarg_tile(4)
    for vs in (0, 1, 2, 3, 5, 12, 16, -1, -4):
        assert clo.segarg_tile(vs) == 0, vs
    assert clo.segarg_carry_tiles() >= 256 and clo.segarg_carry_tiles() % 256 == 0
    ws = clo.api.lib.clo_hip_segarg_workspace_bytes
    T = clo.segarg_tile(4)
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    assert ws(0, 0) == 0
    for a in sizes:
        col = [ws(a, c) for c in sizes]
        row = [ws(n, a) for n in sizes]
        assert col == sorted(col) and row == sorted(row), (a, col, row)       # monotone in both arguments
        assert all(s % 256 == 0 for s in col + row)
        for c in sizes:
            # 8 bytes per segment (the ends) plus, per tile of merge steps, a split, four words and two 64-bit words
            assert ws(a, c) >= 8 * a + 36 * -(-(a + c) // T), (a, c)


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for op in ("", "min", "Argmin", "argmin ", "arg", "sum", None):
            assert "arg operation" in _refused(lambda: clo.SegArg(op, "first", "counts", ctx))
            assert not lib.clo_segarg_new(op.encode() if op is not None else None, b"first", b"counts", None, ctx.h, 5, 5, None)   # err NULL
        for tie in ("", "any", "First", "last ", "middle", None):
            assert "tie" in _refused(lambda: clo.SegArg("argmin", tie, "counts", ctx))
            assert not lib.clo_segarg_new(b"argmin", tie.encode() if tie is not None else None, b"counts", None, ctx.h, 5, 5, None)
        for form in ("", "lengths", "Counts", "count", "offsets ", None):
            assert "form" in _refused(lambda: clo.SegArg("argmin", "first", form, ctx))
            assert not lib.clo_segarg_new(b"argmin", b"first", form.encode() if form is not None else None, None, ctx.h, 5, 5, None)
        for opt in ("tile=4096", "sorted", " "):
            assert "options" in _refused(lambda: clo.SegArg("argmin", "first", "counts", ctx, options=opt))
            assert not lib.clo_segarg_new(b"argmin", b"first", b"counts", opt.encode(), ctx.h, 5, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.SegArg("argmin", "first", "counts", ctx, count_type=ct))
            assert not lib.clo_segarg_new(b"argmax", b"last", b"offsets", None, ctx.h, 5, clo.CLO_TYPES[ct], None)
        for vt in ("char", "uchar", "short", "ushort", "half"):
            assert "int, uint, long, ulong, float or double" in _refused(lambda: clo.SegArg("argmax", "last", "offsets", ctx, vt))
            assert not lib.clo_segarg_new(b"argmin", b"first", b"counts", None, ctx.h, clo.CLO_TYPES[vt], 5, None)
        assert not lib.clo_segarg_new(b"argmin", b"first", b"counts", None, ctx.h, 11, 5, None)          # no such type
        assert not lib.clo_segarg_new(b"argmin", b"first", b"counts", None, None, 5, 5, None)            # no context
        for op in OPS:                                                        # every op, tie, form, value type, count type, both spellings of no options
            for tie in TIES:
                for form in FORMS:
                    for vt in NP:
                        for ct, opt in (("uint", None), ("ulong", "")):
                            s = clo.SegArg(op, tie, form, ctx, vt, ct, options=opt)
                            assert (s.op, s.tie, s.form, s.value_type, s.value_size, s.count_type, s.count_size) == \
                                (op, tie, form, clo.CLO_TYPES[vt], np.dtype(NP[vt]).itemsize, clo.CLO_TYPES[ct], 4 if ct == "uint" else 8)
                            s.close()
        assert len(NP) == 6

        c4, o4 = clo.SegArg("argmin", "first", "counts", ctx), clo.SegArg("argmax", "last", "offsets", ctx, "float")
        c8 = clo.SegArg("argmax", "first", "counts", ctx, "double", "ulong")
        cn, of = np.zeros(16, np.uint32), np.zeros(17, np.uint32)
        cn8 = np.zeros(16, np.uint64)
        vi = np.zeros(16, np.uint32)
        vi8 = np.zeros(16, np.uint64)
        io = np.arange(100, 116, dtype=np.uint32)
        vo = np.arange(200, 216, dtype=np.uint32)
        vo8 = np.arange(400, 416, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 16, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, vals, out_i, out_v, m_h=16, n=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_segarg_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_i), p(out_v), sp(out_n), m_h, n, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_seg", c4, cn, None, vi, io, vo, m_h=1 << 32)
        both("numel_seg", o4, of, nin, vi, io, None, m_h=(1 << 32) + 5)
        both("numel must", c4, cn, None, vi, io, vo, n=1 << 32)
        both("numel must", c8, cn8, None, vi8, io, vo8, n=1 << 63)
        both("the counts", c4, None, None, vi, io, vo)                        # NULL counts_or_offsets
        both("the offsets", o4, None, None, vi, io, vo)
        both("the offsets", o4, None, None, None, None, None, m_h=0, n=0)     # ... in the offsets form always
        both("values_in", c4, cn, None, None, io, vo)
        both("values_in", c4, None, None, None, None, None, m_h=0, n=3)       # ... even without a segment
        both("idx_out", c4, cn, None, vi, None, vo)
        both("idx_out", c8, cn8, nin, vi8, None, None, n=0)                   # ... val_out or not
        both("num_out", c4, cn, None, vi, io, vo, out_n=None)
        both("num_out", o4, of, nin, vi, io, None, out_n=None)

        # overlap: idx_out and val_out (sized by numel_seg rows) on, inside, across the end of, sharing one element with
        # an input, num_in or each other; num_out on each array and on num_in
        one = np.zeros(200, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, vi, cn, vo)                                                     # idx_out on the counts
        both(O, c4, cn, None, vi, io, cn)                                                     # val_out on the counts
        both(O, c4, one[0:32], None, vi, one[8:24], vo, m_h=32)                               # idx_out inside the counts
        both(O, c4, one[0:16], None, vi, io, one[8:24])                                       # val_out across the counts' end
        both(O, c4, one[0:16], None, vi, one[15:31], vo)                                      # one shared element
        both(O, o4, one[0:17], None, vi, io, one[16:32])                                      # val_out on the 17th offset
        both(O, c4, cn, n8(40, 42), vi, one[41:57], vo)                                       # idx_out on num_in's second half
        both(O, c4, cn, n8(40, 42), vi, io, one[25:41])                                       # val_out on num_in's first half
        both(O, c4, cn, None, one[0:16], one[15:31], vo)                                      # idx_out on values_in's last row
        both(O, c4, cn, None, one[0:64], io, one[63:79], n=64)                                # ... sized by numel, not numel_seg
        both(O, c4, cn, None, one[0:16], one[0:16], vo)                                       # idx_out on values_in
        both(O, c4, cn, None, vi, one[0:16], one[0:16])                                       # val_out on idx_out
        both(O, c4, cn, None, vi, one[0:16], one[15:31])                                      # ... on its last row
        both(O, c8, cn8, None, vi8, one[0:16], n8(14, 46))                                    # 8-byte rows on idx_out's last two rows
        both(O, c8, cn8, None, vi8, io, n8(0, 32), out_n=n8(30, 32))                          # num_out on val_out's last row (8-byte rows)
        both(O, c4, cn, None, vi, one[0:16], vo, out_n=n8(0, 2))                              # num_out on idx_out's first rows
        both(O, c4, cn, None, vi, io, one[0:16], out_n=n8(14, 16))                            # num_out on val_out's last rows
        both(O, c4, one[0:16], None, vi, io, vo, out_n=n8(14, 16))                            # num_out on the counts
        both(O, c4, cn, None, one[0:16], io, vo, out_n=n8(2, 4))                              # num_out on values_in
        both(O, c4, cn, n8(20, 22), vi, io, vo, out_n=n8(20, 22))                             # num_out on num_in
        assert np.array_equal(io, np.arange(100, 116)) and np.array_equal(vo, np.arange(200, 216)) and np.array_equal(vo8, np.arange(400, 416))
        assert not one.any() and not cn.any() and not of.any() and not vi.any() and (num == 777).all() and nin[0] == 16

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS (the counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(190, 192)
        for obj, args in ((c4, (one[0:16], None, one[16:32], one[32:48], one[48:64])),
                          (c4, (one[0:16], n8(16, 18), one[18:34], one[34:50], None)),
                          (o4, (one[0:17], None, one[17:33], one[33:49], one[49:65])),
                          (o4, (one[0:17], n8(18, 20), one[20:36], one[36:52], one[52:68]))):
            err = clo.api._Err()
            src, n_in, vals, out_i, out_v = args
            assert not lib.clo_segarg_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_i), p(out_v), sp(out_n), 16, 16, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:190] == 1).all()

        # the Python view checks the element types
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint64), np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.float32))
        with pytest.raises(ValueError):
            o4.with_host_data(np.zeros(0, np.uint32), np.zeros(4, np.float32))
        for s in (c4, o4, c8):
            s.close()
    finally:
        ctx.close()


def test_no_segments_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for op in OPS:
            for tie in TIES:
                for form in FORMS:
                    for ct, cdt in (("uint", np.uint32), ("ulong", np.uint64)):
                        s = clo.SegArg(op, tie, form, ctx, "float", ct)
                        src = np.zeros(1 if form == "offsets" else 0, cdt)
                        i, v, total = s.with_host_data(src, np.arange(5, dtype=np.float32))   # rows, but no segment to put them in
                        assert total == 0 and i.size == 0 and i.dtype == np.uint32 and v.size == 0 and v.dtype == np.float32
                        i, v, total = s.with_host_data(src, np.zeros(0, np.float32), want_values=False)
                        assert total == 0 and i.size == 0 and v is None
                        src = np.arange(1, 6, dtype=cdt)                          # four or five segments, of which num_in takes none
                        i, v, total = s.with_host_data(src, np.arange(20, dtype=np.float32), num_in=0)
                        assert total == 0 and i.size == 0 and v.size == 0
                        # raw: num_out becomes 0, idx_out and val_out are not touched
                        out_i, out_v, num = np.full(5, 7, np.uint32), np.full(5, 9, np.float32), C.c_size_t(55)
                        zero = C.c_size_t(0)
                        vals = np.zeros(20, np.float32)
                        err = clo.api._Err()
                        assert lib.clo_segarg_with_host_data(s.h, None, None, src.ctypes.data, C.byref(zero), vals.ctypes.data,
                                                             out_i.ctypes.data, out_v.ctypes.data, C.byref(num), 4, 20, err.ref)
                        err.raise_if_set()
                        assert num.value == 0 and (out_i == 7).all() and (out_v == 9).all()
                        s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segarg_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "segarg_host", "segarg_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("segarg host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _rank(bits, vt):
    """Where the value with these bits stands in the order, as something Python compares: the integer itself, or for a
    float (class, number, payload): negative NaNs first, the larger payload the earlier; then the numbers, -0.0 before
    +0.0; then the positive NaNs by payload."""
    dt = np.dtype(NP[vt])
    size = dt.itemsize
    if dt.kind == "u":
        return bits
    if dt.kind == "i":
        return bits - (1 << 8 * size) if bits >> (8 * size - 1) else bits
    x = struct.unpack("<f" if size == 4 else "<d", bits.to_bytes(size, "little"))[0]
    negative = bits >> (8 * size - 1)
    magnitude = bits & ((1 << (8 * size - 1)) - 1)
    if math.isnan(x):
        return (0, 0, -magnitude) if negative else (2, 0, magnitude)
    return (1, x, 0 if negative else 1) if x == 0 else (1, x, 0)


def _loop(op, tie, form, src, values, vt, num_in=None):
    """The definition, row by row."""
    src = [int(x) for x in src]
    counts = [(b - a) % (1 << 64) for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    ut = np.dtype("u%d" % np.dtype(NP[vt]).itemsize)
    bits = [int(b) for b in np.ascontiguousarray(values).view(ut)]
    idx, val, at = [], [], 0
    for r in range(m):
        best = None
        for i in range(at, min(at + counts[r], len(bits))):
            if best is None:
                best = i
                continue
            a, b = _rank(bits[i], vt), _rank(bits[best], vt)
            before = a < b if op == "argmin" else a > b
            if before or (a == b and tie == "last"):
                best = i
        at += counts[r]
        idx.append(NONE if best is None else best)
        val.append(int(np.array([none_value(op, vt)]).view(ut)[0]) if best is None else bits[best])
    return idx, val, at


def _values(kind, vt, n, rng):
    dt = np.dtype(NP[vt])
    ut = np.dtype("u%d" % dt.itemsize)
    if dt.kind == "f":
        one = np.array([1.0], dt).view(ut)[0]
        inf = np.array([np.inf], dt).view(ut)[0]
        sign = ut.type(1 << (8 * dt.itemsize - 1))
        special = np.array([0, sign, inf, inf | sign, inf + 1, (inf + 1) | sign, inf + 5, (inf + 5) | sign, np.iinfo(ut).max, np.iinfo(ut).max >> 1,
                            one, one | sign], ut)                            # ±0, ±inf, NaNs of both signs and several payloads, both none values
    else:
        info = np.iinfo(dt)
        special = np.array([info.min, info.max, info.min + 1, info.max - 1, 0, 1], dt).view(ut)
    if kind == "alphabet":                                                   # three letters: ties abound
        return rng.choice(special[[0, 1, -1]] if dt.kind == "f" else special[[0, 4, 5]], n).view(dt)
    if kind == "identities":                                                 # the none values themselves, as rows
        ids = np.array([none_value("argmin", vt), none_value("argmax", vt)], dt).view(ut)
        return rng.choice(ids, n).view(dt)
    return rng.choice(special, n).view(dt)


def test_the_model_against_a_plain_loop():
    """Counts with zeros at the start, in the middle and at the end, consecutive zeros, all ones, a single segment; both
    forms (the offsets with a base that is not 0), num_in below, equal to and above numel_seg, row counts around total
    (segments cut in the middle, segments beyond the rows); every value type x both ops x both ties on a three-letter
    alphabet, on the special values (±0.0, ±inf, NaNs of both signs, the types' extremes) and on the identities."""
    cases = ([0, 0, 3, 1, 0, 2, 0, 0, 0, 5, 1, 0], [0, 4], [4, 0], [0, 0, 0], [1] * 9, [7], [0], [], [2, 0, 0, 0, 0, 3], [1, 0, 1, 0, 1, 0], [13, 11])
    rng = np.random.default_rng(7)
    for counts in cases:
        for form in FORMS:
            cdt = (np.uint32, np.uint64)[len(counts) % 2]
            src = np.array(counts, cdt) if form == "counts" else (np.concatenate(([0], np.cumsum(counts))) + 12345).astype(cdt)
            for num_in in (None, 0, len(counts) // 2, len(counts), len(counts) + 3):
                total = sum(counts[:num_in])
                for n in sorted({0, 1, max(total - 1, 0), total, total + 4, sum(counts) // 2}):
                    for vt in NP:
                        for kind in ("alphabet", "special", "identities"):
                            v = _values(kind, vt, n, rng)
                            ut = np.dtype("u%d" % v.dtype.itemsize)
                            for op in OPS:
                                for tie in TIES:
                                    i, x, t = segarg(op, tie, form, src, v, num_in)
                                    what = (counts, form, num_in, n, vt, kind, op, tie)
                                    assert i.dtype == np.uint32 and x.dtype == NP[vt], what
                                    assert (i.tolist(), x.view(ut).tolist(), t) == _loop(op, tie, form, src, v, vt, num_in), what
    # the none values are what the header's table says
    assert none_value("argmin", "uint") == 0xffffffff and none_value("argmax", "uint") == 0
    assert none_value("argmin", "int") == 2**31 - 1 and none_value("argmax", "long") == -2**63
    assert np.array([none_value("argmin", "float")]).view(np.uint32)[0] == 0x7fffffff
    assert np.array([none_value("argmax", "float")]).view(np.uint32)[0] == 0xffffffff
    assert np.array([none_value("argmin", "double")]).view(np.uint64)[0] == 0x7fffffffffffffff
    assert np.array([none_value("argmax", "double")]).view(np.uint64)[0] == 0xffffffffffffffff
