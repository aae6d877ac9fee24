"""CloSegSort (include/clo_segsort.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs alone, m == 0 succeeds
without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among them
clo_hip_segsort_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/segsort_host/segsort_host_test.c. The reference model the GPU tests compare against (segsort_model.py) is checked
here against a plain Python loop that sorts every clipped segment with Python's stable sort. The move rule of the merge
passes is restated here from its prose, and the cases of tests/test_gpu_segsort.py above ten tiles
are shown to have the masks they claim; the table of thin-ABI argument tuples of that file runs through the host stub
built as a shared library, so that the stub and the device code answer the same tuples alike."""
import ctypes as C
import glob
import os
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from merge_model import order_key
from segsort_model import FORMS, KEY_NP, segsort

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_segsort_new", "clo_segsort_destroy", "clo_segsort_with_device_data", "clo_segsort_with_host_data",
          "clo_segsort_get_context", "clo_segsort_get_form", "clo_segsort_get_key_type", "clo_segsort_get_key_size",
          "clo_segsort_get_value_size", "clo_segsort_get_count_type", "clo_segsort_get_count_size")
THIN = ("clo_hip_segsort", "clo_hip_segsort_workspace_bytes", "clo_hip_segsort_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_segsort.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SEGSORT_FORMS "counts, offsets"' in text
    assert ", ".join(clo.SEGSORT_FORMS) == "counts, offsets" == ", ".join(FORMS)
    for word in ("clo_expand.h", "clo_segreduce.h", "IEEE total order", "STABLE", "no in-place form", "clo_sort_*",   # the segments, the order, the advice
                 "descending order", "get_key", "numel >= 2^32", "values wider than", "k smallest per segment"):          # what is out of scope
        assert word in text, word
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    assert "second copy of the rows" in text
    for i, n in enumerate(FORMS):                                             # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_SEGSORT_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_segsort.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("SegSort", "segsort_tile", "SEGSORT_FORMS"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert "segmented-sort" in clo.__doc__


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    import re
    text = open(os.path.join(ROOT, "cl_ops_amd", "csrc", "clo_segsort.c")).read()
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text


def test_tile_and_workspace_getters():
    T = clo.segsort_tile(4, 0)
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            t = clo.segsort_tile(ks, vs)
            assert t >= 1024 and t % 256 == 0, (ks, vs, t)
    assert clo.segsort_tile() == T
    for ks, vs in ((3, 0), (0, 4), (16, 0), (4, 1), (4, 2), (4, 16), (-1, 4), (4, -4)):
        assert clo.segsort_tile(ks, vs) == 0, (ks, vs)
    ws = clo.api.lib.clo_hip_segsort_workspace_bytes
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            assert ws(0, 0, ks, vs) == 0
            for a in sizes:
                col = [ws(a, c, ks, vs) for c in sizes]
                row = [ws(n, a, ks, vs) for n in sizes]
                assert col == sorted(col) and row == sorted(row), (a, col, row)   # monotone in both counts
                assert all(s % 256 == 0 for s in col + row)
                for c in sizes:
                    assert ws(a, c, ks, vs) >= 8 * a + c * (ks + vs + 1), (a, c)  # the ends, a copy of the rows and a byte per row


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
            assert "form" in _refused(lambda: clo.SegSort(form, ctx))
            assert not lib.clo_segsort_new(form.encode() if form is not None else None, None, ctx.h, 5, 0, 5, None)   # err NULL
        for opt in ("tile=4096", "descending", " "):
            assert "options" in _refused(lambda: clo.SegSort("counts", ctx, options=opt))
            assert not lib.clo_segsort_new(b"counts", opt.encode(), ctx.h, 5, 0, 5, None)
        for vs in (1, 2, 3, 5, 12, 16, 1 << 40):
            assert "value_size" in _refused(lambda: clo.SegSort("counts", ctx, "uint", vs))
            assert not lib.clo_segsort_new(b"offsets", None, ctx.h, 5, vs, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.SegSort("counts", ctx, count_type=ct))
            assert not lib.clo_segsort_new(b"offsets", None, ctx.h, 5, 4, clo.CLO_TYPES[ct], None)
        for kt in (-1, 11, 100):
            assert not lib.clo_segsort_new(b"counts", None, ctx.h, kt, 0, 5, None)
        for form in FORMS:                                                    # every form, key type, value size, count type, both spellings of no options
            for kt in KEY_NP:
                for vs in (0, 4, 8):
                    for ct, opt in (("uint", None), ("ulong", "")):
                        s = clo.SegSort(form, ctx, kt, vs, ct, options=opt)
                        assert (s.form, s.key_type, s.key_size, s.value_size, s.count_type, s.count_size) == \
                            (form, clo.CLO_TYPES[kt], np.dtype(KEY_NP[kt]).itemsize, vs, clo.CLO_TYPES[ct], 4 if ct == "uint" else 8)
                        s.close()

        k0, c4, o4, c8 = (clo.SegSort("counts", ctx), clo.SegSort("counts", ctx, "uint", 4), clo.SegSort("offsets", ctx, "float", 4),
                          clo.SegSort("counts", ctx, "long", 8, "ulong"))
        cn, of = np.zeros(16, np.uint32), np.zeros(17, np.uint32)
        cn8 = np.zeros(16, np.uint64)
        ki, vi = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        ki8, vi8 = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
        ko, vo = np.arange(100, 116, dtype=np.uint32), np.arange(200, 216, dtype=np.uint32)
        ko8, vo8 = np.arange(400, 416, dtype=np.uint64), np.arange(500, 516, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 16, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, keys, vals, out_k, out_v, m_h=16, n=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_segsort_with_host_data(obj.h, None, None, p(src), sp(n_in), p(keys), p(vals), p(out_k), p(out_v), sp(out_n), m_h, n,
                                                err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_seg", c4, cn, None, ki, vi, ko, vo, m_h=1 << 32)
        both("numel_seg", o4, of, nin, ki, vi, ko, vo, m_h=(1 << 32) + 5)
        both("numel must", c4, cn, None, ki, vi, ko, vo, n=1 << 32)
        both("numel must", c8, cn8, None, ki8, vi8, ko8, vo8, n=1 << 63)
        both("the counts", c4, None, None, ki, vi, ko, vo)                     # NULL counts_or_offsets
        both("the offsets", o4, None, None, ki, vi, ko, vo)
        both("the offsets", o4, None, None, None, None, ko, vo, m_h=0, n=0)    # ... in the offsets form always
        both("keys_in", c4, cn, None, None, vi, ko, vo)
        both("keys_in", c4, None, None, None, vi, ko, vo, m_h=0, n=3)          # ... even without a segment
        both("value_size 0", k0, cn, None, ki, vi, ko, None)                   # values passed to a keys-only sort
        both("value_size 0", k0, cn, None, ki, None, ko, vo)
        both("values_out", c4, cn, None, ki, vi, ko, None)
        both("values_out", c4, cn, None, ki, None, ko, None)                   # ... the arg form too
        both("values_in", c8, cn8, None, ki8, None, ko8, vo8)                  # no arg form with 8-byte values
        both("keys_out", c4, cn, None, ki, vi, None, vo)                       # keys_out may be NULL in the arg form only
        both("keys_out", k0, cn, None, ki, None, None, None)
        both("keys_out", c8, cn8, None, ki8, vi8, None, vo8)
        both("num_out", c4, cn, None, ki, vi, ko, vo, out_n=None)
        both("num_out", o4, of, nin, ki, None, None, vo, out_n=None)

        # overlap: an output (sized by numel rows) on, inside, across the end of, sharing one element with an input,
        # num_in, or the other output; num_out on each array and on num_in
        one = np.zeros(200, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, ki, vi, cn, vo)                                                      # keys_out on the counts
        both(O, c4, one[0:32], None, ki, vi, one[8:24], vo, m_h=32)                                # keys_out inside the counts
        both(O, c4, one[0:16], None, ki, vi, ko, one[15:31])                                       # values_out sharing the counts' last element
        both(O, o4, one[0:17], None, ki, vi, one[16:32], vo)                                       # keys_out on the 17th offset
        both(O, c4, cn, n8(40, 42), ki, vi, ko, one[41:57])                                        # values_out on num_in's second half
        both(O, c4, cn, None, one[0:16], vi, one[15:31], vo)                                       # keys_out on keys_in's last row
        both(O, c4, cn, None, one[0:16], vi, one[0:16], vo)                                        # keys_out on keys_in: no in-place form
        both(O, c4, cn, None, ki, one[0:16], ko, one[0:16])                                        # values_out on values_in
        both(O, c4, cn, None, one[0:16], vi, ko, one[15:31])                                       # values_out on keys_in's last row
        both(O, c4, cn, None, ki, one[0:16], one[15:31], vo)                                       # keys_out on values_in's last row
        both(O, c4, cn, None, ki, vi, one[0:16], one[15:31])                                       # the outputs share one element
        both(O, c4, cn, None, ki, vi, one[0:16], one[0:16])                                        # the outputs on each other
        both(O, c4, cn, None, one[0:64], vi, one[63:79], vo, m_h=4, n=64)                          # ... sized by numel, not numel_seg
        both(O, c8, cn8, None, ki8, vi8, one[0:32].view(np.uint64), vo8, out_n=n8(30, 32))         # num_out on keys_out's last row (8-byte rows)
        both(O, c4, cn, None, ki, vi, ko, one[0:16], out_n=n8(0, 2))                               # num_out on values_out's first rows
        both(O, c4, one[0:16], None, ki, vi, ko, vo, out_n=n8(14, 16))                             # num_out on the counts
        both(O, c4, cn, None, one[0:16], vi, ko, vo, out_n=n8(2, 4))                               # num_out on keys_in
        both(O, c4, cn, None, ki, one[0:16], ko, vo, out_n=n8(2, 4))                               # num_out on values_in
        both(O, c4, cn, n8(20, 22), ki, vi, ko, vo, out_n=n8(20, 22))                              # num_out on num_in
        assert np.array_equal(ko, np.arange(100, 116)) and np.array_equal(vo, np.arange(200, 216))
        assert np.array_equal(ko8, np.arange(400, 416)) and np.array_equal(vo8, np.arange(500, 516))
        assert not one.any() and not cn.any() and not of.any() and not ki.any() and not vi.any() and (num == 777).all() and nin[0] == 16

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS (the counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(190, 192)
        for obj, args in ((c4, (one[0:16], None, one[16:32], one[32:48], one[48:64], one[64:80])),
                          (c4, (one[0:16], n8(16, 18), one[18:34], None, one[34:50], one[50:66])),
                          (o4, (one[0:17], None, one[17:33], one[33:49], one[49:65], one[65:81])),
                          (o4, (one[0:17], n8(18, 20), one[20:36], None, None, one[36:52]))):
            err = clo.api._Err()
            src, n_in, keys, vals, out_k, out_v = args
            assert not lib.clo_segsort_with_host_data(obj.h, None, None, p(src), sp(n_in), p(keys), p(vals), p(out_k), p(out_v), sp(out_n), 16, 16, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:190] == 1).all()

        # the Python view checks the element types
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint64), np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.int32))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            o4.with_host_data(np.zeros(0, np.uint32), np.zeros(4, np.float32))
        for s in (k0, c4, o4, c8):
            s.close()
    finally:
        ctx.close()


def test_no_segments_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for form in FORMS:
            for ct, cdt in (("uint", np.uint32), ("ulong", np.uint64)):
                for kt, vs in (("int", 0), ("half", 4), ("double", 8)):
                    s = clo.SegSort(form, ctx, kt, vs, ct)
                    kdt = KEY_NP[kt]
                    vals = (lambda n: np.zeros(n, "u%d" % vs) if vs else None)
                    src = np.zeros(1 if form == "offsets" else 0, cdt)
                    k, v, total = s.with_host_data(src, np.arange(5).astype(kdt), vals(5))   # rows, but no segment to put them in
                    assert total == 0 and k.size == 0 and k.dtype == kdt and (v is None) == (vs == 0)
                    k, v, total = s.with_host_data(src, np.zeros(0, kdt), vals(0))
                    assert total == 0 and k.size == 0
                    src = np.arange(1, 6, dtype=cdt)                          # four or five segments, of which num_in takes none
                    k, v, total = s.with_host_data(src, np.arange(20).astype(kdt), vals(20), num_in=0)
                    assert total == 0 and k.size == 0
                    # raw: num_out becomes 0, the outputs are not touched
                    out_k, out_v, num = np.full(20, 7, kdt), np.full(20, 9, np.uint64), C.c_size_t(55)
                    zero = C.c_size_t(0)
                    keys, vin = np.zeros(20, kdt), np.zeros(20, np.uint64)
                    err = clo.api._Err()
                    assert lib.clo_segsort_with_host_data(s.h, None, None, src.ctypes.data, C.byref(zero), keys.ctypes.data,
                                                          vin.ctypes.data if vs else None, out_k.ctypes.data, out_v.ctypes.data if vs else None,
                                                          C.byref(num), 4, 20, err.ref)
                    err.raise_if_set()
                    assert num.value == 0 and (out_k == 7).all() and (out_v == 9).all()
                    s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segsort_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "segsort_host", "segsort_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("segsort host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(form, src, keys, num_in=None):
    """The definition: Python's stable sort of every clipped segment's rows by their order keys."""
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    ok = [int(x) for x in order_key(keys)]
    out, at = [], 0
    for r in range(m):
        rows = [i for i in range(at, at + counts[r]) if i < len(ok)]
        at += counts[r]
        out += sorted(rows, key=lambda i: ok[i])
    return out, at


def test_the_order_keys():
    """Signed keys numerically, floating-point keys in IEEE total order: -NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN."""
    for dt in (np.float16, np.float32, np.float64):
        ut = np.dtype("u%d" % np.dtype(dt).itemsize)
        neg_nan = (np.array([np.nan], dt).view(ut) | ut.type(1 << (8 * ut.itemsize - 1))).view(dt)
        k = np.concatenate((neg_nan, np.array([-np.inf, -1.0, -0.0, 0.0, 1.0, np.inf, np.nan], dt)))
        ok = order_key(k)
        assert (np.diff(ok.astype(object)) > 0).all(), (dt, ok)
    for dt in (np.int8, np.int16, np.int32, np.int64):
        info = np.iinfo(dt)
        k = np.array([info.min, -2, -1, 0, 1, info.max], dt)
        assert (np.diff(order_key(k).astype(object)) > 0).all(), dt


def test_the_model_against_a_plain_loop():
    """Counts with zeros at the start, in the middle and at the end, consecutive zeros, all ones, a single segment; both
    forms (the offsets with a base that is not 0), num_in below, equal to and above numel_seg, row counts around total
    (segments cut in the middle, segments beyond the rows), every key type with few distinct keys, so that ties are
    common."""
    cases = ([0, 0, 3, 1, 0, 2, 0, 0, 0, 5, 1, 0], [0, 4], [4, 0], [0, 0, 0], [1] * 9, [7], [0], [], [2, 0, 0, 0, 0, 30], [1, 0, 1, 0, 1, 0])
    rng = np.random.default_rng(7)
    for counts in cases:
        for form in FORMS:
            for cdt in (np.uint32, np.uint64):
                src = np.array(counts, cdt) if form == "counts" else (np.concatenate(([0], np.cumsum(counts))) + 12345).astype(cdt)
                for num_in in (None, 0, len(counts) // 2, len(counts), len(counts) + 3):
                    total = sum(counts[:num_in])
                    for n in sorted({0, 1, max(total - 1, 0), total, total + 4, sum(counts) // 2}):
                        for kt, dt in KEY_NP.items():
                            pool = rng.integers(0, 256, 4 * np.dtype(dt).itemsize, dtype=np.uint8).view(dt)
                            keys = pool[rng.integers(0, 4, n)]
                            p, t = segsort(form, src, keys, num_in)
                            what = (counts, form, num_in, n, kt)
                            assert p.dtype == np.uint32 and p.size == min(t, n), what
                            assert (p.tolist(), t) == (_loop(form, src, keys, num_in)[0], _loop(form, src, keys, num_in)[1]), what
    p, t = segsort("counts", np.array([1 << 63, 1 << 63, 5], np.uint64), np.arange(4, dtype=np.uint32))   # ends modulo 2^64
    assert t == 5                                                             # (the ends do not ascend: the rows' contents are unspecified)


# ---- the move rule of DESIGN.md section 22, restated from its prose, and what the GPU cases promise about it ----

def move_mask(s, e, T):
    """Bit p: pass p moves the segment [s, e). Pass p works on blocks of W = T * 2^p rows; with a the block of the
    segment's first row and b of its last, the segment moves iff there is an odd k with a < k <= b (the middle of a pair
    of blocks strictly inside it). From the pass at which a == b on, nothing moves."""
    mask, p = 0, 0
    while s < e:
        W = T << p
        a, b = s // W, (e - 1) // W
        if a == b:
            break
        odd = a + 1 if (a + 1) % 2 else a + 2                                 # the smallest odd k above a
        if odd <= b:
            mask |= 1 << p
        p += 1
    return mask


def segment_masks(counts, n, T):
    """[(s, e, mask)] of the non-empty clipped segments."""
    ends = np.minimum(np.cumsum(np.asarray(counts, np.int64)), n)
    starts = np.concatenate(([0], ends[:-1]))
    return [(int(s), int(e), move_mask(int(s), int(e), T)) for s, e in zip(starts, ends) if e > s]


def opposite_moves_in_one_tile(segs, T):
    """The tiles whose first row's and last row's segments differ, both move in some pass p, and have moves of different
    parity left at p: one is read from the workspace and the other from the outputs by the same work-group."""
    found = []
    by_tile = {}
    for s, e, m in segs:
        if m:
            by_tile.setdefault(s // T, []).append((s, e, m))                  # the tile of its first row: it is B there
            by_tile.setdefault((e - 1) // T, []).append((s, e, m))            # ... and A in the tile of its last row
    for t, both in by_tile.items():
        A = [g for g in both if g[0] < t * T]                                 # starts before the tile
        B = [g for g in both if g[1] > (t + 1) * T]                           # ends behind it
        for a in A:
            for b in B:
                if a is b:
                    continue
                for p in range(32):
                    if (a[2] >> p) & 1 and (b[2] >> p) & 1 and (bin(a[2] >> p).count("1") + bin(b[2] >> p).count("1")) % 2:
                        found.append((t, p))
    return found


def test_the_move_masks_the_gpu_cases_pin():
    """What tests/test_gpu_segsort.py's cases above ten tiles claim to reach, shown on the CPU: the pinned masks, a tile
    whose two boundary segments move in opposite directions in one pass, and every pass 0 .. 8 as the highest bit of
    some mask."""
    import test_gpu_segsort as G
    T = clo.segsort_tile(4, 0)
    assert move_mask(0, T, T) == 0 and move_mask(T - 1, T + 1, T) == 1 and move_mask(0, 3 * T, T) == 0b11
    assert move_mask(3 * T + T // 2, 4 * T + T // 2, T) == 0b100 and move_mask(0, 8 * T + 1, T) == 0b1111   # section 22's own examples
    highest = set()
    n = G.PINNED_TILES * T
    segs = segment_masks(G.pinned_counts(T, G.PINNED_TILES, G.PINNED), n, T)
    long = [g for g in segs if g[1] - g[0] > 200]
    assert [(2 * s // T, 2 * e // T) for s, e, _ in long] == list(G.PINNED)
    assert tuple(m for _, _, m in long) == G.PINNED_MASKS == (0b101, 0b1001, 0b10011, 0b100001, 0b1000000)
    highest |= {m.bit_length() - 1 for _, _, m in segs if m}
    for k in G.SINGLE_BIT:
        segs = segment_masks(G.pinned_counts(T, k + 2, ((2 * k - 1, 2 * k + 1),), seed=k), (k + 2) * T, T)
        assert [m for s, e, m in segs if e - s > 200] == [k]
        highest |= {m.bit_length() - 1 for _, _, m in segs if m}
    for size in G.big_sizes(T):
        m = move_mask(0, size, T)
        assert m == (1 << (m.bit_length())) - 1                               # a segment from row 0 moves at every pass up to its last
        highest.add(m.bit_length() - 1)
    assert {3, 4, 5} <= {move_mask(0, size, T).bit_length() - 1 for size in G.big_sizes(T)}
    counts = G.end_to_end_counts(T)
    assert int(counts.sum()) == G.END_TO_END_TILES * T and counts.min() >= 1 and counts[:-1].min() >= T // 2 and counts.max() <= 40 * T
    segs = segment_masks(counts, G.END_TO_END_TILES * T, T)
    assert opposite_moves_in_one_tile(segs, T), "no tile of the end-to-end case has A and B with different parities in a pass where both move"
    assert max(bin(m).count("1") for _, _, m in segs) >= 4 and any((e - s) > 32 * T for s, e, _ in segs)   # a merge with a part above 4 T
    highest |= {m.bit_length() - 1 for _, _, m in segs if m}
    assert set(range(9)) <= highest, sorted(highest)


def _aligned(nbytes, fill=0xA5, align=256):
    """(owner, address, view): nbytes of host memory at a multiple of `align`, filled."""
    raw = np.full(nbytes + align, fill, np.uint8)
    at = -raw.ctypes.data % align
    return raw, raw.ctypes.data + at, raw[at:at + nbytes]


def test_the_host_stub_answers_the_thin_abi_table_as_the_device_code_does(tmp_path):
    """tests/hoststub/clo_hip_segsort_stub.c restates the rules of clo_hip_segsort; the GPU test runs the table of
    test_gpu_segsort.ThinABI through the device code, this runs the same table through the stub: the same status for
    every refused tuple (but the workspace's alignment, which the stub cannot check), nothing written, and the model's
    rows for every accepted one."""
    import test_gpu_segsort as G
    so = str(tmp_path / "libsegsort_stub.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-shared", "-fPIC", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "hoststub", "clo_hip_segsort_stub.c"), "-o", so])
    stub = C.CDLL(so)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    stub.clo_hip_segsort.restype = ci
    stub.clo_hip_segsort.argtypes = [ci, vp, ci, vp, vp, vp, vp, vp, vp, sz, sz, ci, ci, vp, sz, vp]
    stub.clo_hip_segsort_workspace_bytes.restype = sz
    stub.clo_hip_segsort_workspace_bytes.argtypes = [sz, sz, ci, ci]
    lib = clo.api.lib
    T = clo.segsort_tile(4, 0)
    abi = G.ThinABI(T, clo.CLO_TYPES, lib.clo_hip_segsort_workspace_bytes)
    for a, b, ks, vs in ((abi.m_h, abi.n, 4, 4), (abi.m_h + 1, abi.n + 1, 8, 8), (0, 0, 4, 4), (5, 0, 1, 0), (0, 7, 2, 4), (abi.m_h, abi.n, 3, 4)):
        assert stub.clo_hip_segsort_workspace_bytes(a, b, ks, vs) == lib.clo_hip_segsort_workspace_bytes(a, b, ks, vs), (a, b, ks, vs)
    held = {}
    for name, data in (("cn", abi.counts), ("ki", abi.keys), ("vi", abi.vals), ("ni", abi.num_in)):
        held[name] = _aligned(data.nbytes)
        held[name][2][:] = data.view(np.uint8)
    for name, nbytes in (("ko", abi.out_bytes), ("vo", abi.out_bytes), ("num", 16), ("ws", abi.big)):
        held[name] = _aligned(nbytes)
    P = {k: v[1] for k, v in held.items()}
    call = lambda kw: stub.clo_hip_segsort(*[kw[k] for k in G.ThinABI.ORDER], None)
    checked = 0
    for what, kw, status, on_stub in abi.refusals(P):
        if on_stub:
            assert call(kw) == status, what
            checked += 1
    assert checked >= 40
    for name in ("ko", "vo", "num"):
        assert (held[name][2] == 0xA5).all(), "a refused call wrote " + name
    for what, kw, spec in abi.accepted(P):
        assert call(kw) == 0, what
        want_k, want_v, total = abi.want(spec, kw["form"]) if spec[4] else (None, None, 0)
        assert int(held["num"][2][:8].view(np.uint64)[0]) == total, what
        for name, want in (("ko", want_k), ("vo", want_v)):
            if kw[name] is not None and want is not None:
                at = 4 * spec[0]
                assert np.array_equal(held[name][2][at:at + want.nbytes], want.view(np.uint8)), (what, name)
    for name, data in (("cn", abi.counts), ("ki", abi.keys), ("vi", abi.vals), ("ni", abi.num_in)):
        assert np.array_equal(held[name][2], data.view(np.uint8)), name
