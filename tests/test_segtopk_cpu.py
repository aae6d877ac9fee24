"""CloSegTopK (include/clo_segtopk.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile, cap and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs alone, m == 0 and k == 0
succeed without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c, among
them clo_hip_segtopk_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/segtopk_host/segtopk_host_test.c. The reference model the GPU tests compare against (segtopk_model.py) is checked
here against a plain Python loop over Python integers and struct-unpacked floats, and the host stub, built as a shared
library, against the model."""
import ctypes as C
import glob
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from segtopk_model import FORMS, KEY_NP, WHICH, dense, segtopk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_segtopk_new", "clo_segtopk_destroy", "clo_segtopk_with_device_data", "clo_segtopk_with_host_data",
          "clo_segtopk_get_context", "clo_segtopk_get_which", "clo_segtopk_get_form", "clo_segtopk_get_key_type", "clo_segtopk_get_key_size",
          "clo_segtopk_get_value_size", "clo_segtopk_get_count_type", "clo_segtopk_get_count_size")
THIN = ("clo_hip_segtopk", "clo_hip_segtopk_workspace_bytes", "clo_hip_segtopk_tile", "clo_hip_segtopk_k_max")


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = _read("include", "clo_segtopk.h")
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SEGTOPK_WHICH "smallest, largest"' in text and "CLO_SEGREDUCE_FORMS" in text
    assert ", ".join(clo.SEGTOPK_WHICH) == "smallest, largest" == ", ".join(WHICH)
    for word in ("clo_segsort.h", "IEEE total order", "CloSegArg", "CloTopK", "CloSegSort", "ASCENDING row index", "stride k", "UNCLAMPED",
                 "clo_hip_segtopk_k_max", "NOT written", "no in-place form"):
        assert word in text, word
    scope = text[text.index("Out of scope"):]
    for word in ("k per segment read from device memory", "compacted (CSR) output", "padding", "get_key", "numel >= 2^32",
                 "values wider than 8 bytes", "a k above the cap"):
        assert word in scope, word
    text = _read("include", "clo_hip.h")
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(WHICH):                                             # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_SEGTOPK_%s %d\n" % (n.upper(), i) in text, n
    for i, n in enumerate(FORMS):
        assert "#define CLO_HIP_SEGTOPK_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_segtopk.h"' in _read("include", "cl_ops.h")
    for n in ("SegTopK", "segtopk_tile", "segtopk_k_max", "SEGTOPK_WHICH"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert "segmented-top-k" in clo.__doc__


def test_the_older_headers_point_here_and_keep_their_words():
    """The out-of-scope lines of the three headers that named this operation keep the words existing tests pin, and now
    say where it is."""
    for name, word in (("clo_segsort.h", "k smallest per segment"), ("clo_segarg.h", "k smallest per segment"), ("clo_topk.h", "k per segment")):
        text = _read("include", name)
        scope = text[text.index("Out of scope"):]
        assert word in scope and "clo_segtopk.h" in scope, name
    design = _read("DESIGN.md")
    assert "CloSegTopK" in design and "§28" in design


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    text = _read("cl_ops_amd", "csrc", "clo_segtopk.c")
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text


def test_the_kernels_share_the_tile_sort_with_segsort():
    """One text of the on-chip network: both kernel files include the header and neither keeps a copy of its steps."""
    hdr = _read("cl_ops_amd", "csrc", "hip", "clo_hip_tile_sort_device.h")
    for word in ("clo_ts_at(", "struct clo_ts_item", "clo_ts_less(", "clo_ts_cx(", "clo_ts_reg_step(", "clo_ts_lds_step(", "i ^ ((i >> 3) & 7u)"):
        assert word in hdr, word
    for name in ("clo_hip_segsort.hip", "clo_hip_segtopk.hip"):
        text = _read("cl_ops_amd", "csrc", "hip", name)
        assert '#include "clo_hip_tile_sort_device.h"' in text and "CLO_TS_SORT(" in text, name
        assert "(i >> 3) & 7u" not in text and "asm" not in text, name


def test_tile_cap_and_workspace_getters():
    T, cap = clo.segtopk_tile(4, 0), clo.segtopk_k_max(4, 0)
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            assert clo.segtopk_tile(ks, vs) == T and T >= 1024 and T % 256 == 0
            assert clo.segtopk_k_max(ks, vs) == cap and 256 <= cap <= T
    assert clo.segtopk_tile() == T == clo.segsort_tile() and clo.segtopk_k_max() == cap
    for ks, vs in ((3, 0), (0, 4), (16, 0), (4, 1), (4, 2), (4, 16), (-1, 4), (4, -4)):
        assert clo.segtopk_tile(ks, vs) == 0 and clo.segtopk_k_max(ks, vs) == 0, (ks, vs)
    ws = clo.api.lib.clo_hip_segtopk_workspace_bytes
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    kk = (0, 1, 2, 63, 64, cap)
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            for k in kk:
                assert ws(0, 0, k, ks, vs) == 0
            for k in kk:
                for a in sizes:
                    col = [ws(a, c, k, ks, vs) for c in sizes]
                    row = [ws(n, a, k, ks, vs) for n in sizes]
                    assert col == sorted(col) and row == sorted(row), (a, k, col, row)   # monotone in both counts
                    assert all(s % 256 == 0 for s in col + row)
            for a in (1, T + 1, 1 << 20):
                by_k = [ws(a, a, k, ks, vs) for k in kk]
                assert by_k == sorted(by_k) and by_k[-1] > by_k[0], (a, by_k)   # ... and in k
                tiles = -(-a // T)
                assert ws(a, a, cap, ks, vs) >= 8 * a + 5 * a + tiles * 2 * cap * (ks + 4)   # the ends, a byte and a number per row, two lists per tile
    for ks, vs in ((3, 0), (4, 2)):
        assert ws(5, 5, 4, ks, vs) == 0


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    cap = clo.segtopk_k_max(4, 4)
    try:
        for which in ("", "biggest", "Smallest", "small", "largest ", None):
            assert "which" in _refused(lambda: clo.SegTopK(which, "counts", ctx))
            assert not lib.clo_segtopk_new(which.encode() if which is not None else None, b"counts", None, ctx.h, 5, 0, 5, None)   # err NULL
        for form in ("", "lengths", "Counts", "count", "offsets ", None):
            assert "form" in _refused(lambda: clo.SegTopK("smallest", form, ctx))
            assert not lib.clo_segtopk_new(b"largest", form.encode() if form is not None else None, None, ctx.h, 5, 0, 5, None)
        for opt in ("k=4", "descending", " "):
            assert "options" in _refused(lambda: clo.SegTopK("smallest", "counts", ctx, options=opt))
            assert not lib.clo_segtopk_new(b"smallest", b"counts", opt.encode(), ctx.h, 5, 0, 5, None)
        for vs in (1, 2, 3, 5, 12, 16, 1 << 40):
            assert "value_size" in _refused(lambda: clo.SegTopK("smallest", "counts", ctx, "uint", vs))
            assert not lib.clo_segtopk_new(b"smallest", b"offsets", None, ctx.h, 5, vs, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.SegTopK("largest", "counts", ctx, count_type=ct))
            assert not lib.clo_segtopk_new(b"largest", b"offsets", None, ctx.h, 5, 4, clo.CLO_TYPES[ct], None)
        for kt in (-1, 11, 100):
            assert not lib.clo_segtopk_new(b"smallest", b"counts", None, ctx.h, kt, 0, 5, None)
        for which in WHICH:                                                   # every which, form, key type, value size, count type
            for form in FORMS:
                for kt in KEY_NP:
                    for vs in (0, 4, 8):
                        for ct, opt in (("uint", None), ("ulong", "")):
                            s = clo.SegTopK(which, form, ctx, kt, vs, ct, options=opt)
                            assert (s.which, s.form, s.key_type, s.key_size, s.value_size, s.count_type, s.count_size) == \
                                (which, form, clo.CLO_TYPES[kt], np.dtype(KEY_NP[kt]).itemsize, vs, clo.CLO_TYPES[ct], 4 if ct == "uint" else 8)
                            s.close()

        k0, c4, o4, c8 = (clo.SegTopK("smallest", "counts", ctx), clo.SegTopK("largest", "counts", ctx, "uint", 4),
                          clo.SegTopK("smallest", "offsets", ctx, "float", 4), clo.SegTopK("largest", "counts", ctx, "long", 8, "ulong"))
        # 8 segments, 16 rows, k = 2: outputs of 16 slots
        cn, of = np.zeros(8, np.uint32), np.zeros(9, np.uint32)
        cn8 = np.zeros(8, np.uint64)
        ki, vi = np.zeros(16, np.uint32), np.zeros(16, np.uint32)
        ki8, vi8 = np.zeros(16, np.uint64), np.zeros(16, np.uint64)
        ko, vo, co = np.arange(100, 116, dtype=np.uint32), np.arange(200, 216, dtype=np.uint32), np.arange(300, 308, dtype=np.uint32)
        ko8, vo8 = np.arange(400, 416, dtype=np.uint64), np.arange(500, 516, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 8, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, keys, vals, out_k, out_v, out_c=co, m_h=8, n=16, k=2, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_segtopk_with_host_data(obj.h, None, None, p(src), sp(n_in), p(keys), p(vals), p(out_k), p(out_v), p(out_c), sp(out_n), m_h, n, k,
                                                err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_seg must", c4, cn, None, ki, vi, ko, vo, m_h=1 << 32)
        both("numel_seg must", o4, of, nin, ki, vi, ko, vo, m_h=(1 << 32) + 5)
        both("numel must", c4, cn, None, ki, vi, ko, vo, n=1 << 32)
        both("numel must", c8, cn8, None, ki8, vi8, ko8, vo8, n=1 << 63)
        both("cap", c4, cn, None, ki, vi, ko, vo, k=cap + 1)                   # k above the cap
        both("cap", c8, cn8, None, ki8, vi8, ko8, vo8, k=1 << 50)
        both("numel_seg * k", c4, cn, None, ki, vi, ko, vo, m_h=1 << 24, k=256)   # m_h * k = 2^32
        both("numel_seg * k", c4, cn, None, ki, vi, ko, vo, m_h=(1 << 32) - 1, k=cap)
        both("the counts", c4, None, None, ki, vi, ko, vo)                     # NULL counts_or_offsets
        both("the offsets", o4, None, None, ki, vi, ko, vo)
        both("the offsets", o4, None, None, None, None, ko, vo, m_h=0, n=0)    # ... in the offsets form always
        both("keys_in", c4, cn, None, None, vi, ko, vo)
        both("keys_in", c4, None, None, None, vi, ko, vo, m_h=0, n=3)          # ... even without a segment
        both("value_size 0", k0, cn, None, ki, vi, ko, None)                   # values passed to a keys-only top-k
        both("value_size 0", k0, cn, None, ki, None, ko, vo)
        both("values_out", c4, cn, None, ki, vi, ko, None)
        both("values_out", c4, cn, None, ki, None, ko, None)                   # ... the arg form too
        both("values_in", c8, cn8, None, ki8, None, ko8, vo8)                  # no arg form with 8-byte values
        both("keys_out", c4, cn, None, ki, vi, None, vo)                       # keys_out may be NULL in the arg form only
        both("keys_out", k0, cn, None, ki, None, None, None)
        both("keys_out", c8, cn8, None, ki8, vi8, None, vo8)
        both("counts_out", c4, cn, None, ki, vi, ko, vo, out_c=None)
        both("counts_out", o4, of, nin, ki, None, None, vo, out_c=None)
        both("num_out", c4, cn, None, ki, vi, ko, vo, out_n=None)
        both("num_out", o4, of, nin, ki, None, None, vo, out_n=None)

        # overlap: an output (keys_out and values_out sized by numel_seg * k slots, counts_out by numel_seg) on, inside,
        # across the end of, sharing one element with an input, num_in, or another output; num_out on each array
        one = np.zeros(200, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, ki, vi, cn, vo, k=1)                                                 # keys_out on the counts
        both(O, c4, one[0:32], None, ki, vi, one[8:24], vo, m_h=32, k=1)                           # keys_out inside the counts... of 32 slots
        both(O, c4, one[0:8], None, ki, vi, ko, one[7:23])                                         # values_out sharing the counts' last element
        both(O, o4, one[0:9], None, ki, vi, one[8:24], vo)                                         # keys_out on the 9th offset
        both(O, c4, cn, n8(40, 42), ki, vi, ko, one[41:57])                                        # values_out on num_in's second half
        both(O, c4, cn, None, one[0:16], vi, one[15:31], vo)                                       # keys_out on keys_in's last row
        both(O, c4, cn, None, one[0:16], vi, one[0:16], vo)                                        # keys_out on keys_in: no in-place form
        both(O, c4, cn, None, ki, one[0:16], ko, one[0:16])                                        # values_out on values_in
        both(O, c4, cn, None, one[0:16], vi, ko, one[15:31])                                       # values_out on keys_in's last row
        both(O, c4, cn, None, ki, vi, one[0:16], one[15:31])                                       # the outputs share one slot
        both(O, c4, cn, None, ki, vi, one[0:16], one[0:16])                                        # the outputs on each other
        both(O, c4, cn, None, ki, vi, one[0:32], one[31:63], k=4)                                  # ... sized by numel_seg * k, not by numel
        both(O, c4, cn, None, ki, vi, one[0:16], vo, out_c=one[15:23])                             # counts_out on keys_out's last slot
        both(O, c4, cn, None, ki, vi, ko, one[0:16], out_c=one[8:16])                              # counts_out inside values_out
        both(O, c4, cn, None, ki, one[0:16], ko, vo, out_c=one[15:23])                             # counts_out on values_in's last row
        both(O, c4, one[0:8], None, ki, vi, ko, vo, out_c=one[0:8])                                # counts_out on the counts
        both(O, c8, cn8, None, ki8, vi8, one[0:32].view(np.uint64), vo8, out_n=n8(30, 32))         # num_out on keys_out's last slot (8-byte slots)
        both(O, c4, cn, None, ki, vi, ko, one[0:16], out_n=n8(0, 2))                               # num_out on values_out's first slots
        both(O, c4, cn, None, ki, vi, ko, vo, out_c=one[0:8], out_n=n8(6, 8))                      # num_out on counts_out
        both(O, c4, one[0:8], None, ki, vi, ko, vo, out_n=n8(6, 8))                                # num_out on the counts
        both(O, c4, cn, None, one[0:16], vi, ko, vo, out_n=n8(2, 4))                               # num_out on keys_in
        both(O, c4, cn, n8(20, 22), ki, vi, ko, vo, out_n=n8(20, 22))                              # num_out on num_in
        assert np.array_equal(ko, np.arange(100, 116)) and np.array_equal(vo, np.arange(200, 216)) and np.array_equal(co, np.arange(300, 308))
        assert np.array_equal(ko8, np.arange(400, 416)) and np.array_equal(vo8, np.arange(500, 516))
        assert not one.any() and not cn.any() and not of.any() and not ki.any() and not vi.any() and (num == 777).all() and nin[0] == 8

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS (the counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(190, 192)
        for obj, args in ((c4, (one[0:8], None, one[8:24], one[24:40], one[40:56], one[56:72], one[72:80])),
                          (c4, (one[0:8], n8(8, 10), one[10:26], None, one[26:42], one[42:58], one[58:66])),
                          (o4, (one[0:9], None, one[9:25], one[25:41], one[41:57], one[57:73], one[73:81])),
                          (o4, (one[0:9], n8(10, 12), one[12:28], None, None, one[28:44], one[44:52]))):
            err = clo.api._Err()
            src, n_in, keys, vals, out_k, out_v, out_c = args
            assert not lib.clo_segtopk_with_host_data(obj.h, None, None, p(src), sp(n_in), p(keys), p(vals), p(out_k), p(out_v), p(out_c), sp(out_n), 8, 16, 2,
                                                      err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:190] == 1).all()

        # the Python view checks the element types
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint64), np.zeros(4, np.uint32), 2)
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.int32), 2)
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32), 2, np.zeros(4, np.uint64))
        with pytest.raises(ValueError):
            o4.with_host_data(np.zeros(0, np.uint32), np.zeros(4, np.float32), 2)
        for s in (k0, c4, o4, c8):
            s.close()
    finally:
        ctx.close()


def test_no_segments_and_k_zero_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for form in FORMS:
            for ct, cdt in (("uint", np.uint32), ("ulong", np.uint64)):
                for which, kt, vs in (("smallest", "int", 0), ("largest", "half", 4), ("smallest", "double", 8)):
                    s = clo.SegTopK(which, form, ctx, kt, vs, ct)
                    kdt = KEY_NP[kt]
                    vals = (lambda n: np.zeros(n, "u%d" % vs) if vs else None)
                    src = np.zeros(1 if form == "offsets" else 0, cdt)
                    k, v, c, total = s.with_host_data(src, np.arange(5).astype(kdt), 3, vals(5))   # rows, but no segment to put them in
                    assert total == 0 and k.shape == (0, 3) and k.dtype == kdt and (v is None) == (vs == 0) and c.size == 0
                    k, v, c, total = s.with_host_data(src, np.zeros(0, kdt), 0, vals(0))            # ... and k = 0
                    assert total == 0 and k.shape == (0, 0)
                    for fill in (-1, 0xA5A5A5A5, 1 << 40):              # a fill the outputs' types cannot hold is cast, not refused
                        k, v, c, total = s.with_host_data(src, np.arange(5).astype(kdt), 3, vals(5), fill=fill)
                        assert total == 0 and k.shape == (0, 3)
                    src = np.arange(1, 6, dtype=cdt)                          # four or five segments, of which num_in takes none
                    k, v, c, total = s.with_host_data(src, np.arange(20).astype(kdt), 2, vals(20), num_in=0)
                    assert total == 0 and k.shape == (0, 2) and c.size == 0
                    # raw: num_out becomes 0, the outputs are not touched
                    out_k, out_v, out_c, num = np.full(20, 7, kdt), np.full(20, 9, np.uint64), np.full(5, 11, np.uint32), C.c_size_t(55)
                    zero = C.c_size_t(0)
                    keys, vin = np.zeros(20, kdt), np.zeros(20, np.uint64)
                    err = clo.api._Err()
                    assert lib.clo_segtopk_with_host_data(s.h, None, None, src.ctypes.data, C.byref(zero), keys.ctypes.data,
                                                          vin.ctypes.data if vs else None, out_k.ctypes.data, out_v.ctypes.data if vs else None,
                                                          out_c.ctypes.data, C.byref(num), 4, 20, 4, err.ref)
                    err.raise_if_set()
                    assert num.value == 0 and (out_k == 7).all() and (out_v == 9).all() and (out_c == 11).all()
                    s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segtopk_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "segtopk_host", "segtopk_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("segtopk host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


_FMT = {np.float16: "e", np.float32: "f", np.float64: "d"}


def _rank(which, key):
    """A Python number (or pair) whose order is the selection's, from the key's value alone: integers numerically;
    floating-point keys through struct as Python floats, NaNs by their payload beyond the infinities, -0 below +0."""
    dt = key.dtype
    if dt.kind in "iu":
        x = (0, int(key))
    else:
        raw = key.tobytes()
        bits = int.from_bytes(raw, "little")
        sign = bits >> (8 * dt.itemsize - 1)
        mag = bits & ((1 << (8 * dt.itemsize - 1)) - 1)
        val = struct.unpack("<" + _FMT[dt.type], raw)[0]
        if val != val:                                                        # NaN: beyond the infinity of its sign, by payload
            x = (-2, -mag) if sign else (2, mag)
        elif val == 0:
            x = (0, -0.5 if sign else 0.5)                                    # -0 < +0, between the negative and the positive numbers
        else:
            x = (-1, -mag) if sign else (1, mag)                              # finite and infinite: by sign, then by magnitude's bits
    return tuple(-c for c in x) if which == "largest" else x


def _loop(which, form, src, keys, k, num_in=None):
    """The definition: per clipped segment, Python's stable sort of the rows by their rank, cut at k."""
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    rk = [_rank(which, keys[i]) for i in range(len(keys))]
    out, cnt, at = [], [], 0
    for r in range(m):
        rows = [i for i in range(at, at + counts[r]) if i < len(rk)]
        at += counts[r]
        best = sorted(rows, key=lambda i: rk[i])[:k]
        out.append(best + [-1] * (k - len(best)))
        cnt.append(len(best))
    return out, cnt, at


def test_the_model_against_a_plain_loop():
    """Counts with zeros at the start, in the middle and at the end, all ones, a single segment; both forms (the offsets
    with a base that is not 0), num_in below, equal to and above numel_seg, row counts around total, every key type
    with few distinct keys (ties are common; for the floats both zeros, infinities and NaNs of both signs), both which,
    k below, at and above the segment lengths."""
    cases = ([0, 0, 3, 1, 0, 2, 0, 0, 0, 5, 1, 0], [0, 4], [4, 0], [0, 0, 0], [1] * 9, [7], [0], [], [2, 0, 0, 0, 0, 30])
    rng = np.random.default_rng(7)
    for counts in cases:
        for form in FORMS:
            cdt = (np.uint32, np.uint64)[len(counts) % 2]
            src = np.array(counts, cdt) if form == "counts" else (np.concatenate(([0], np.cumsum(counts))) + 12345).astype(cdt)
            for num_in in (None, 0, len(counts) // 2, len(counts) + 3):
                total = sum(counts[:num_in])
                for n in sorted({0, max(total - 1, 0), total, total + 4}):
                    for kt, dt in KEY_NP.items():
                        if np.dtype(dt).kind == "f":
                            pool = np.array([-np.inf, -1.5, -0.0, 0.0, 2.0, np.inf, np.nan, -np.nan], dt)
                            pool = np.concatenate((pool, (pool[6:].view("u%d" % pool.itemsize) + 3).view(dt)))   # two more payloads
                        else:
                            pool = rng.integers(0, 256, 4 * np.dtype(dt).itemsize, dtype=np.uint8).view(dt)
                        keys = pool[rng.integers(0, pool.size, n)]
                        for which in WHICH:
                            for k in (1, 3, 40):
                                idx, cnt, t = segtopk(which, form, src, keys, k, num_in)
                                want = _loop(which, form, src, keys, k, num_in)
                                what = (counts, form, num_in, n, kt, which, k)
                                assert idx.dtype == np.int64 and cnt.dtype == np.uint32, what
                                assert (idx.tolist(), cnt.tolist(), t) == want, what
    idx, cnt, t = segtopk("smallest", "counts", np.array([1 << 63, 1 << 63, 5], np.uint64), np.arange(4, dtype=np.uint32), 2)   # ends modulo 2^64
    assert t == 5                                                             # (the ends do not ascend: the rows' contents are unspecified)
    assert dense(np.array([[1, -1]]), np.array([5, 6, 7], np.uint8), 9).tolist() == [[6, 9]]


def _aligned(nbytes, fill=0xA5, align=256):
    """(owner, address, view): nbytes of host memory at a multiple of `align`, filled."""
    raw = np.full(nbytes + align, fill, np.uint8)
    at = -raw.ctypes.data % align
    return raw, raw.ctypes.data + at, raw[at:at + nbytes]


def test_the_host_stub_answers_as_the_model_and_the_thin_abi_table(tmp_path):
    """tests/hoststub/clo_hip_segtopk_stub.c restates the rules of clo_hip_segtopk: its workspace size is the library's,
    it answers the table of refused argument tuples of tests/test_gpu_segtopk.py with the same status codes (but the
    workspace's alignment, which it cannot check) and writes nothing, and its rows are the model's."""
    import test_gpu_segtopk as G
    so = str(tmp_path / "libsegtopk_stub.so")
    subprocess.check_call(["gcc", "-O1", "-std=c11", "-shared", "-fPIC", "-w", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "hoststub", "clo_hip_segtopk_stub.c"), "-o", so])
    stub = C.CDLL(so)
    vp, ci, sz = C.c_void_p, C.c_int, C.c_size_t
    stub.clo_hip_segtopk.restype = ci
    stub.clo_hip_segtopk.argtypes = [ci, ci, vp, ci, vp, vp, vp, vp, vp, vp, vp, sz, sz, sz, ci, ci, vp, sz, vp]
    stub.clo_hip_segtopk_workspace_bytes.restype = sz
    stub.clo_hip_segtopk_workspace_bytes.argtypes = [sz, sz, sz, ci, ci]
    lib = clo.api.lib
    T, cap = clo.segtopk_tile(4, 0), clo.segtopk_k_max(4, 0)
    for a, b, k, ks, vs in ((700, 5 * T + 1, 24, 4, 4), (701, 5 * T, cap, 8, 8), (0, 0, 4, 4, 4), (5, 0, 1, 1, 0), (0, 7, 2, 2, 4), (9, 9, 3, 3, 4)):
        assert stub.clo_hip_segtopk_workspace_bytes(a, b, k, ks, vs) == lib.clo_hip_segtopk_workspace_bytes(a, b, k, ks, vs), (a, b, k, ks, vs)
    rng = np.random.default_rng(5)
    counts = rng.geometric(1 / 9, 120).astype(np.uint32)
    counts[::7] = 0
    m_h, n, k = counts.size, int(counts.sum()), 5
    keys, vals = rng.integers(-4, 5, n).astype(np.int32), rng.integers(0, 1 << 32, n, dtype=np.uint32)
    need = lib.clo_hip_segtopk_workspace_bytes(m_h, n, k, 4, 4)
    held = {}
    for name, data in (("cn", counts), ("ki", keys), ("vi", vals), ("ni", np.array([m_h - 3, 0], np.uint64))):
        held[name] = _aligned(data.nbytes)
        held[name][2][:] = data.view(np.uint8)
    for name, nbytes in (("ko", 4 * m_h * k), ("vo", 4 * m_h * k), ("co", 4 * m_h), ("num", 16), ("ws", need + 512)):
        held[name] = _aligned(nbytes)
    P = {name: v[1] for name, v in held.items()}
    INT = clo.CLO_TYPES["int"]
    good = dict(which=0, form=0, cn=P["cn"], cs=4, ni=P["ni"], ki=P["ki"], vi=P["vi"], ko=P["ko"], vo=P["vo"], co=P["co"], num=P["num"], m_h=m_h, n=n, k=k,
                kt=INT, vs=4, ws=P["ws"], wsb=need)
    call = lambda kw: stub.clo_hip_segtopk(*[kw[x] for x in G.ORDER], None)
    checked = 0
    for what, change, status in G.thin_table(T, cap, INT):
        if what == "workspace misaligned":
            continue
        kw = dict(good)
        for name, v in change.items():
            kw[name] = (good[name] + v if v is not None and name in ("cn", "ni", "ki", "vi", "ko", "vo", "co", "num", "ws", "wsb") else v)
        assert call(kw) == status, what
        checked += 1
    assert checked >= 28
    for name in ("ko", "vo", "co", "num"):
        assert (held[name][2] == 0xA5).all(), "a refused call wrote " + name
    for which in (0, 1):
        for num_in in (None, P["ni"]):
            for arg in (False, True):
                for name in ("ko", "vo", "co", "num"):
                    held[name][2][:] = 0xA5
                assert call(dict(good, which=which, ni=num_in, vi=None if arg else P["vi"])) == 0
                idx, cnt, total = segtopk(WHICH[which], "counts", counts, keys, k, None if num_in is None else m_h - 3)
                m = idx.shape[0]
                assert int(held["num"][2][:8].view(np.uint64)[0]) == total
                want_c = np.full(m_h, 0xA5A5A5A5, np.uint32)
                want_c[:m] = cnt
                assert np.array_equal(held["co"][2].view(np.uint32), want_c)
                for name, col in (("ko", keys), ("vo", np.arange(n, dtype=np.uint32) if arg else vals)):
                    want = np.full((m_h, k), 0xA5A5A5A5, np.uint32)
                    want[:m] = dense(idx, col.view(np.uint32), want[:m])
                    assert np.array_equal(held[name][2].view(np.uint32).reshape(m_h, k), want), (which, num_in, arg, name)
    for name, data in (("cn", counts), ("ki", keys), ("vi", vals)):
        assert np.array_equal(held[name][2], data.view(np.uint8)), name
