"""CloSegScan (include/clo_segscan.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs and inputs alone, the
exact in-place alias passes the checks while a shifted or a wider one does not, m == 0 succeeds without a device, the
host stub answers the thin ABI's status-code table, and the C driver runs over the host stubs of the thin C-ABI
(tests/hoststub/*stub*.c, among them clo_hip_segscan_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone
program tests/segscan_host/segscan_host_test.c. The reference model the GPU tests compare against (segscan_model.py) is
checked here against a plain Python loop over Python integers, and the strata of the GPU fuzz (segscan_strata.py) are
shown to reach the tile edges they are there for; those of its second family (strata_lanes) the lanes and waves, seen
through tests/segscan_lane_model.py."""
import ctypes as C
import glob
import os
import re
import subprocess
import zlib

import numpy as np
import pytest

import cl_ops_amd as clo
from cl_ops_amd.api import CLO_ERROR_ARGS
from segscan_model import FORMS, NP, OPS, PAIRS, identity, merge_steps, segscan
from segscan_lane_model import ITEMS, WAVE, lanes
from segscan_strata import CLIPS, DISTS, LANE_DISTS, LANE_ITEMS, LANE_STRATA, LANE_WAVE, NUM_INS, SEED, STRATA, strata, strata_lanes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_segscan_new", "clo_segscan_destroy", "clo_segscan_with_device_data", "clo_segscan_with_host_data",
          "clo_segscan_get_context", "clo_segscan_get_op", "clo_segscan_get_form", "clo_segscan_get_inclusive",
          "clo_segscan_get_value_type", "clo_segscan_get_value_size", "clo_segscan_get_sum_type", "clo_segscan_get_sum_size",
          "clo_segscan_get_count_type", "clo_segscan_get_count_size")
THIN = ("clo_hip_segscan", "clo_hip_segscan_workspace_bytes", "clo_hip_segscan_tile")


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_segscan.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert '#define CLO_SEGSCAN_FORMS "counts, offsets"' in text
    assert ", ".join(clo.SEGSCAN_FORMS) == "counts, offsets" == ", ".join(FORMS)
    assert clo.SEGSCAN_OPS == ("sum", "min", "max") == OPS
    assert '#define CLO_SCAN_BY_KEY_OPS "%s"' % ", ".join(OPS) in open(os.path.join(ROOT, "include", "clo_scan_by_key.h")).read()
    for word in ("floating point", "reverse (suffix) scans", "initial value per segment", "several value columns", "numel >= 2^32",
                 "single-sweep look-back", "rank_out"):                       # what the header says is out of scope, and where ones are
        assert word in text, word
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(FORMS):                                             # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_SEGSCAN_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_segscan.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    for n in ("SegScan", "segscan_tile", "SEGSCAN_OPS", "SEGSCAN_FORMS"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert "segmented-scan" in clo.__doc__


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    text = open(os.path.join(ROOT, "cl_ops_amd", "csrc", "clo_segscan.c")).read()
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text


def test_tile_and_workspace_getters():
    for vs, ss in ((4, 4), (4, 8), (8, 8)):
        t = clo.segscan_tile(vs, ss)
        assert t >= 1024 and t % 256 == 0 and t < 65536, (vs, ss, t)
    assert clo.segscan_tile(4) == clo.segscan_tile(4, 4)
    for vs, ss in ((8, 4), (2, 4), (4, 2), (0, 4), (4, 0), (16, 16), (-1, 4)):
        assert clo.segscan_tile(vs, ss) == 0, (vs, ss)
    ws = clo.api.lib.clo_hip_segscan_workspace_bytes
    T = clo.segscan_tile(4, 4)
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    assert ws(0, 0) == 0
    for a in sizes:
        col = [ws(a, c) for c in sizes]
        row = [ws(n, a) for n in sizes]
        assert col == sorted(col) and row == sorted(row), (a, col, row)       # monotone in both arguments
        assert all(s % 256 == 0 for s in col + row)
        for c in sizes:
            assert ws(a, c) >= 8 * a + 16 * -(-(a + c) // T), (a, c)          # 8 bytes per segment plus 16 per tile of merge steps
            assert ws(a, c) <= 8 * a + 16 * -(-(a + c) // T) + 8 * (a // 4096 + 2) + 5 * 256, (a, c)   # and five roundings to 256


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for op in ("", "mean", "Sum", "sum ", "rank", None):
            assert "scan" in _refused(lambda: clo.SegScan(op, "counts", ctx))
            assert not lib.clo_segscan_new(op.encode() if op is not None else None, b"counts", None, ctx.h, 5, 5, 5, None)   # err NULL
        for form in ("", "lengths", "Counts", "count", "offsets ", None):
            assert "form" in _refused(lambda: clo.SegScan("sum", form, ctx))
            assert not lib.clo_segscan_new(b"sum", form.encode() if form is not None else None, None, ctx.h, 5, 5, 5, None)
        for opt in ("tile=4096", "inclusive", "inclusive=2", "inclusive=", "inclusive=1,tile=2", "exclusive=1", " ", "Inclusive=1"):
            assert "options" in _refused(lambda: clo.SegScan("sum", "counts", ctx, options=opt)), opt
            assert not lib.clo_segscan_new(b"sum", b"counts", opt.encode(), ctx.h, 5, 5, 5, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.SegScan("sum", "counts", ctx, count_type=ct))
            assert not lib.clo_segscan_new(b"sum", b"offsets", None, ctx.h, 5, 5, clo.CLO_TYPES[ct], None)
        for vt in ("char", "uchar", "short", "ushort", "half", "float", "double"):   # neither as the value nor as the sum type
            assert "int, uint, long or ulong" in _refused(lambda: clo.SegScan("sum", "counts", ctx, vt, "ulong"))
            assert "int, uint, long or ulong" in _refused(lambda: clo.SegScan("max", "offsets", ctx, "uint", vt))
            assert not lib.clo_segscan_new(b"sum", b"counts", None, ctx.h, clo.CLO_TYPES[vt], 7, 5, None)
        for vt, st in (("long", "int"), ("long", "uint"), ("ulong", "int"), ("ulong", "uint")):
            assert "narrower" in _refused(lambda: clo.SegScan("min", "counts", ctx, vt, st))
            assert not lib.clo_segscan_new(b"min", b"counts", None, ctx.h, clo.CLO_TYPES[vt], clo.CLO_TYPES[st], 5, None)
        # every op, form, legal type pair, count type and every spelling of the two kinds
        kinds = ((None, False), ("", False), ("inclusive=0", False), ("inclusive=1", True))
        for op in OPS:
            for form in FORMS:
                for k, (vt, st) in enumerate(PAIRS):
                    for ct in ("uint", "ulong"):
                        opt, incl = kinds[(k + (ct == "ulong")) % 4]
                        s = clo.SegScan(op, form, ctx, vt, st, ct, options=opt) if opt is not None else clo.SegScan(op, form, ctx, vt, st, ct)
                        assert (s.op, s.form, s.inclusive, s.value_type, s.value_size, s.sum_type, s.sum_size, s.count_type, s.count_size) == \
                            (op, form, incl, clo.CLO_TYPES[vt], np.dtype(NP[vt]).itemsize, clo.CLO_TYPES[st], np.dtype(NP[st]).itemsize,
                             clo.CLO_TYPES[ct], 4 if ct == "uint" else 8)
                        s.close()
        assert len(PAIRS) == 12
        s = clo.SegScan("sum", "counts", ctx, "long", inclusive=True)           # sum_type None: the value type; the keyword
        assert s.sum_type == clo.CLO_TYPES["long"] and s.inclusive
        s.close()

        c4, o4, c8 = clo.SegScan("sum", "counts", ctx), clo.SegScan("min", "offsets", ctx, "int", inclusive=True), clo.SegScan("max", "counts", ctx, "int", "long", "ulong")
        cn, of = np.zeros(16, np.uint32), np.zeros(17, np.uint32)
        cn8 = np.zeros(16, np.uint64)
        vi = np.zeros(16, np.uint32)
        do = np.arange(100, 116, dtype=np.uint32)
        do8 = np.arange(400, 416, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 16, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, vals, out_d, m_h=16, n=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_segscan_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_d), sp(out_n), m_h, n, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_seg", c4, cn, None, vi, do, m_h=1 << 32)
        both("numel_seg", o4, of, nin, vi, do, m_h=(1 << 32) + 5)
        both("numel must", c4, cn, None, vi, do, n=1 << 32)
        both("numel must", c8, cn8, None, vi, do8, n=1 << 63)
        both("the counts", c4, None, None, vi, do)                            # NULL counts_or_offsets
        both("the offsets", o4, None, None, vi, do)
        both("the offsets", o4, None, None, None, None, m_h=0, n=0)           # ... in the offsets form always
        both("values_in", c4, cn, None, None, do)
        both("values_in", c4, None, None, None, do, m_h=0, n=3)               # ... whenever numel > 0, even without a segment
        both("rank_out", c4, cn, None, None, do)                              # where "all ones" is to be had
        both("data_out", c4, cn, None, vi, None)
        both("data_out", c8, cn8, nin, vi, None, n=1)
        both("num_out", c4, cn, None, vi, do, out_n=None)
        both("num_out", o4, of, nin, vi, do, out_n=None)

        # overlap: data_out (sized by numel rows) on, inside, across the end of, sharing one element with an input or
        # num_in; num_out on each array and on num_in; the aliases of values_in that are not the exact one
        one = np.zeros(160, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, vi, cn)                                                         # data_out on the counts
        both(O, c4, one[0:32], None, vi, one[8:24], m_h=32)                                   # data_out inside the counts
        both(O, c4, one[0:16], None, vi, one[8:24])                                           # data_out across the counts' end
        both(O, c4, one[0:16], None, vi, one[15:31])                                          # one shared element
        both(O, o4, one[0:17], None, vi, one[16:32])                                          # data_out on the 17th offset
        both(O, c4, cn, n8(40, 42), vi, one[41:57])                                           # data_out on num_in's second half
        both(O, c4, cn, None, one[0:16], one[15:31])                                          # data_out on values_in's last row
        both(O, c4, one[100:104], None, one[0:64], one[63:127], m_h=4, n=64)                  # ... sized by numel, not numel_seg
        both(O, c4, cn, None, one[0:16], one[1:17])                                           # values_in shifted by one element
        both(O, c4, cn, None, one[1:17], one[0:16])                                           # ... the other way
        both(O, c8, cn8, None, one[0:16].view(np.int32), one[0:32].view(np.uint64))           # at values_in, with a wider sum type
        both(O, c8, cn8, None, vi, one[0:32].view(np.uint64), out_n=n8(30, 32))               # num_out on data_out's last row (8-byte rows)
        both(O, c4, cn, None, vi, one[0:16], out_n=n8(0, 2))                                  # num_out on data_out's first rows
        both(O, c4, cn, None, one[0:16], one[0:16], out_n=n8(2, 4))                           # ... in place: on the values too
        both(O, c4, one[0:16], None, vi, do, out_n=n8(14, 16))                                # num_out on the counts
        both(O, c4, cn, None, one[0:16], do, out_n=n8(2, 4))                                  # num_out on values_in
        both(O, c4, cn, n8(20, 22), vi, do, out_n=n8(20, 22))                                 # num_out on num_in
        assert np.array_equal(do, np.arange(100, 116)) and np.array_equal(do8, np.arange(400, 416))
        assert not one.any() and not cn.any() and not of.any() and not vi.any() and (num == 777).all() and nin[0] == 16

        # what lies next to another range without touching it, and the EXACT in-place alias with equal widths, are
        # accepted as far as the checks go: the call then fails for want of a device, not with CLO_ERROR_ARGS (the
        # counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(150, 152)
        l4 = clo.SegScan("max", "counts", ctx, "long", "ulong", "uint")
        for obj, args in ((c4, (one[0:16], None, one[16:32], one[32:48])),
                          (c4, (one[0:16], n8(16, 18), one[18:34], one[34:50])),
                          (o4, (one[0:17], None, one[17:33], one[33:49])),
                          (o4, (one[0:17], n8(18, 20), one[20:36], one[36:52])),
                          (c4, (one[0:16], None, one[16:32], one[16:32])),                   # in place, uint -> uint
                          (o4, (one[0:17], n8(18, 20), one[20:36], one[20:36])),             # in place, int -> int, with num_in
                          (l4, (one[0:16], None, one[16:48], one[16:48]))):                  # in place, long -> ulong
            err = clo.api._Err()
            src, n_in, vals, out_d = args
            assert not lib.clo_segscan_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out_d), sp(out_n), 16, 16, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:150] == 1).all()
        l4.close()

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
                    s = clo.SegScan(op, form, ctx, "int", "long", ct, inclusive=op == "min")
                    src = np.zeros(1 if form == "offsets" else 0, cdt)
                    d, total = s.with_host_data(src, np.arange(5, dtype=np.int32), fill=-3)   # rows, but no segment to put them in
                    assert total == 0 and d.dtype == np.int64 and (d == -3).all() and d.size == 5
                    d, total = s.with_host_data(src, np.zeros(0, np.int32))
                    assert total == 0 and d.size == 0
                    src = np.arange(1, 6, dtype=cdt)                              # four or five segments, of which num_in takes none
                    d, total = s.with_host_data(src, np.arange(20, dtype=np.int32), num_in=0, fill=9)
                    assert total == 0 and (d == 9).all()
                    # raw: num_out becomes 0, data_out is not touched
                    out_d, num = np.full(20, 7, np.int64), C.c_size_t(55)
                    zero = C.c_size_t(0)
                    vals = np.zeros(20, np.int32)
                    err = clo.api._Err()
                    assert lib.clo_segscan_with_host_data(s.h, None, None, src.ctypes.data, C.byref(zero), vals.ctypes.data,
                                                          out_d.ctypes.data, C.byref(num), 4, 20, err.ref)
                    err.raise_if_set()
                    assert num.value == 0 and (out_d == 7).all()
                    s.close()
    finally:
        ctx.close()


# ---- the thin ABI's status codes: the table tests/test_gpu_segscan.py asks of the device code, asked here of the stub ----

STATUS_SOURCE = r"""
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include "clo_hip.h"
int main(void) {
	static uint64_t cn[16], num, nin = 16;
	static uint32_t vi[16], out[16];
	const size_t need = clo_hip_segscan_workspace_bytes(16, 16);
	void* ws = aligned_alloc(256, need);
	char* odd = (char*) vi + 2;
#define ROW(name, call) printf("%s %d\n", name, (call))
	ROW("ok", clo_hip_segscan(0, 0, 0, cn, 8, &nin, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("ok_inclusive_offsets", clo_hip_segscan(2, 1, 1, cn, 8, NULL, vi, out, &num, 15, 16, 4, 4, ws, need, NULL));
	ROW("ok_in_place", clo_hip_segscan(1, 1, 0, cn, 8, NULL, vi, vi, &num, 16, 16, 5, 4, ws, need, NULL));
	ROW("ok_empty", clo_hip_segscan(0, 0, 0, NULL, 4, NULL, vi, out, &num, 0, 16, 5, 5, NULL, 0, NULL));
	ROW("op", clo_hip_segscan(3, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("op_negative", clo_hip_segscan(-1, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("inclusive", clo_hip_segscan(0, 2, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("form", clo_hip_segscan(0, 0, 2, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("count_size", clo_hip_segscan(0, 0, 0, cn, 2, NULL, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("value_type", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 9, 5, ws, need, NULL));
	ROW("sum_type", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 3, ws, need, NULL));
	ROW("sum_narrower", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 7, 5, ws, need, NULL));
	ROW("numel_seg", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, (size_t) 1 << 32, 16, 5, 5, ws, need, NULL));
	ROW("numel", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, (size_t) 1 << 32, 5, 5, ws, need, NULL));
	ROW("counts_null", clo_hip_segscan(0, 0, 0, NULL, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("offsets_null_empty", clo_hip_segscan(0, 0, 1, NULL, 8, NULL, NULL, NULL, &num, 0, 0, 5, 5, ws, need, NULL));
	ROW("values_null", clo_hip_segscan(0, 0, 0, cn, 8, NULL, NULL, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("out_null", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, NULL, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("num_out_null", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, NULL, 16, 16, 5, 5, ws, need, NULL));
	ROW("num_out_odd", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, (uint64_t*) ((char*) &num + 4), 16, 16, 5, 5, ws, need, NULL));
	ROW("num_in_odd", clo_hip_segscan(0, 0, 0, cn, 8, (uint64_t*) ((char*) cn + 4), vi, out, &num, 16, 16, 5, 5, ws, need, NULL));
	ROW("counts_odd", clo_hip_segscan(0, 0, 0, (char*) cn + 4, 8, NULL, vi, out, &num, 15, 16, 5, 5, ws, need, NULL));
	ROW("values_odd", clo_hip_segscan(0, 0, 0, cn, 8, NULL, odd, out, &num, 16, 15, 5, 5, ws, need, NULL));
	ROW("out_odd", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, (char*) out + 2, &num, 16, 15, 5, 5, ws, need, NULL));
	ROW("ws_null", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, NULL, need, NULL));
	ROW("ws_short", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, need - 1, NULL));
	ROW("ws_zero", clo_hip_segscan(0, 0, 0, cn, 8, NULL, vi, out, &num, 16, 16, 5, 5, ws, 0, NULL));
	free(ws);
	return 0;
}
"""

# CLO_HIP_EARGS -1, CLO_HIP_EUNSUPPORTED -2, CLO_HIP_EWORKSPACE -3 (include/clo_hip.h); tests/test_gpu_segscan.py makes
# the same calls on device memory and expects the same answers
STATUS_TABLE = (("ok", 0), ("ok_inclusive_offsets", 0), ("ok_in_place", 0), ("ok_empty", 0), ("op", "EARGS"), ("op_negative", "EARGS"),
                ("inclusive", "EARGS"), ("form", "EARGS"), ("count_size", "EUNSUPPORTED"), ("value_type", "EUNSUPPORTED"),
                ("sum_type", "EUNSUPPORTED"), ("sum_narrower", "EUNSUPPORTED"), ("numel_seg", "EARGS"), ("numel", "EARGS"),
                ("counts_null", "EARGS"), ("offsets_null_empty", "EARGS"), ("values_null", "EARGS"), ("out_null", "EARGS"),
                ("num_out_null", "EARGS"), ("num_out_odd", "EARGS"), ("num_in_odd", "EARGS"), ("counts_odd", "EARGS"),
                ("values_odd", "EARGS"), ("out_odd", "EARGS"), ("ws_null", "EARGS"), ("ws_short", "EWORKSPACE"), ("ws_zero", "EWORKSPACE"))


def status_codes():
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    return {n: int(re.search(r"#define CLO_HIP_%s\s+\(?(-?\d+)\)?" % n, text).group(1)) for n in ("EARGS", "EUNSUPPORTED", "EWORKSPACE")}


def test_the_stub_answers_the_status_code_table(tmp_path):
    src = tmp_path / "status.c"
    src.write_text(STATUS_SOURCE)
    exe = str(tmp_path / "status")
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-w", "-fsanitize=address,undefined",
                           "-I" + os.path.join(ROOT, "include"), str(src), os.path.join(ROOT, "tests", "hoststub", "clo_hip_segscan_stub.c"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr, r.stderr[-3000:]
    got = [tuple(l.split()) for l in r.stdout.splitlines()]
    codes = status_codes()
    assert got == [(n, str(codes.get(c, c))) for n, c in STATUS_TABLE]


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segscan_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "segscan_host", "segscan_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("segscan host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


def _loop(op, form, src, values, vt, st, inclusive, num_in=None):
    """The definition, over Python integers: the C cast, then the running op over the rows of each segment that exist;
    rows at and beyond the total are not written."""
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    bits, signed = 8 * np.dtype(NP[st]).itemsize, np.dtype(NP[st]).kind == "i"
    wrap = lambda x: ((x + (1 << (bits - 1))) % (1 << bits)) - (1 << (bits - 1)) if signed else x % (1 << bits)
    vals = [wrap(int(x)) for x in values]                                     # int(x) of a numpy integer keeps its sign: C's cast
    f = {"sum": lambda a, b: wrap(a + b), "min": min, "max": max}[op]
    out, at = [], 0
    for r in range(m):
        acc = int(identity(op, st))
        for i in range(at, at + counts[r]):
            if i < len(vals):
                after = f(acc, vals[i])
                out.append(after if inclusive else acc)
                acc = after
        at += counts[r]
    return out, at


def test_the_model_against_a_plain_loop():
    """Counts with zeros at the start, in the middle and at the end, consecutive zeros, all ones, a single segment; both
    forms (the offsets with a base that is not 0), num_in below, equal to and above numel_seg, row counts around total
    (segments cut in the middle, rows beyond the total), every type pair with values at the types' extremes, both kinds."""
    cases = ([0, 0, 3, 1, 0, 2, 0, 0, 0, 5, 1, 0], [0, 4], [4, 0], [0, 0, 0], [1] * 9, [7], [0], [], [2, 0, 0, 0, 0, 3], [1, 0, 1, 0, 1, 0], [40, 3, 0, 29],
             [3, 200, 0, 1, 131, 2])                                          # segments above segscan_model.LONG rows: scanned on their own
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
                                for incl in (False, True):
                                    d, t = segscan(op, form, src, v, st, incl, num_in)
                                    what = (counts, form, num_in, n, vt, st, op, incl)
                                    assert d.dtype == NP[st] and d.size == min(t, n), what
                                    assert (d.tolist(), t) == _loop(op, form, src, v, vt, st, incl, num_in), what
    d, t = segscan("sum", "counts", np.array([1 << 63, 1 << 63, 5], np.uint64), np.arange(4, dtype=np.uint32), "uint")   # ends modulo 2^64
    assert t == 5 and d.size == 4                                             # (the ends do not ascend: the rows' contents are unspecified)


def test_the_fuzz_strata_reach_the_tile_edges():
    """What tests/test_gpu_segscan_fuzz.py runs, seen through the model alone: every value of every dimension is dealt,
    n <= 4 T everywhere, and among the strata there are a tile in which nothing closes (with rows before and after it),
    a close on a tile's first and on a tile's last step, empty segments at a tile edge, totals above and below n."""
    T = clo.segscan_tile(4, 4)
    ss = strata(T)
    assert len(ss) == STRATA >= 200
    seen = {k: set() for k in ("form", "count_type", "op", "inclusive", "dist", "clip", "num_mode")}
    pairs = set()
    reach = dict(no_close=0, first=0, last=0, empty_edge=0, above=0, below=0, exact=0, carry_through=0)
    for s in ss:
        for k in seen:
            seen[k].add(s[k])
        pairs.add((s["value_type"], s["sum_type"]))
        assert s["n"] == s["values"].size <= 4 * T and s["values"].dtype == NP[s["value_type"]]
        close, m, total = merge_steps(s["form"], s["src"], s["n"], s["num_in"])
        steps = m + s["n"]
        tiles = -(-steps // T)
        per_tile = np.bincount(close // T, minlength=tiles) if m else np.zeros(tiles, np.int64)
        reach["no_close"] += int((per_tile == 0).any())
        # the carry passes THROUGH a tile: nothing closes in it, it is not the first, and a later tile has rows below ct
        inner = [t for t in range(1, tiles - 1) if per_tile[t] == 0]
        reach["carry_through"] += int(bool(inner) and min(total, s["n"]) > 0)
        reach["first"] += int(m > 0 and (close % T == 0).any())
        reach["last"] += int(m > 0 and (close % T == T - 1).any())
        if m:
            ends = close - np.arange(m)
            empty = np.concatenate(([ends[0] == 0], ends[1:] == ends[:-1]))
            reach["empty_edge"] += int((empty & ((close % T == 0) | (close % T == T - 1))).any())
        reach["above"] += int(total > s["n"])
        reach["below"] += int(total < s["n"])
        reach["exact"] += int(total == s["n"])
    assert seen == dict(form=set(FORMS), count_type={"uint", "ulong"}, op=set(OPS), inclusive={False, True}, dist=set(DISTS),
                        clip=set(CLIPS), num_mode=set(NUM_INS))
    assert pairs == set(PAIRS)
    assert all(v >= 1 for v in reach.values()), reach


def test_the_lane_strata_reach_the_lanes_and_waves():
    """What the second family of tests/test_gpu_segscan_fuzz.py runs, seen through the lane model: every value of every
    dimension is dealt, in_place only where the widths match and in at least a quarter of the strata, n <= 3 T; among
    them a lane with 17 closes, a wave of nothing but closes, a close on a lane's first and on a lane's last step, a
    lane with no close, a tile without rows. The first family is what it was."""
    T = clo.segscan_tile(4, 4)
    assert (LANE_ITEMS, LANE_WAVE) == (ITEMS, WAVE) and SEED == 20231
    first = strata(T)
    assert len(first) == STRATA == 216 and "in_place" not in first[0]
    digest = zlib.crc32(b"".join(s["src"].tobytes() + s["values"].tobytes() for s in first))
    assert (sum(s["n"] for s in first), sum(s["m_h"] for s in first), digest) == (1330631, 235600, 3640288040)   # as before the second family
    ss = strata_lanes(T)
    assert len(ss) == LANE_STRATA == 96
    seen = {k: set() for k in ("form", "count_type", "op", "inclusive", "dist", "clip", "num_mode", "in_place")}
    pairs, placed = set(), 0
    reach = dict(lane_of_closes=0, wave_of_closes=0, bit_0=0, bit_16=0, lane_without=0, tile_without_rows=0, above=0, below=0)
    for s in ss:
        for k in seen:
            seen[k].add(s[k])
        pairs.add((s["value_type"], s["sum_type"]))
        assert s["n"] == s["values"].size <= 3 * T and s["values"].dtype == NP[s["value_type"]] and s["m_h"] <= 3 * T
        same = np.dtype(NP[s["value_type"]]).itemsize == np.dtype(NP[s["sum_type"]]).itemsize
        assert same or not s["in_place"]
        placed += int(s["in_place"])
        L = lanes(s["form"], s["src"], s["n"], T, s["num_in"], s["values"].dtype.itemsize)
        close, m, total = merge_steps(s["form"], s["src"], s["n"], s["num_in"])
        assert np.array_equal(L.na, np.bincount(close // T, minlength=L.tiles)[:L.tiles] if m else np.zeros(L.tiles, np.int64))
        reach["lane_of_closes"] += int((L.ne == ITEMS).any())
        reach["wave_of_closes"] += int((L.wave_closes == ITEMS * WAVE).any())
        reach["bit_0"] += int((L.closes & 1).any())
        reach["bit_16"] += int(((L.closes >> (ITEMS - 1)) & 1).any())
        reach["lane_without"] += int(((L.ne == 0) & (L.steps == ITEMS)).any())
        reach["tile_without_rows"] += int(((L.nb == 0) & (L.cnt > 0)).any())
        reach["above"] += int(total > s["n"])
        reach["below"] += int(total < s["n"])
    assert seen == dict(form=set(FORMS), count_type={"uint", "ulong"}, op=set(OPS), inclusive={False, True}, dist=set(LANE_DISTS),
                        clip=set(CLIPS), num_mode=set(NUM_INS), in_place={False, True})
    assert pairs == set(PAIRS)
    assert 4 * placed >= LANE_STRATA, placed
    assert all(v >= 1 for v in reach.values()), reach
