"""CloSegFSum (include/clo_segfsum.h) on the CPU: the library exports the new public and thin-ABI entry points and the
headers declare them, the tile and workspace getters answer, every refusal comes back as CLO_ERROR_ARGS through an
offline context before anything touches a device (err == NULL included) and leaves the outputs and the inputs alone,
m == 0 succeeds without a device, and the C driver runs over the host stubs of the thin C-ABI (tests/hoststub/*stub*.c,
among them clo_hip_segfsum_stub.c) under AddressSanitizer + UBSan, driven by the stand-alone program
tests/segfsum_host/segfsum_host_test.c. The model of the addition order the GPU tests compare against (segfsum_model.py)
is checked here: with an integer sum type it is segreduce_model's sum on every layout (which row reaches which segment);
on telescoping inputs it gives the exact sums; on rounding and mixed-sign inputs it stays within gamma_D times the sum of
the magnitudes of math.fsum; and each of six deliberately different stages changes a bit on the committed inputs."""
import ctypes as C
import glob
import math
import os
import re
import subprocess

import numpy as np
import pytest

import cl_ops_amd as clo
import segfsum_model as M
from cl_ops_amd.api import CLO_ERROR_ARGS
from segfsum_model import FORMS, NP, PAIRS, same_bits, segfsum
from segreduce_model import segreduce

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PUBLIC = ("clo_segfsum_new", "clo_segfsum_destroy", "clo_segfsum_with_device_data", "clo_segfsum_with_host_data",
          "clo_segfsum_get_context", "clo_segfsum_get_form", "clo_segfsum_get_value_type", "clo_segfsum_get_value_size",
          "clo_segfsum_get_sum_type", "clo_segfsum_get_sum_size", "clo_segfsum_get_count_type", "clo_segfsum_get_count_size")
THIN = ("clo_hip_segfsum", "clo_hip_segfsum_workspace_bytes", "clo_hip_segfsum_tile")
T = M.TILE


def test_exports():
    for n in PUBLIC + THIN:
        assert hasattr(clo.api.lib, n), n
    text = open(os.path.join(ROOT, "include", "clo_segfsum.h")).read()
    for n in PUBLIC:
        assert n + "(" in text, n
    assert "CLO_SEGREDUCE_FORMS" in text and "THE ORDER IS THE CONTRACT" in text and "D(tiles)" in text and "gamma_D" in text
    assert "MAY depend on where the segment lies" in text
    for word in ("means", "float min and max", "half sums", "bfloat16", "compensated or exact summation", "several value columns", "numel >= 2^32",
                 "reduce\n * by key, scan by key and the segmented scan"):
        assert word in text[text.index("Out of scope"):], word                # what the header says is out of scope
    text = open(os.path.join(ROOT, "include", "clo_hip.h")).read()
    for n in THIN:
        assert n + "(" in text, n
    for i, n in enumerate(FORMS):                                             # the thin ABI's numbers are the names' positions
        assert "#define CLO_HIP_SEGFSUM_%s %d\n" % (n.upper(), i) in text, n
    assert '#include "clo_segfsum.h"' in open(os.path.join(ROOT, "include", "cl_ops.h")).read()
    assert "clo_segfsum.h" in open(os.path.join(ROOT, "include", "clo_segreduce.h")).read()     # the pointer from where floats are refused
    for n in ("SegFSum", "segfsum_tile", "SEGFSUM_PAIRS"):
        assert getattr(clo, n) is not None and n in clo.__all__
    assert clo.SEGFSUM_PAIRS == PAIRS and FORMS == clo.SEGREDUCE_FORMS
    assert "segmented-float-sum" in clo.__doc__


def test_the_driver_stands_on_the_shared_host_layer():
    """The rules tests/test_op_host_cpu.py keeps for the drivers it lists."""
    text = open(os.path.join(ROOT, "cl_ops_amd", "csrc", "clo_segfsum.c")).read()
    assert not re.search(r"^static[^;{]*\w(_overlap|_key_kind|_value_type_ok|_index)\(", text, re.M)
    for word in ("intern_queue", "error_handler:", "ccl_queue_new(", "ccl_buffer_new(", "calloc(", "clo_stream_guard_enter("):
        assert word not in text, word
    assert "clo_op_head head;" in text and "clo_stage_close(" in text


def test_tile_and_workspace_getters():
    sizes = {np.dtype(NP[v]).itemsize for v in NP}
    for vs in (0, 1, 2, 3, 4, 5, 8, 12, 16, -1, -4):
        for ss in (0, 1, 2, 3, 4, 8, 16, -8):
            built = (vs, ss) in {(np.dtype(NP[v]).itemsize, np.dtype(NP[s]).itemsize) for v, s in PAIRS}
            assert clo.segfsum_tile(vs, ss) == (T if built else 0), (vs, ss)
    assert clo.segfsum_tile() == T == 4352 and sizes == {2, 4, 8}
    ws = clo.api.lib.clo_hip_segfsum_workspace_bytes
    sizes = (0, 1, 63, T, T + 1, 1 << 20, (1 << 32) - 1)
    assert ws(0, 0) == 0
    for a in sizes:
        col = [ws(a, c) for c in sizes]
        row = [ws(n, a) for n in sizes]
        assert col == sorted(col) and row == sorted(row), (a, col, row)       # monotone in both arguments
        assert all(s % 256 == 0 for s in col + row)
        for c in sizes:
            # 8 bytes per segment (the ends) plus, per tile of merge steps, a split, two words and a 64-bit word
            assert ws(a, c) >= 8 * a + 20 * -(-(a + c) // T), (a, c)
            assert ws(a, c) == clo.api.lib.clo_hip_segreduce_workspace_bytes(a, c)   # the schedule is CloSegReduce's


def _refused(call):
    with pytest.raises(clo.CloError) as e:
        call()
    assert e.value.code == CLO_ERROR_ARGS, e.value
    return e.value.message


def test_refusals_through_an_offline_context():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    F, D, H, U = (clo.CLO_TYPES[t] for t in ("float", "double", "half", "uint"))
    try:
        for form in ("", "lengths", "Counts", "count", "offsets ", None):
            assert "form" in _refused(lambda: clo.SegFSum(form, ctx))
            assert not lib.clo_segfsum_new(form.encode() if form is not None else None, None, ctx.h, F, F, U, None)   # err NULL
        for opt in ("tile=4096", "sorted", " "):
            assert "options" in _refused(lambda: clo.SegFSum("counts", ctx, options=opt))
            assert not lib.clo_segfsum_new(b"counts", opt.encode(), ctx.h, F, F, U, None)
        for ct in ("char", "uchar", "short", "ushort", "int", "long", "half", "float", "double"):
            assert "count_type" in _refused(lambda: clo.SegFSum("counts", ctx, count_type=ct))
            assert not lib.clo_segfsum_new(b"offsets", None, ctx.h, F, F, clo.CLO_TYPES[ct], None)
        ints = ("char", "uchar", "short", "ushort", "int", "uint", "long", "ulong")
        for t in ints:                                                        # integers: the message points to CloSegReduce
            for vt, st in ((t, "float"), ("float", t), (t, t), (t, "double")):
                assert "CloSegReduce" in _refused(lambda: clo.SegFSum("counts", ctx, vt, st))
                assert not lib.clo_segfsum_new(b"counts", None, ctx.h, clo.CLO_TYPES[vt], clo.CLO_TYPES[st], U, None)
        for vt in ("half", "float", "double"):                                # half sums
            assert "half sums" in _refused(lambda: clo.SegFSum("counts", ctx, vt, "half"))
            assert not lib.clo_segfsum_new(b"counts", None, ctx.h, clo.CLO_TYPES[vt], H, U, None)
        assert "narrower" in _refused(lambda: clo.SegFSum("counts", ctx, "double", "float"))
        assert not lib.clo_segfsum_new(b"counts", None, ctx.h, D, F, U, None)
        assert "not built" in _refused(lambda: clo.SegFSum("counts", ctx, "half", "double"))
        assert not lib.clo_segfsum_new(b"counts", None, ctx.h, H, D, U, None)
        assert not lib.clo_segfsum_new(b"counts", None, ctx.h, 11, F, U, None)       # no such type
        assert not lib.clo_segfsum_new(b"counts", None, ctx.h, F, 11, U, None)
        assert not lib.clo_segfsum_new(b"counts", None, None, F, F, U, None)         # no context
        for form in FORMS:                                                    # every form, pair, count type, both spellings of no options
            for vt, st in PAIRS:
                for ct, opt in (("uint", None), ("ulong", "")):
                    s = clo.SegFSum(form, ctx, vt, st, ct, options=opt)
                    assert (s.form, s.value_type, s.value_size, s.sum_type, s.sum_size, s.count_type, s.count_size) == \
                        (form, clo.CLO_TYPES[vt], np.dtype(NP[vt]).itemsize, clo.CLO_TYPES[st], np.dtype(NP[st]).itemsize, clo.CLO_TYPES[ct],
                         4 if ct == "uint" else 8)
                    s.close()
        assert clo.SegFSum("counts", ctx, "double").sum_type == D             # sum_type None: the value type

        c4, o4 = clo.SegFSum("counts", ctx), clo.SegFSum("offsets", ctx, "half", "float")
        c8 = clo.SegFSum("counts", ctx, "float", "double", "ulong")
        cn, of = np.zeros(16, np.uint32), np.zeros(17, np.uint32)
        cn8 = np.zeros(16, np.uint64)
        vi = np.zeros(16, np.uint32)
        so = np.arange(100, 116, dtype=np.uint32)
        so8 = np.arange(400, 416, dtype=np.uint64)
        num = np.full(2, 777, np.uint64)
        nin = np.full(1, 16, np.uint64)
        p = lambda x: x.ctypes.data if x is not None else None
        sp = lambda x: C.cast(p(x), C.POINTER(C.c_size_t))

        def host(obj, src, n_in, vals, out, m_h=16, n=16, out_n=num, with_err=True):
            err = clo.api._Err()
            ok = lib.clo_segfsum_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out), sp(out_n), m_h, n, err.ref if with_err else None)
            assert not ok
            if with_err:
                return _refused(err.raise_if_set)

        def both(word, *args, **kw):
            assert word in host(*args, **kw), (word, args)
            host(*args, with_err=False, **kw)

        both("numel_seg", c4, cn, None, vi, so, m_h=1 << 32)
        both("numel_seg", o4, of, nin, vi, so, m_h=(1 << 32) + 5)
        both("numel must", c4, cn, None, vi, so, n=1 << 32)
        both("numel must", c8, cn8, None, vi, so8, n=1 << 63)
        both("the counts", c4, None, None, vi, so)                            # NULL counts_or_offsets
        both("the offsets", o4, None, None, vi, so)
        both("the offsets", o4, None, None, None, None, m_h=0, n=0)           # ... in the offsets form always
        both("values_in", c4, cn, None, None, so)
        both("values_in", c4, None, None, None, None, m_h=0, n=3)             # ... even without a segment
        both("sums_out", c4, cn, None, vi, None)
        both("sums_out", c8, cn8, nin, None, None, n=0)
        both("num_out", c4, cn, None, vi, so, out_n=None)
        both("num_out", o4, of, nin, vi, so, out_n=None)

        # overlap: sums_out (sized by numel_seg rows) on, inside, across the end of, sharing one element with an input or
        # num_in; num_out on each array and on num_in
        one = np.zeros(200, np.uint32)
        n8 = lambda a, b: one[a:b].view(np.uint64)
        O = "overlap"
        both(O, c4, cn, None, vi, cn)                                         # sums_out on the counts
        both(O, c4, one[0:32], None, vi, one[8:24], m_h=32)                   # sums_out inside the counts
        both(O, c4, one[0:16], None, vi, one[8:24])                           # across the counts' end
        both(O, c4, one[0:16], None, vi, one[15:31])                          # one shared element
        both(O, o4, one[0:17], None, vi, one[16:32])                          # on the 17th offset
        both(O, c4, cn, n8(40, 42), vi, one[41:57])                           # on num_in's second half
        both(O, c4, cn, None, one[0:16], one[15:31])                          # on values_in's last row
        both(O, c4, cn, None, one[0:64], one[63:79], n=64)                    # ... sized by numel, not numel_seg
        both(O, o4, of, None, one[0:8], one[7:23])                            # ... of half rows: 16 of them end inside one[7]
        both(O, c4, cn, None, one[0:16], one[0:16])                           # sums_out on values_in
        both(O, c8, cn8, None, vi, n8(0, 32), out_n=n8(30, 32))               # num_out on sums_out's last row (8-byte rows)
        both(O, c4, cn, None, vi, one[0:16], out_n=n8(0, 2))                  # num_out on sums_out's first rows
        both(O, c4, one[0:16], None, vi, so, out_n=n8(14, 16))                # num_out on the counts
        both(O, c4, cn, None, one[0:16], so, out_n=n8(2, 4))                  # num_out on values_in
        both(O, c4, cn, n8(20, 22), vi, so, out_n=n8(20, 22))                 # num_out on num_in
        assert np.array_equal(so, np.arange(100, 116)) and np.array_equal(so8, np.arange(400, 416))
        assert not one.any() and not cn.any() and not of.any() and not vi.any() and (num == 777).all() and nin[0] == 16

        # what lies next to another range without touching it is accepted as far as the checks go: the call then fails
        # for want of a device, not with CLO_ERROR_ARGS (the counts are ones: m == 0 would need no device)
        one[:] = 1
        out_n = n8(190, 192)
        for obj, args in ((c4, (one[0:16], None, one[16:32], one[32:48])),
                          (c4, (one[0:16], n8(16, 18), one[18:34], one[34:50])),
                          (o4, (one[0:17], None, one[17:25], one[25:41])),
                          (o4, (one[0:17], n8(18, 20), one[20:28], one[28:44]))):
            err = clo.api._Err()
            src, n_in, vals, out = args
            assert not lib.clo_segfsum_with_host_data(obj.h, None, None, p(src), sp(n_in), p(vals), p(out), sp(out_n), 16, 16, err.ref)
            with pytest.raises(clo.CloError) as e:
                err.raise_if_set()
            assert e.value.domain == "ccl-hip-error-quark", (obj.form, e.value)
        assert (one[:190] == 1).all()

        # the Python view checks the element types
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint64), np.zeros(4, np.float32))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.float64))
        with pytest.raises(ValueError):
            c4.with_host_data(np.zeros(4, np.uint32), np.zeros(4, np.uint32))
        with pytest.raises(ValueError):
            o4.with_host_data(np.zeros(0, np.uint32), np.zeros(4, np.float16))
        for s in (c4, o4, c8):
            s.close()
    finally:
        ctx.close()


def test_no_segments_without_a_device():
    ctx = clo.Context(offline=True)
    lib = clo.api.lib
    try:
        for form in FORMS:
            for (vt, st), (ct, cdt) in zip(PAIRS, (("uint", np.uint32), ("ulong", np.uint64)) * 2):
                s = clo.SegFSum(form, ctx, vt, st, ct)
                src = np.zeros(1 if form == "offsets" else 0, cdt)
                a, total = s.with_host_data(src, np.arange(5, dtype=NP[vt]))   # rows, but no segment to put them in
                assert total == 0 and a.size == 0 and a.dtype == NP[st]
                src = np.arange(1, 6, dtype=cdt)                              # four or five segments, of which num_in takes none
                a, total = s.with_host_data(src, np.arange(20, dtype=NP[vt]), num_in=0)
                assert total == 0 and a.size == 0
                # raw: num_out becomes 0, sums_out is not touched
                out, num = np.full(5, 7, NP[st]), C.c_size_t(55)
                zero = C.c_size_t(0)
                vals = np.zeros(20, NP[vt])
                err = clo.api._Err()
                assert lib.clo_segfsum_with_host_data(s.h, None, None, src.ctypes.data, C.byref(zero), vals.ctypes.data,
                                                      out.ctypes.data, C.byref(num), 4, 20, err.ref)
                err.raise_if_set()
                assert num.value == 0 and (out == 7).all()
                s.close()
    finally:
        ctx.close()


def test_driver_under_sanitizers(tmp_path):
    exe = str(tmp_path / "segfsum_host")
    srcs = (sorted(glob.glob(os.path.join(ROOT, "cl_ops_amd", "csrc", "*.c"))) +
            sorted(glob.glob(os.path.join(ROOT, "tests", "hoststub", "*stub*.c"))) +
            [os.path.join(ROOT, "tests", "segfsum_host", "segfsum_host_test.c")])
    subprocess.check_call(["gcc", "-O1", "-g", "-std=c11", "-D_GNU_SOURCE", "-fno-omit-frame-pointer", "-w",
                           "-fsanitize=address,undefined", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "cl_ops_amd", "csrc"), *srcs, "-lpthread", "-lm", "-o", exe])
    env = dict(os.environ, CLO_NO_WARMUP="1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and r.stdout.count("segfsum host ok") == 1, out[-4000:]
    for n in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert n not in out, out[-4000:]


# ---- the model ----

def _cases():
    """Every layout at every row count of the GPU tests, both forms, num_in as the layout has it."""
    for n in M.ROWS:
        for name in M.LAYOUTS:
            counts, num_in = M.layout(name, n)
            yield n, name, counts, num_in


def test_the_models_tree_is_segreduces_sum_on_integers():
    """With uint32 in place of the sum type every order gives the same wrapped sums: the tree must give
    segreduce_model's sum bit for bit, which pins which row reaches which segment independently of floating point."""
    for n, name, counts, num_in in _cases():
        v = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint32)
        for form, cdt in zip(FORMS, (np.uint32, np.uint64)):
            src = M.source(form, counts, cdt, base=77)
            got, total = segfsum(form, src, v, np.uint32, num_in)
            want, total2 = segreduce("sum", form, src, v, "uint", num_in)
            assert got.dtype == np.uint32 and np.array_equal(got, want) and total == total2, (n, name, form)
    # ... and across the threads, the waves and the trips of the carry scan
    rng = np.random.default_rng(1)
    for tiles in (17, 1025, 2 * M.CARRY_TRIP + 108):
        steps = tiles * T
        counts = np.array([5, 0, steps // 2, 9, steps - steps // 2 - 300, 7], np.uint64)
        n = int(counts.sum())
        v = rng.integers(0, 1 << 32, n, dtype=np.uint32)
        got, _ = segfsum("counts", counts, v, np.uint32)
        want, _ = segreduce("sum", "counts", counts, v, "uint")
        assert np.array_equal(got, want), tiles


def test_telescoping_inputs_give_the_exact_sums():
    for vt, st in PAIRS:
        for n, name, counts, num_in in _cases():
            v = M.telescoping(vt, st, n)
            got, _ = segfsum("counts", counts, v, st, num_in)
            c, _ = M.clipped_ends("counts", counts, n, num_in)
            exact = [sum(int(x) for x in v[a:b]) for a, b in zip(np.concatenate(([0], c[:-1])), c)]
            assert same_bits(got, np.array(exact, np.float64).astype(NP[st]) + NP[st](0)), (vt, st, n, name)


def _within_bound(got, v, c, st, tiles):
    u = 2.0 ** (-24 if st == "float" else -53)
    D = M.depth(tiles)
    gamma = D * u / (1 - D * u)
    x = v.astype(np.float64)
    for r, (a, b) in enumerate(zip(np.concatenate(([0], c[:-1])), c)):
        assert abs(float(got[r]) - math.fsum(x[a:b])) <= gamma * float(np.abs(x[a:b]).sum()), (st, r, a, b)


def test_rounding_and_mixed_inputs_stay_within_the_bound_of_fsum():
    assert M.depth(1) == 43 and M.depth(2) == 69 and M.depth(4096) == 69 and M.depth(4097) == 73 and M.depth(2 * 4096 + 108) == 77
    for vt, st in PAIRS:
        for n in (1089, 2 * T + 5):
            for name in ("one", "geometric", "three_tiles", "tile_edges"):
                counts, num_in = M.layout(name, n)
                c, _ = M.clipped_ends("counts", counts, n, num_in)
                for v in (M.rounding(vt, n), M.mixed(vt, n)):
                    got, _ = segfsum("counts", counts, v, st, num_in)
                    _within_bound(got, v, c, st, -(-(c.size + n) // T))
    n = 40 * T                                                                # the carry scan
    v = M.rounding("float", n)
    for st in ("float", "double"):
        counts = np.array([7, n - 20, 13], np.uint64)
        got, _ = segfsum("counts", counts, v, st)
        _within_bound(got, v, np.cumsum(counts).astype(np.int64), st, 41)


# six deliberately different stages

def _pairwise_lane_walk(close, x):
    """A lane without a close adds its 17 rows pairwise; the others as they were."""
    h, a = M.lane_walk(close, x)
    parts = [x[k] for k in range(M.ITEMS)]
    while len(parts) > 1:
        parts = [parts[i] + parts[i + 1] for i in range(0, len(parts) - 1, 2)] + ([parts[-1]] if len(parts) % 2 else [])
    return h, np.where(h, a, parts[0])


def _swapped_network(h, a):
    return M.network(h, a, M.NETWORK[:4] + ("bcast31", "bcast15"))


def _paired_waves(th, ta, run_h=None, run_a=None):
    """before and all as left to right, but the tile's state as (w0 + w1) + (w2 + w3)."""
    bh, ba, all_h, all_a = M.waves(th, ta, run_h, run_a)
    lh, la = M.combine(th[:, 0], ta[:, 0], th[:, 1], ta[:, 1])
    rh, ra = M.combine(th[:, 2], ta[:, 2], th[:, 3], ta[:, 3])
    all_h, all_a = M.combine(lh, la, rh, ra)
    return bh, ba, all_h, all_a


def _right_to_left_thread(sh, sa):
    h, a = sh[:, -1], sa[:, -1]
    for j in range(M.CARRY_ITEMS - 2, -1, -1):
        h, a = M.combine(sh[:, j], sa[:, j], h, a)
    return h, a


def _running_last(th, ta, run_h, run_a):
    """The waves left to right from (0, +0), the running state of the trips before added last."""
    bh, ba, all_h, all_a = M.waves(th, ta)
    bh, ba = M.combine(run_h[:, None], run_a[:, None], bh, ba)
    all_h, all_a = M.combine(run_h, run_a, all_h, all_a)
    return bh, ba, all_h, all_a


def _no_fixup(sums, first, carries):
    return sums


MUTANTS = (("a lane adds pairwise", {"lane_walk": _pairwise_lane_walk}),
           ("the network's last two steps swapped", {"network": _swapped_network}),
           ("the waves grouped (w0 + w1) + (w2 + w3)", {"waves": _paired_waves}),
           ("the carry's 16 states per thread right to left", {"carry_thread": _right_to_left_thread}),
           ("the running state of a trip added last", {"carry_waves": _running_last}),
           ("the fix-up dropped", {"fixup": _no_fixup}))


def test_every_different_stage_changes_a_bit_on_the_committed_inputs():
    """The inputs of the GPU tests tell the tree from six near misses: on rounding rows (segfsum_model.ROUNDING_SEED), the
    shapes of test_gpu_segfsum.py's carry tests — a segment across 16 + 1 and 1024 + 1 tiles — and, for the running
    state, the tile states of (2 * 4096 + 108) tiles given to the carry scan alone. On integers the swapped network and the
    dropped fix-up lose rows; the other four change nothing there: they are other orders of the same rows."""
    shown = {}
    for tiles in (17, 1025):
        n = tiles * T - 1
        counts = np.array([n], np.uint64)
        for vt, st in (("float", "float"), ("float", "double")):
            v = M.rows_for(vt, st, n)
            ref, _ = segfsum("counts", counts, v, st)
            for name, stages in MUTANTS:
                got, _ = segfsum("counts", counts, v, st, stages=stages)
                shown[name] = shown.get(name, False) or not same_bits(got, ref)
        vi = np.random.default_rng(tiles).integers(0, 1 << 32, n, dtype=np.uint32)
        ref, _ = segfsum("counts", counts, vi, np.uint32)
        for k, (name, stages) in enumerate(MUTANTS):
            assert np.array_equal(segfsum("counts", counts, vi, np.uint32, stages=stages)[0], ref) == (k in (0, 2, 3, 4)), name
    # the trips: open sums only, so that the running state crosses two trip edges
    tiles = 2 * M.CARRY_TRIP + 108
    for st in ("float", "double"):
        ta = M.rounding(st, tiles)
        th = np.zeros(tiles, bool)
        ref = M.carry(th, ta)
        for name, stages in MUTANTS[3:5]:
            shown[name] = shown.get(name, False) or not same_bits(M.carry(th, ta, stages), ref)
        assert same_bits(M.carry(th, ta, MUTANTS[4][1])[:M.CARRY_TRIP], ref[:M.CARRY_TRIP])      # the first trip has no running state
    assert all(shown.get(name) for name, _ in MUTANTS), shown
