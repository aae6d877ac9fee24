"""CloSegScan (include/clo_segscan.h) on the GPU against the numpy model of tests/segscan_model.py, bit for bit. Every
array is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); data_out and num_out are pre-filled with the pattern, and after every call num_out is the model's
unclamped total, the rows below ct = min(total, n) equal the model's, and the guards, every input and every row at index
>= ct are unchanged. With T = clo_hip_segscan_tile, the merge steps (segment ends plus rows) of a tile: row counts and
m + n around the tile edges x count patterns; all segments empty, runs of 4 T + 5 and of 2^20 empty segments; totals above
and below n; num_in below, at and above; both forms, both count types, rebased offsets and uint offsets that end at
2^32 - 1; every legal (value, sum) pair x the three ops x both kinds on values at the types' extremes; in place for each
sum size; cross-checks against scan by key on CloExpand's segment ids, against CloSegReduce through the last row of every
segment, and a chain behind reduce by key without a host wait; element-aligned views, two queues, the host form, the thin
ABI's status codes, a captured graph replayed on other counts and values; offsets that do not ascend and sums that wrap
(in bounds, contents not compared); rows above 2^31 against a closed form; and open values carried across and through
whole trips of the one-group carry scan (about 36 M rows)."""
import ctypes as C

import numpy as np
import pytest

from segscan_model import FORMS, NP, OPS, PAIRS, identity, merge_steps, segscan
from segreduce_model import segreduce
from test_gpu_histogram import Region
from test_gpu_segreduce import CARRY_LAYOUTS, CARRY_TRIP, carry_layout, counts_of, source, values_for

pytestmark = pytest.mark.gpu

CDT = {"uint": np.uint32, "ulong": np.uint64}


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def T(dev):
    clo = dev[0]
    t = clo.segscan_tile(4, 4)
    assert t >= 1024 and all(clo.segscan_tile(v, s) == t for v, s in ((4, 8), (8, 8)))
    assert t == clo.segreduce_tile(4, 4)                                      # the layouts borrowed from test_gpu_segreduce.py are in these steps
    return t


def run_scan(dev, op, incl, form, ct, vt, st, counts, n, what, num_in=None, base=0, offs=(0, 0, 0), obj=None, q=None, src=None, compare=True, seed=0,
             vals=None, in_place=False):
    """One call on views at byte offsets offs = (counts_or_offsets, values_in, data_out) with n rows of values; checks
    everything and returns (total, data). src: the input as it is (broken preconditions); compare False: the rows'
    contents are not compared; vals: the n values, instead of values_for(vt, n, seed); in_place: data_out is values_in."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = source(form, ct, counts, base)
    m_h = src.size - (1 if form == "offsets" else 0)
    if vals is None:
        vals = values_for(vt, n, seed)
    assert vals.dtype == NP[vt] and vals.size == n
    data, total = segscan(op, form, src, vals, st, incl, num_in) if compare else (None, None)
    what = "%s %s %s %s %s->%s n %d%s, %s" % ("inclusive" if incl else "exclusive", op, form, ct, vt, st, n, " in place" if in_place else "", what)
    ss = np.dtype(NP[st]).itemsize
    sc = obj or clo.SegScan(op, form, ctx, vt, st, ct, inclusive=incl)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0) if src.size else None
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if n else None
    d_r = v_r if in_place else Region(rdev, n * ss, offs[2], None, 2) if n else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert sc.with_device_data(q, view(s_r), view(n_r), view(v_r), view(d_r), num_r.view, m_h, n), what
        q.finish()
        got = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        if compare:
            assert got == total, "%s: num_out = %d, the model's total is %d" % (what, got, total)
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            if d_r:
                now = d_r.base.read(q, np.uint8, d_r.host.size)[d_r.at:d_r.at + data.nbytes].copy().view(NP[st])
                bad = np.flatnonzero(now != data)
                assert bad.size == 0, "%s: %d of %d rows differ, first %d: %r, the model has %r" % (
                    what, bad.size, data.size, bad[0], now[bad[0]], data[bad[0]])
                d_r.check(data, what + ": data_out")                        # ... and nothing behind the ct rows written
        elif d_r:                                                          # in bounds: the guards
            now = d_r.base.read(q, np.uint8, d_r.host.size)
            d_r.check(now[d_r.at:d_r.at + n * ss], what)
        if s_r:
            s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if v_r and not in_place:
            v_r.check(vals, what + ": values_in")
        return got, data
    finally:
        for r in (s_r, n_r, v_r, None if in_place else d_r, num_r):
            if r:
                r.close()
        if obj is None:
            sc.close()


PATTERNS = ("ones", "one segment", "geometric", "alternating 0 and 3", "long between ones", "an end on every tile edge")


def rotate(case):
    """An op, a kind, a form, a count type and a type pair for case number `case`: every one of them meets every pattern."""
    return OPS[case % 3], bool(case // 3 % 2), FORMS[case // 6 % 2], ("uint", "ulong")[case // 12 % 2], PAIRS[case % len(PAIRS)]


def test_sizes_and_count_patterns(dev, T):
    """Row counts around the wave, the work-group and the tile x the count patterns: all ones, a single segment,
    geometric lengths of mean 16, half of the segments empty, a segment across three tiles (the carry passes through a
    tile in which nothing closes), an end on the last and on the first step of every tile."""
    case = 0
    for n in (0, 1, 63, 64, 255, 256, T - 1, T, T + 1, 2 * T + 1, 3 * T + 5):
        for pattern in PATTERNS:
            op, incl, form, ct, (vt, st) = rotate(case)
            case += 1
            counts = counts_of(pattern, n, T, case)
            if pattern == "long between ones" and n >= 3 * T + 5:
                close, _, _ = merge_steps("counts", counts, n)
                assert (np.bincount(close // T)[1:-1] == 0).any()             # a tile without a close between tiles with rows
            got, _ = run_scan(dev, op, incl, form, ct, vt, st, counts, n, "%s" % pattern, base=case * 1000, seed=case)
            assert got == n


def test_merge_lengths_around_the_tile_edges(dev, T):
    """m + n, the number of merge steps, one below, on and one above one, two and three tiles' length, with few long, as
    many and many short segments."""
    case = 0
    for steps in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T - 1, 3 * T, 3 * T + 1):
        for m in (3, steps // 2, steps - 5):
            n = steps - m
            counts = np.full(m, n // m, np.int64)
            counts[:n % m] += 1
            op, incl, form, ct, (vt, st) = rotate(case)
            case += 1
            got, _ = run_scan(dev, op, incl, form, ct, vt, st, counts, n, "%d segments + %d rows" % (m, n), seed=case)
            assert got == n


@pytest.fixture(scope="module")
def carry_cases(T):
    """The two layouts of test_gpu_segreduce.py and one array of values per value type, shared by the cases: in every
    long segment the type's minimum and maximum are planted within the first T / 2 rows, before the trip edge, so that a
    running value that loses what was carried in is wrong from there to the segment's end."""
    layouts = {name: carry_layout(T, name) for name in CARRY_LAYOUTS}
    rows = max(int(c.sum()) for c, _ in layouts.values())
    vals = {vt: values_for(vt, rows, 70) for vt in ("int", "uint")}
    for vt, v in vals.items():
        info = np.iinfo(NP[vt])
        for _, longs in layouts.values():
            for _, row, length, _, _ in longs:
                assert length > T // 2
                v[row + 5], v[row + T // 4] = info.min, info.max
    return layouts, vals


@pytest.mark.parametrize("case", range(4))
@pytest.mark.parametrize("layout", CARRY_LAYOUTS)
def test_open_values_cross_the_trips_of_the_carry_scan(dev, T, carry_cases, layout, case):
    """m + n = (2 * 4096 + 108) T merge steps, three trips of the one-group carry scan. Layout 1: short segments, one
    segment over the steps [4096 T - 2.5 T, 4096 T + 2.5 T) and one over [8192 T - T / 2, 8192 T + T / 2): an open value is
    carried from one trip into the next. Layout 2: one segment from step 100 T + 7 to step 8292 T - 9: the whole second
    trip holds no segment end and the carried state passes through it unchanged."""
    op, vt, st, incl = (("sum", "int", "long", True), ("sum", "uint", "uint", False), ("min", "int", "int", False), ("max", "uint", "uint", True))[case]
    layouts, vals = carry_cases
    counts, longs = layouts[layout]
    m, n = counts.size, int(counts.sum())
    E = CARRY_TRIP * T
    assert m + n == 2 * E + 108 * T
    if layout == CARRY_LAYOUTS[0]:                                        # the segments lie where the docstring says
        assert [(first, steps) for _, _, _, first, steps in longs] == [(E - 5 * T // 2, 5 * T), (2 * E - T // 2, T)]
    else:
        (_, _, _, first, steps), = longs
        assert (first, first + steps) == (100 * T + 7, 2 * E + 100 * T - 9) and first < E and first + steps > 2 * E + T
    k = case + CARRY_LAYOUTS.index(layout)
    got, data = run_scan(dev, op, incl, FORMS[k % 2], ("uint", "ulong")[k // 2 % 2], vt, st, counts, n, layout, base=7 * k, vals=vals[vt][:n])
    assert got == n
    info = np.iinfo(NP[vt])
    for seg, row, length, _, _ in longs:
        if op != "sum":                                                       # from the planted extreme to the segment's end
            assert (data[row + T // 4 + 1:row + length] == (info.min if op == "min" else info.max)).all(), (layout, op, seg)


def test_empty_segments(dev, T):
    case = 0
    for m in (1, 5, T, 2 * T + 1):                                        # nothing but empty segments, without and with rows nobody owns
        for n in (0, 7, T + 3):
            op, incl, form, ct, (vt, st) = rotate(case)
            case += 1
            got, data = run_scan(dev, op, incl, form, ct, vt, st, np.zeros(m, np.int64), n, "%d empty segments" % m, seed=case)
            assert got == 0 and data.size == 0
    counts = np.concatenate((np.full(9, T // 4 + 1), np.zeros(4 * T + 5, np.int64), np.full(9, T // 4 + 1)))
    for op in OPS:
        for incl, form, ct in ((False, "counts", "ulong"), (True, "offsets", "uint")):
            run_scan(dev, op, incl, form, ct, "int", "long", counts, int(counts.sum()), "4 T + 5 empty segments between rows", seed=3)
    counts = np.concatenate(([1], np.zeros(4 * T + 5, np.int64), [1]))
    for op, incl in (("sum", True), ("min", False), ("max", False)):
        run_scan(dev, op, incl, "counts", "uint", "int", "int", counts, 2, "4 T + 5 empty segments between two rows", seed=4)


def test_a_million_empty_segments_take_bounded_work(dev, T):
    """2^20 empty segments at one position, between rows: a tile is T merge steps whatever they are, so this is 2^20 / T
    more tiles of the same work, not one work-group that walks 2^20 ends."""
    counts = np.concatenate((np.full(5, 700), np.zeros(1 << 20, np.int64), np.full(5, 900), np.zeros(3, np.int64)))
    for op, incl, form in (("sum", False, "counts"), ("min", True, "offsets"), ("max", False, "counts")):
        got, _ = run_scan(dev, op, incl, form, "uint", "int", "int", counts, 8000, "2^20 empty segments", seed=4)
        assert got == 8000


def test_totals_above_and_below_the_rows(dev, T):
    """num_out always receives the unclamped total. Above: a segment cut by n scans the rows it has. Below: the rows at
    and beyond the total keep what they held."""
    case = 0
    for total in (T + 1, 3 * T + 11):
        for pattern in ("geometric", "long between ones", "one segment"):
            counts = counts_of(pattern, total, T, 7)
            for n in (0, 1, total // 2, total - 3, total - 1, total + 1, total + T + 9, total + 2 * T + 1):
                op, incl, form, ct, (vt, st) = rotate(case)
                case += 1
                got, data = run_scan(dev, op, incl, form, ct, vt, st, counts, n, "%s, total %d" % (pattern, total), seed=case)
                assert got == total and data.size == min(total, n)


def test_num_in(dev, T):
    counts = counts_of("geometric", 3 * T + 9, T, 6)
    counts[::6] = 0
    m_h = counts.size
    for i, num_in in enumerate((0, 1, m_h // 2, m_h - 1, m_h, m_h + 1, 1 << 40)):
        for form in FORMS:
            want = int(counts[:min(num_in, m_h)].sum())
            got, data = run_scan(dev, OPS[i % 3], bool(i % 2), form, ("uint", "ulong")[i % 2], "uint", "ulong", counts, 3 * T + 9,
                                 "num_in %d of %d" % (num_in, m_h), num_in=num_in, base=5 * i, seed=i)
            assert got == want and data.size == want


@pytest.mark.parametrize("ct", ["uint", "ulong"])
@pytest.mark.parametrize("form", FORMS)
def test_forms_and_types(dev, T, form, ct):
    """Both forms x both count types x every legal (value, sum) pair x the three ops x both kinds, empty segments among
    the others. The sums wrap; signed min and max go through the flip, and the exclusive heads hold the identity."""
    counts = counts_of("geometric", 2 * T + 3, T, 5)
    counts[::7] = 0
    heads = np.cumsum(counts)[:-1][counts[1:] > 0]
    for i, (vt, st) in enumerate(PAIRS):
        vals = values_for(vt, 2 * T + 3, i)
        if np.dtype(NP[st]).itemsize == np.dtype(NP[vt]).itemsize:
            wide = np.add.reduceat(vals.astype(np.float64), np.concatenate(([0], heads)))
            assert (np.abs(wide) > float(np.iinfo(NP[st]).max)).any()         # a segment's sum leaves the sum type: it wraps
        for op in OPS:
            for incl in (False, True):
                _, data = run_scan(dev, op, incl, form, ct, vt, st, counts, 2 * T + 3, "every type", base=3, vals=vals)
                if not incl:
                    assert (data[heads] == identity(op, st)).all() and data[0] == identity(op, st)


def test_offsets_with_a_base(dev, T):
    counts = counts_of("geometric", 2 * T + 100, T, 8)
    total = int(counts.sum())
    run_scan(dev, "sum", True, "offsets", "uint", "int", "long", counts, total, "offsets[0] = 12345", base=12345)
    run_scan(dev, "min", False, "offsets", "ulong", "int", "int", counts, total, "offsets[0] = 2^40 + 12345", base=(1 << 40) + 12345)
    src = source("offsets", "uint", counts, (1 << 32) - 1 - total)
    assert int(src[-1]) == (1 << 32) - 1
    run_scan(dev, "max", True, "offsets", "uint", "uint", "uint", counts, total, "uint offsets that end at 2^32 - 1", src=src)


def test_in_place(dev, T):
    """data_out is values_in, for each sum size, every op and kind: rows below ct hold the result, the rows at and beyond
    the total their values."""
    counts = counts_of("geometric", 3 * T + 21, T, 12)
    counts[::5] = 0
    total = int(counts.sum())
    case = 0
    for vt, st in (("uint", "uint"), ("int", "uint"), ("long", "long"), ("ulong", "long")):
        for op in OPS:
            for incl in (False, True):
                for n in (total, total - 7, total + T + 3):
                    run_scan(dev, op, incl, FORMS[case % 2], ("uint", "ulong")[case // 2 % 2], vt, st, counts, n, "in place", seed=case, in_place=True,
                             offs=(0, (0, 4, 8)[case % 3] if vt in ("uint", "int") else (0, 8)[case % 2], 0))
                    case += 1
    counts = counts_of("long between ones", 3 * T + 5, T, 1)              # a tile that only reads before another group writes
    run_scan(dev, "sum", True, "counts", "uint", "uint", "uint", counts, 3 * T + 5, "in place, a long segment", in_place=True)


def test_against_scan_by_key_on_expanded_segment_ids(dev, T):
    """Scan by key on CloExpand's seg_out computes the same rows: the composition this operation replaces."""
    clo, ctx, q = dev
    counts = counts_of("geometric", 3 * T + 50, T, 21)
    counts[::4] = 0
    m, n = counts.size, int(counts.sum())
    for op in OPS:
        for incl, (vt, st) in ((False, ("int", "long")), (True, ("uint", "uint")), (False, ("long", "ulong"))):
            vals = values_for(vt, n, 21)
            ss = np.dtype(NP[st]).itemsize
            c_r, v_r = Region(dev, 4 * m, 0, counts.astype(np.uint32), 0), Region(dev, vals.nbytes, 0, vals, 1)
            seg_r, n1_r, d1_r = Region(dev, 4 * n, 0, None, 2), Region(dev, 8, 0, None, 0), Region(dev, ss * n, 0, None, 1)
            d2_r, n2_r = Region(dev, ss * n, 0, None, 2), Region(dev, 8, 0, None, 0)
            ex, sbk, sc = clo.Expand("counts", ctx, None, "uint"), clo.ScanByKey(ctx, "uint", vt, st, op, incl), clo.SegScan(op, "counts", ctx, vt, st, "uint", inclusive=incl)
            try:
                assert ex.with_device_data(q, c_r.view, None, None, None, seg_r.view, None, n1_r.view, m, n)
                assert sbk.with_device_data(q, seg_r.view, v_r.view, d1_r.view, n)
                assert sc.with_device_data(q, c_r.view, None, v_r.view, d2_r.view, n2_r.view, m, n)
                q.finish()
                n2_r.check(np.array([n], np.uint64), "num_out")
                composed = d1_r.base.read(q, np.uint8, d1_r.host.size)[d1_r.at:d1_r.at + ss * n].copy().view(NP[st])
                d2_r.check(composed, "%s %s->%s: segment scan against expand + scan by key" % (op, vt, st))
                d2_r.check(segscan(op, "counts", counts, vals, st, incl)[0], "the model")
            finally:
                for x in (c_r, v_r, seg_r, n1_r, d1_r, d2_r, n2_r, ex, sbk, sc):
                    x.close()


def test_last_rows_are_the_segment_reduction(dev, T):
    """The last row of every non-empty segment of the inclusive result is CloSegReduce's row of that segment."""
    clo, ctx, q = dev
    counts = counts_of("geometric", 3 * T + 77, T, 22)
    counts[::4] = 0
    m, n = counts.size, int(counts.sum())
    last = (np.cumsum(counts) - 1)[counts > 0]
    for op in OPS:
        for ct, vt, st in (("uint", "int", "long"), ("ulong", "uint", "uint")):
            vals = values_for(vt, n, 22)
            ss = np.dtype(NP[st]).itemsize
            c_r, v_r = Region(dev, m * np.dtype(CDT[ct]).itemsize, 0, counts.astype(CDT[ct]), 0), Region(dev, vals.nbytes, 0, vals, 1)
            d_r, n1_r, a_r, n2_r = Region(dev, ss * n, 0, None, 2), Region(dev, 8, 0, None, 0), Region(dev, ss * m, 0, None, 1), Region(dev, 8, 0, None, 2)
            sc, sr = clo.SegScan(op, "counts", ctx, vt, st, ct, inclusive=True), clo.SegReduce(op, "counts", ctx, vt, st, ct)
            try:
                assert sc.with_device_data(q, c_r.view, None, v_r.view, d_r.view, n1_r.view, m, n)
                assert sr.with_device_data(q, c_r.view, None, v_r.view, a_r.view, n2_r.view, m, n)
                q.finish()
                data = d_r.base.read(q, np.uint8, d_r.host.size)[d_r.at:d_r.at + ss * n].copy().view(NP[st])
                aggr = a_r.base.read(q, np.uint8, a_r.host.size)[a_r.at:a_r.at + ss * m].copy().view(NP[st])
                assert np.array_equal(data[last], aggr[counts > 0]), (op, ct, vt, st)
                assert np.array_equal(aggr, segreduce(op, "counts", counts, vals, st)[0])
            finally:
                for x in (c_r, v_r, d_r, n1_r, a_r, n2_r, sc, sr):
                    x.close()


def test_chain_behind_reduce_by_key(dev, T):
    """Reduce by key collapses keys into (key, run length) rows; its num_runs_out is the segment scan's num_in and its
    run lengths are the counts, numel_seg being the buffers' row count: the running maximum within every run. One queue,
    no host wait in between."""
    clo, ctx, q = dev
    n = 3 * T + 5
    keys = np.sort(np.random.default_rng(30).integers(0, 500, n).astype(np.uint32))
    vals = values_for("int", n, 30)
    k_r, v_r = Region(dev, 4 * n, 0, keys, 0), Region(dev, 4 * n, 0, vals, 1)
    rk_r, len_r, runs_r = Region(dev, 4 * n, 0, None, 0), Region(dev, 4 * n, 0, None, 1), Region(dev, 8, 0, None, 2)
    d_r, num_r = Region(dev, 8 * n, 0, None, 0), Region(dev, 8, 0, None, 1)
    rbk, sc = clo.ReduceByKey(ctx, "uint", None, "uint"), clo.SegScan("max", "counts", ctx, "int", "long", "uint", inclusive=True)
    try:
        assert rbk.with_device_data(q, k_r.view, None, rk_r.view, len_r.view, runs_r.view, n)
        assert sc.with_device_data(q, len_r.view, runs_r.view, v_r.view, d_r.view, num_r.view, n, n)
        q.finish()
        uniq, cnt = np.unique(keys, return_counts=True)
        runs_r.check(np.array([uniq.size], np.uint64), "num_runs_out")
        num_r.check(np.array([n], np.uint64), "num_out")
        d_r.check(segscan("max", "counts", cnt, vals, "long", True)[0], "the running maximum of every run")
    finally:
        for x in (k_r, v_r, rk_r, len_r, runs_r, d_r, num_r, rbk, sc):
            x.close()


def test_element_aligned_views(dev, T):
    """Every array one (or three) elements past a 16-byte boundary: nothing may assume more than the element's
    alignment."""
    counts = counts_of("geometric", 2 * T + 37, T, 9)
    counts[5:9] = 0
    n = 2 * T + 37
    cases = (("counts", "uint", "int", "int", (4, 4, 4)), ("offsets", "uint", "uint", "ulong", (12, 12, 8)), ("counts", "ulong", "long", "long", (8, 8, 8)),
             ("offsets", "ulong", "int", "long", (8, 4, 8)), ("counts", "uint", "uint", "uint", (12, 8, 12)), ("offsets", "uint", "ulong", "ulong", (4, 8, 8)))
    for i, (form, ct, vt, st, offs) in enumerate(cases):
        run_scan(dev, OPS[i % 3], bool(i % 2), form, ct, vt, st, counts, n, "views at %s" % (offs,), offs=offs, base=9, seed=i)
    counts = counts_of("one segment", 3 * T + 2, T, 0)                        # the tails' loads: every tile whole, from an odd element
    for i, (vt, st, off) in enumerate((("int", "int", 4), ("uint", "ulong", 12), ("long", "long", 8))):
        run_scan(dev, OPS[i], True, "counts", "uint", vt, st, counts, 3 * T + 2, "one segment at %d" % off, offs=(0, off, off & 8), seed=i)


def test_two_objects_on_two_queues_and_one_object_moved(dev, T):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds; then
    one object used on the first queue, the second and the first again (its workspace follows the queue)."""
    clo, ctx, _ = dev
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("sum", False, "counts", "uint", "uint", "uint"), ("min", True, "offsets", "ulong", "int", "long"))
    objs = [clo.SegScan(op, form, ctx, vt, st, ct, inclusive=incl) for op, incl, form, ct, vt, st in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (op, incl, form, ct, vt, st) in enumerate(specs):
                counts = counts_of("geometric", 40 * T + 9 + rnd, T, 10 * rnd + i)
                counts[::9] = 0
                n = int(counts.sum())
                src, vals = source(form, ct, counts, 7), values_for(vt, n, rnd)
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, src.nbytes, 0, src, 0), Region(rdev, vals.nbytes, 0, vals, 1),
                        Region(rdev, n * np.dtype(NP[st]).itemsize, 0, None, 2), Region(rdev, 8, 0, None, 0)]
                sent.append((src, vals, counts.size, n, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (src, vals, m_h, n, regs) in enumerate(sent):
                assert objs[i].with_device_data(qs[i], regs[0].view, None, regs[1].view, regs[2].view, regs[3].view, m_h, n)
            for i in range(2):
                qs[i].finish()
            for i, (src, vals, m_h, n, regs) in enumerate(sent):
                data, t = segscan(specs[i][0], specs[i][2], src, vals, specs[i][5], specs[i][1])
                what = "round %d, %s" % (rnd, specs[i][2])
                regs[3].check(np.array([t], np.uint64), what + ": num_out")
                regs[2].check(data, what + ": data_out")
                for r in regs:
                    r.close()
        for j, qi in enumerate((0, 1, 0, 1)):
            total = (5, 60, 2, 30)[j] * T + j                               # small, large, small, large
            counts = counts_of("geometric", total, T, 40 + j)
            run_scan((clo, ctx, qs[qi]), "sum", False, "counts", "uint", "uint", "uint", counts, total, "moved, call %d" % j, obj=objs[0], q=qs[qi], seed=j)
    finally:
        for x in objs + qs:
            x.close()


def test_host_data_form(dev, T):
    clo, ctx, q = dev
    counts = counts_of("geometric", 2 * T + 9, T, 11)
    counts[::5] = 0
    total, qc = int(counts.sum()), clo.Queue(ctx)
    try:
        for form in FORMS:
            for op, incl, ct, vt, st in (("sum", True, "uint", "int", "long"), ("min", False, "ulong", "uint", "uint"), ("max", True, "uint", "long", "long")):
                src = source(form, ct, counts, 4321)
                sc = clo.SegScan(op, form, ctx, vt, st, ct, inclusive=incl)
                modes = ((None, q, qc), (counts.size // 2, None, None), (counts.size + 9, q, None))   # a queue of its own: the middle one
                for k, n in enumerate((0, total - 5, total, total + 7)):                             # the modes take turns: every n meets two of them
                    vals = values_for(vt, n, n)
                    for num_in, qe, qcomm in (modes[(k + FORMS.index(form)) % 3], modes[(k + FORMS.index(form) + 1) % 3])[:1 if n == 0 else 2]:
                        data, t = segscan(op, form, src, vals, st, incl, num_in)
                        d, got = sc.with_host_data(src, vals, num_in=num_in, q_exec=qe, q_comm=qcomm, fill=77)
                        what = (form, op, incl, ct, vt, st, n, num_in)
                        assert got == t and d.dtype == data.dtype and d.size == n, what
                        assert np.array_equal(d[:data.size], data) and (d[data.size:] == 77).all(), what   # the rows beyond the total: not written
                if vt == st or (vt, st) == ("uint", "uint"):                  # in place through the host form
                    vals = values_for(vt, total, 5)
                    data, t = segscan(op, form, src, vals, st, incl)
                    buf, num = vals.copy(), C.c_size_t(0)
                    err = clo.api._Err()
                    ok = clo.api.lib.clo_segscan_with_host_data(sc.h, q.h, None, src.ctypes.data, None, buf.ctypes.data, buf.ctypes.data, C.byref(num),
                                                                counts.size, total, err.ref)
                    err.raise_if_set()
                    assert ok and num.value == t and np.array_equal(buf.view(NP[st]), data)
                sc.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev, T):
    """The table of tests/test_segscan_cpu.py (which asks it of the host stub), on device memory, and then what is asked
    for works."""
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    INT, UINT, LONG, ULONG = (clo.CLO_TYPES[t] for t in ("int", "uint", "long", "ulong"))
    m_h, n = 1000, 3 * T
    need = lib.clo_hip_segscan_workspace_bytes(m_h, n)
    assert need > 0 and need % 256 == 0
    counts = np.random.default_rng(5).integers(0, 9, 2 * m_h + 4, dtype=np.uint32)
    vals = values_for("uint", 2 * n + 4, 5)
    cn, vi, ni = Region(dev, counts.nbytes, 0, counts, 0), Region(dev, vals.nbytes, 0, vals, 1), Region(dev, 16, 0, np.array([m_h // 2, 0], np.uint64), 2)
    do, num = Region(dev, 8 * n + 16, 0, None, 0), Region(dev, 16, 0, None, 1)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(c_p, v_p, d_p, op=0, incl=0, form=0, cs=4, n_p=None, num_p=num.ptr, numel_seg=m_h, numel=n, vt=UINT, st=UINT, w=ws.ptr, wb=need):
        return lib.clo_hip_segscan(op, incl, form, c_p, cs, n_p, v_p, d_p, num_p, numel_seg, numel, vt, st, w, wb, s)

    try:
        full = (cn.ptr, vi.ptr, do.ptr)
        for op in (-1, 3, 100):
            assert call(*full, op=op) == EARGS
        for incl in (-1, 2, 100):
            assert call(*full, incl=incl) == EARGS
        for form in (-1, 2, 100):
            assert call(*full, form=form) == EARGS
        for cs in (0, 1, 2, 3, 16):
            assert call(*full, cs=cs) == EUNSUPPORTED, cs
        for vt, st in ((LONG, UINT), (ULONG, INT), (clo.CLO_TYPES["float"], UINT), (UINT, clo.CLO_TYPES["double"]), (clo.CLO_TYPES["ushort"], UINT), (-1, UINT)):
            assert call(*full, vt=vt, st=st) == EUNSUPPORTED, (vt, st)
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(*full, n_p=ni.ptr + 4) == EARGS                                                     # num_in misaligned
        assert call(*full, numel_seg=1 << 32) == EARGS and call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, do.ptr) == EARGS and call(None, None, None, form=1, numel_seg=0, numel=0) == EARGS
        assert call(cn.ptr, None, do.ptr) == EARGS and call(cn.ptr, vi.ptr, None) == EARGS              # values_in, data_out missing
        for i in range(3):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        for i, kw in ((0, dict(cs=8)), (1, dict(vt=LONG, st=LONG)), (2, dict(st=ULONG))):               # 4-aligned is not 8-aligned
            args = list(full)
            args[i] += 4
            assert call(*args, **kw) == EARGS, i
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        q.finish()
        for r in (do, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; num_in; views at an odd element; numel_seg 0
        # needs no workspace, no counts
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        rows = lambda dt, k: do.base.read(q, np.uint8, do.host.size)[do.at:do.at + k * np.dtype(dt).itemsize].copy().view(dt)
        assert call(*full) == 0
        q.finish()
        want, t = segscan("sum", "counts", counts[:m_h], vals[:n], "uint")
        assert first() == t and np.array_equal(rows(np.uint32, want.size), want)
        assert call(*full, op=2, incl=1, n_p=ni.ptr, st=ULONG) == 0
        q.finish()
        want, t = segscan("max", "counts", counts[:m_h], vals[:n], "ulong", True, m_h // 2)
        assert first() == t and np.array_equal(rows(np.uint64, want.size), want)
        assert call(cn.ptr + 4, vi.ptr + 4, do.ptr + 4, op=1, vt=INT, st=INT) == 0
        q.finish()
        want, t = segscan("min", "counts", counts[1:m_h + 1], vals[1:n + 1].view(np.int32), "int")
        assert first() == t and np.array_equal(rows(np.int32, want.size + 1)[1:], want)
        assert call(None, vi.ptr, do.ptr, numel_seg=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (cn, vi, ni, do, num):
            r.close()


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, T, form):
    """clo_hip_segscan captured from one client stream (a linear graph) after one eager warm-up and replayed three times,
    the counts, num_in and the values rewritten and data_out and num_out refilled with a canary before each replay (the
    protocol of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the rows."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, n = 900, 4 * T + 3
    need = lib.clo_hip_segscan_workspace_bytes(m_h, n)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, 4 * n, 8 * n, 8, need)]
    src_m, nin_m, vi, do, num, ws = made
    means = [16, 3, 40, 9, 16]                                              # 900 segments of mean 40: above the rows
    totals = set()
    INT, LONG = clo.CLO_TYPES["int"], clo.CLO_TYPES["long"]

    def load(r):
        counts = np.random.default_rng(300 + r).geometric(1 / means[r], m_h) - (np.arange(m_h) % 4 == r % 4)
        src, num_in, vals = source(form, "uint", counts, 50 * r), m_h - 100 * (r % 3), values_for("int", n, r)
        for m in (do, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (vi, vals)):
            mem_.put(arr)
        want = segscan("min", form, src, vals, "long", True, num_in)
        totals.add(want[1])
        return want, vals

    def enqueue():
        return lib.clo_hip_segscan(1, 1, FORMS.index(form), src_m.ptr, 4, nin_m.ptr, vi.ptr, do.ptr, num.ptr, m_h, n, INT, LONG, ws.ptr, need, q.stream)

    def verify(r, want):
        (data, total), vals = want
        tag = "%s round %d" % (form, r)
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        GC.same(do.get(np.int64, n), np.concatenate((data, GC.canary(np.int64, n - data.size))), tag + ": data_out")
        GC.same(vi.get(np.int32, n), vals, "values_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(totals) >= 4 and max(totals) > n > min(totals), totals
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def test_broken_preconditions_stay_in_bounds(dev, T):
    """Offsets that descend or are unordered, counts whose sums wrap 2^64, a num_in above numel_seg: the call completes,
    the canaries and the inputs are intact. Contents are not compared: DESIGN.md section 23 gives the argument that this
    holds by construction, and this run shows it once."""
    rng = np.random.default_rng(90)
    m_h, n = 3 * T + 700, 3 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 2).astype(np.uint32)
    unordered = rng.integers(0, 2 * n, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for i, (form, ct, src) in enumerate((("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping))):
        for op in OPS:
            run_scan(dev, op, bool(i % 2), form, ct, "int", "long", None, n, "broken preconditions", num_in=m_h + 1000, src=src, compare=False, seed=i)


def test_rows_above_2p31(dev, T):
    """n = 2^31 + 2^20 + 5 rows of int values, the inclusive sum in int: segments of 5 rows and one of 3 T + 1 rows laid
    across row 2^31 (the run structure of test_gpu_above_2p31.py). Counts and values are made on the device, value i
    being i & 0xff, and the rows are checked there in chunks against the closed form P(i + 1) - P(b(i)), P(x) the sum of
    j & 0xff over j < x."""
    import torch
    from test_gpu_above_2p31 import N, Runs, as_buffer, chunks
    clo, ctx, q = dev
    if torch.cuda.get_device_properties(0).total_memory < (96 << 30):
        pytest.skip("needs ~60 GiB of device memory")
    runs = Runs(T)
    m = runs.rows
    counts = torch.full((m,), 5, dtype=torch.int32, device="cuda")
    counts[runs.r0] = runs.long
    counts[m - 1] = runs.last
    vals = torch.empty(N, dtype=torch.int32, device="cuda")
    for lo, hi in chunks(N):
        vals[lo:hi] = (torch.arange(lo, hi, dtype=torch.int64, device="cuda") & 0xff).to(torch.int32)
    out = torch.full((N + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")                          # bytes A5 A5 A5 A5
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (counts, vals, out, cnt)]
    sc = clo.SegScan("sum", "counts", ctx, "int", "int", "uint", inclusive=True)
    P = lambda x: (x >> 8) * 32640 + (x & 0xff) * ((x & 0xff) - 1) // 2
    try:
        assert sc.with_device_data(q, bufs[0], None, bufs[1], bufs[2], bufs[3], m, N)
        q.finish()
        assert int(cnt[0]) == N
        for lo, hi in chunks(N):
            i, _, b = runs.run_and_start(torch, lo, hi)
            want = P(i + 1) - P(b)                                                                      # (below 2^31: 3 T + 1 rows of at most 255)
            assert bool((out[lo:hi].to(torch.int64) == want).all()), "data_out differs in rows [%d, %d)" % (lo, hi)
        assert bool((out[N:] == -0x5A5A5A5B).all()), "rows >= n were written"
    finally:
        for x in bufs + [sc]:
            x.close()
        del counts, vals, out
        torch.cuda.empty_cache()
