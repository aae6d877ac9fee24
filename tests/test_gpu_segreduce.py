"""CloSegReduce (include/clo_segreduce.h) on the GPU against the numpy model of tests/segreduce_model.py, bit for bit.
Every array is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); aggr_out and num_out are pre-filled with the pattern, and after every call num_out is the model's
unclamped total, the m rows written equal the model's, and the guards, every input and every row at index >= m are
unchanged. With T = clo_hip_segreduce_tile, the merge steps (segment ends plus rows) of a tile: row counts and m + n around
the tile edges x count patterns; all segments empty, runs of 4 T + 5 and of 2^20 empty segments; totals above n; num_in
below, at and above; both forms, both count types, rebased offsets and uint offsets that end at 2^32 - 1; every legal
(value, sum) pair x the three ops on values at the types' extremes; cross-checks against reduce by key on CloExpand's
segment ids, the round trip through CloExpand and a chain behind reduce by key without a host wait; element-aligned
views, two queues, the host form, the thin ABI's status codes, a captured graph replayed on other counts and values;
offsets that do not ascend and sums that wrap (in bounds, contents not compared); rows above 2^31 against a closed
form; and open aggregates carried across and through whole trips of the one-group carry scan (about 35 M rows)."""
import numpy as np
import pytest

from segreduce_model import FORMS, NP, OPS, PAIRS, identity, segreduce
from test_gpu_histogram import Region

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
    t = clo.segreduce_tile(4, 4)
    assert t >= 1024 and all(clo.segreduce_tile(v, s) == t for v, s in ((4, 8), (8, 8)))
    return t


def values_for(vt, n, seed=0):
    """A quarter of the values at the type's extremes (wrapped sums; the signed and the unsigned order differ), the rest
    over the whole range except the extremes themselves, so that an identity is no value present."""
    rng = np.random.default_rng(1000 + seed)
    info = np.iinfo(NP[vt])
    v = rng.integers(info.min + 2, info.max - 1, n, dtype=NP[vt])
    ext = np.array([info.min + 1, info.max - 1, -1 if info.min < 0 else info.max // 2 + 1, 0], dtype=NP[vt])
    pick = rng.random(n) < 0.25
    v[pick] = rng.choice(ext, int(pick.sum()))
    return v


def source(form, ct, counts, base=0):
    counts = np.asarray(counts, dtype=np.uint64)
    if form == "counts":
        return counts.astype(CDT[ct])
    return (np.concatenate((np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64))) + np.uint64(base)).astype(CDT[ct])


def run_seg(dev, op, form, ct, vt, st, counts, n, what, num_in=None, base=0, offs=(0, 0, 0), obj=None, q=None, src=None, compare=True, seed=0,
            vals=None):
    """One call on views at byte offsets offs = (counts_or_offsets, values_in, aggr_out) with n rows of values; checks
    everything and returns (total, aggr). src: the input as it is (broken preconditions); compare False: the rows'
    contents are not compared; vals: the n values, instead of values_for(vt, n, seed)."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = source(form, ct, counts, base)
    m_h = src.size - (1 if form == "offsets" else 0)
    if vals is None:
        vals = values_for(vt, n, seed)
    assert vals.dtype == NP[vt] and vals.size == n
    aggr, total = segreduce(op, form, src, vals, st, num_in) if compare else (None, None)
    what = "%s %s %s %s->%s n %d, %s" % (op, form, ct, vt, st, n, what)
    ss = np.dtype(NP[st]).itemsize
    sr = obj or clo.SegReduce(op, form, ctx, vt, st, ct)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0)
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if n else None
    a_r = Region(rdev, m_h * ss, offs[2], None, 2) if m_h else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert sr.with_device_data(q, s_r.view, view(n_r), view(v_r), view(a_r), num_r.view, m_h, n), what
        q.finish()
        got = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        if compare:
            assert got == total, "%s: num_out = %d, the model's total is %d" % (what, got, total)
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            if a_r:
                now = a_r.base.read(q, np.uint8, a_r.host.size)[a_r.at:a_r.at + aggr.nbytes].copy().view(NP[st])
                bad = np.flatnonzero(now != aggr)
                assert bad.size == 0, "%s: %d of %d segments differ, first %d: %r, the model has %r" % (
                    what, bad.size, aggr.size, bad[0], now[bad[0]], aggr[bad[0]])
                a_r.check(aggr, what + ": aggr_out")                        # ... and nothing behind the m rows written
        elif a_r:                                                          # in bounds: the guards
            now = a_r.base.read(q, np.uint8, a_r.host.size)
            a_r.check(now[a_r.at:a_r.at + m_h * ss], what)
        s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return got, aggr
    finally:
        for r in (s_r, n_r, v_r, a_r, num_r):
            if r:
                r.close()
        if obj is None:
            sr.close()


PATTERNS = ("ones", "sevens", "one segment", "long between ones", "alternating 0 and 3", "zeros at the start", "zeros at the end",
            "an end on every tile edge", "geometric")


def counts_of(pattern, total, T, seed):
    """Counts of the pattern whose sum is total."""
    def fit(c):                                                           # cut to the total, the last count takes the rest
        c = np.asarray(c, np.int64)
        keep = int(np.searchsorted(np.cumsum(c), total, "left")) + 1 if total else 0
        c = c[:keep].copy()
        if c.size:
            c[-1] -= int(c.sum()) - total
        assert int(c.sum()) == total and (c >= 0).all()
        return c
    if pattern == "ones":
        return fit(np.ones(total, np.int64))
    if pattern == "sevens":
        return fit(np.full(total // 7 + 1, 7))
    if pattern == "one segment":
        return np.array([total], np.int64)
    if pattern == "long between ones":                                    # a segment that spans three tiles and more
        long = min(3 * T + 1, max(total - 2, 0))
        before = (total - long) // 2
        return np.concatenate((np.ones(before, np.int64), [long], np.ones(total - long - before, np.int64)))
    if pattern == "alternating 0 and 3":
        return fit(np.tile([0, 3], total // 3 + 1))
    if pattern == "zeros at the start":
        return np.concatenate((np.zeros(41, np.int64), fit(np.full(total // 5 + 1, 5))))
    if pattern == "zeros at the end":
        return np.concatenate((fit(np.full(total // 5 + 1, 5)), np.zeros(41, np.int64)))
    if pattern == "an end on every tile edge":
        # closing segment r is merge step r + e_r: the steps k T - 2, k T - 1 and k T (the last of a tile, the first of the next)
        steps = sorted(d for k in range(1, 8) for d in (k * T - 2, k * T - 1, k * T))
        ends = [d - r for r, d in enumerate(steps) if d - r <= total]
        ends = np.array(ends + [total], np.int64)
        return np.diff(np.concatenate(([0], ends)))
    return fit(np.random.default_rng(seed).geometric(1 / 16, total // 8 + 8))


def rotate(case):
    """An op, a form, a count type and a type pair for case number `case`: every one of them meets every pattern."""
    return OPS[case % 3], FORMS[case // 3 % 2], ("uint", "ulong")[case // 6 % 2], PAIRS[case % len(PAIRS)]


def test_sizes_and_count_patterns(dev, T):
    case = 0
    for n in (0, 1, T - 1, T, T + 1, 2 * T + 3, 5 * T + 17):
        for pattern in PATTERNS:
            op, form, ct, (vt, st) = rotate(case)
            case += 1
            counts = counts_of(pattern, n, T, case)
            got, _ = run_seg(dev, op, form, ct, vt, st, counts, n, "%s" % pattern, base=case * 1000, seed=case)
            assert got == n


def test_merge_lengths_around_the_tile_edges(dev, T):
    """m + n, the number of merge steps, one below, on and one above a tile's and two tiles' length, with few long, as
    many and many short segments."""
    case = 0
    for steps in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 3):
        for m in (3, steps // 2, steps - 5):
            n = steps - m
            counts = np.full(m, n // m, np.int64)
            counts[:n % m] += 1
            op, form, ct, (vt, st) = rotate(case)
            case += 1
            got, _ = run_seg(dev, op, form, ct, vt, st, counts, n, "%d segments + %d rows" % (m, n), seed=case)
            assert got == n


# clo_hip_seg_device.h: CLO_SEG_CARRY_TRIP = CLO_SEG_THREADS * CLO_SEG_CARRY_ITEMS, the tile states the one work-group of the carry
# scan takes per trip (4096 today; there is no getter). The cases below hold two trips and 108 tiles: three trips, and
# still a second one if a trip were doubled.
CARRY_TRIP = 4096
CARRY_LAYOUTS = ("a segment across each trip edge", "one segment through the whole second trip")


def fill_steps(rng, steps, mean=16):
    """Counts of geometric length that take exactly `steps` merge steps: a segment of c rows takes c + 1, its rows and
    its end."""
    if steps <= 0:
        return np.zeros(0, np.int64)
    c = rng.geometric(1 / mean, steps // (mean + 1) + 64)
    while int((c + 1).sum()) < steps:
        c = np.concatenate((c, rng.geometric(1 / mean, 64)))
    c = c[:int(np.searchsorted(np.cumsum(c + 1), steps, "left")) + 1].copy()
    c[-1] -= int((c + 1).sum()) - steps                                   # (0 at the least: an empty segment)
    assert int((c + 1).sum()) == steps and (c >= 0).all()
    return c


def carry_layout(T, layout):
    """(counts, [(segment, first row, rows, first step, steps)] of the long segments): 2 * CARRY_TRIP + 108 tiles of merge
    steps. Positions are in merge steps, rows plus the segment ends before them: segment r with rows [s, e) takes the
    steps [s + r, e + r]."""
    E = CARRY_TRIP * T
    if layout == CARRY_LAYOUTS[0]:
        spans = ((E - 5 * T // 2, E + 5 * T // 2), (2 * E - T // 2, 2 * E + T // 2))
    else:
        spans = ((100 * T + 7, 2 * E + 100 * T - 9),)
    rng = np.random.default_rng(70 + CARRY_LAYOUTS.index(layout))
    parts, longs, at, seg, row = [], [], 0, 0, 0
    for a, b in spans:
        f = fill_steps(rng, a - at)
        seg, row = seg + f.size, row + int(f.sum())
        parts += [f, np.array([b - a - 1])]
        longs.append((seg, row, b - a - 1, a, b - a))
        seg, row, at = seg + 1, row + b - a - 1, b
    parts.append(fill_steps(rng, 2 * E + 108 * T - at))
    return np.concatenate(parts).astype(np.int64), longs


@pytest.fixture(scope="module")
def carry_cases(T):
    """The two layouts and one array of values per value type, shared by the cases: in every long segment the type's
    minimum and maximum are planted within the first T / 2 rows, before the trip edge, so that an aggregate that loses
    what was carried in is wrong."""
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
def test_open_aggregates_cross_the_trips_of_the_carry_scan(dev, T, carry_cases, layout, case):
    """m + n = (2 * 4096 + 108) T merge steps. Layout 1: short segments, one segment over the steps [4096 T - 2.5 T,
    4096 T + 2.5 T) and one over [8192 T - T / 2, 8192 T + T / 2): an open aggregate is carried from one trip of the carry
    scan into the next. Layout 2: one segment from step 100 T to step 8292 T: the whole second trip holds no segment end
    and the carried state passes through it unchanged."""
    op, vt, st = (("sum", "int", "long"), ("sum", "uint", "uint"), ("min", "int", "int"), ("max", "uint", "uint"))[case]
    layouts, vals = carry_cases
    counts, longs = layouts[layout]
    m, n = counts.size, int(counts.sum())
    E = CARRY_TRIP * T
    assert m + n == 2 * E + 108 * T
    if layout == CARRY_LAYOUTS[0]:                                        # the segments lie where the docstring says
        assert [(first, steps) for _, _, _, first, steps in longs] == [(E - 5 * T // 2, 5 * T), (2 * E - T // 2, T)]
    else:
        (_, _, _, first, steps), = longs
        assert first < E and first + steps > 2 * E + T
    for seg, row, length, first, steps in longs:                          # ... in merge steps: rows plus ends before
        assert counts[seg] == length and int(counts[:seg].sum()) == row and row + seg == first and length + 1 == steps
    k = case + CARRY_LAYOUTS.index(layout)
    got, aggr = run_seg(dev, op, FORMS[k % 2], ("uint", "ulong")[k // 2 % 2], vt, st, counts, n, layout, base=7 * k, vals=vals[vt][:n])
    assert got == n
    info = np.iinfo(NP[vt])
    for seg, row, length, _, _ in longs:
        if op != "sum":
            assert aggr[seg] == (info.min if op == "min" else info.max), (layout, op, seg)
    if vt == "uint" and op == "sum":                                      # the sums wrap
        wide = np.add.reduceat(vals["uint"][:n].astype(np.uint64), np.cumsum(counts)[:-1][counts[1:] > 0][:1000])
        assert (wide >= 1 << 32).any()


def test_empty_segments(dev, T):
    case = 0
    for m in (1, 5, T, 2 * T + 1):                                        # nothing but empty segments, without and with rows nobody owns
        for n in (0, 7, T + 3):
            op, form, ct, (vt, st) = rotate(case)
            case += 1
            got, aggr = run_seg(dev, op, form, ct, vt, st, np.zeros(m, np.int64), n, "%d empty segments" % m, seed=case)
            assert got == 0 and (aggr == identity(op, st)).all()
    counts = np.concatenate((np.full(9, T // 4 + 1), np.zeros(4 * T + 5, np.int64), np.full(9, T // 4 + 1)))
    for op in OPS:
        for form, ct in (("counts", "ulong"), ("offsets", "uint")):
            run_seg(dev, op, form, ct, "int", "long", counts, int(counts.sum()), "4 T + 5 empty segments between rows", seed=3)


def test_a_million_empty_segments_take_bounded_work(dev, T):
    """2^20 empty segments at one position, between rows: a tile is T merge steps whatever they are, so this is 2^20 / T
    more tiles of the same work, not one work-group that walks 2^20 ends."""
    counts = np.concatenate((np.full(5, 700), np.zeros(1 << 20, np.int64), np.full(5, 900), np.zeros(3, np.int64)))
    for op, form in (("sum", "counts"), ("min", "offsets"), ("max", "counts")):
        got, aggr = run_seg(dev, op, form, "uint", "int", "int", counts, 8000, "2^20 empty segments", seed=4)
        assert got == 8000 and (aggr[5:5 + (1 << 20)] == identity(op, "int")).all()


def test_totals_above_the_rows(dev, T):
    """num_out always receives the unclamped total; a segment cut by n reduces the rows it has, the segments beyond
    receive the identity."""
    case = 0
    for total in (T + 1, 3 * T + 11):
        for pattern in ("sevens", "geometric", "long between ones"):
            counts = counts_of(pattern, total, T, 7)
            for n in (0, 1, total // 2, total - 3, total - 1):
                op, form, ct, (vt, st) = rotate(case)
                case += 1
                got, aggr = run_seg(dev, op, form, ct, vt, st, counts, n, "%s, total %d" % (pattern, total), seed=case)
                ends = np.cumsum(counts)
                assert got == total and (aggr[np.concatenate(([0], ends[:-1])) >= n] == identity(op, st)).all()


def test_num_in(dev, T):
    counts = counts_of("geometric", 3 * T + 9, T, 6)
    counts[::6] = 0
    m_h = counts.size
    for i, num_in in enumerate((0, 1, m_h // 2, m_h - 1, m_h, m_h + 1, 1 << 40)):
        for form in FORMS:
            want = int(counts[:min(num_in, m_h)].sum())
            got, aggr = run_seg(dev, OPS[i % 3], form, ("uint", "ulong")[i % 2], "uint", "ulong", counts, 3 * T + 9, "num_in %d of %d" % (num_in, m_h),
                                num_in=num_in, base=5 * i, seed=i)
            assert got == want and aggr.size == min(num_in, m_h)


@pytest.mark.parametrize("ct", ["uint", "ulong"])
@pytest.mark.parametrize("form", FORMS)
def test_forms_and_types(dev, T, form, ct):
    """Both forms x both count types x every legal (value, sum) pair x the three ops, empty segments among the others."""
    counts = counts_of("geometric", 2 * T + 3, T, 5)
    counts[::7] = 0
    for i, (vt, st) in enumerate(PAIRS):
        for op in OPS:
            _, aggr = run_seg(dev, op, form, ct, vt, st, counts, 2 * T + 3, "every type", base=3, seed=i)
            assert (aggr[::7] == identity(op, st)).all()


def test_offsets_with_a_base(dev, T):
    counts = counts_of("geometric", 2 * T + 100, T, 8)
    total = int(counts.sum())
    run_seg(dev, "sum", "offsets", "uint", "int", "long", counts, total, "offsets[0] = 12345", base=12345)
    run_seg(dev, "min", "offsets", "ulong", "int", "int", counts, total, "offsets[0] = 2^40 + 12345", base=(1 << 40) + 12345)
    src = source("offsets", "uint", counts, (1 << 32) - 1 - total)
    assert int(src[-1]) == (1 << 32) - 1
    run_seg(dev, "max", "offsets", "uint", "uint", "uint", counts, total, "uint offsets that end at 2^32 - 1", src=src)


def test_against_reduce_by_key_on_expanded_segment_ids(dev, T):
    """Where no segment is empty, reduce by key on CloExpand's seg_out computes the same rows."""
    clo, ctx, q = dev
    counts = counts_of("geometric", 3 * T + 50, T, 21)
    m, n = counts.size, int(counts.sum())
    assert (counts > 0).all()
    for op in OPS:
        for vt, st in (("int", "long"), ("uint", "uint"), ("long", "ulong")):
            vals = values_for(vt, n, 21)
            ss = np.dtype(NP[st]).itemsize
            c_r, v_r = Region(dev, 4 * m, 0, counts.astype(np.uint32), 0), Region(dev, vals.nbytes, 0, vals, 1)
            seg_r, n1_r, ka_r, a1_r, runs_r = (Region(dev, 4 * n, 0, None, 2), Region(dev, 8, 0, None, 0), Region(dev, 4 * n, 0, None, 1),
                                               Region(dev, ss * n, 0, None, 2), Region(dev, 8, 0, None, 0))
            a2_r, n2_r = Region(dev, ss * m, 0, None, 1), Region(dev, 8, 0, None, 2)
            ex, rbk, sr = clo.Expand("counts", ctx, None, "uint"), clo.ReduceByKey(ctx, "uint", vt, st, op), clo.SegReduce(op, "counts", ctx, vt, st, "uint")
            try:
                assert ex.with_device_data(q, c_r.view, None, None, None, seg_r.view, None, n1_r.view, m, n)
                assert rbk.with_device_data(q, seg_r.view, v_r.view, ka_r.view, a1_r.view, runs_r.view, n)
                assert sr.with_device_data(q, c_r.view, None, v_r.view, a2_r.view, n2_r.view, m, n)
                q.finish()
                runs_r.check(np.array([m], np.uint64), "num_runs_out")
                composed = a1_r.base.read(q, np.uint8, a1_r.host.size)[a1_r.at:a1_r.at + ss * m].copy().view(NP[st])
                a2_r.check(composed, "%s %s->%s: segment reduce against expand + reduce by key" % (op, vt, st))
                a2_r.check(segreduce(op, "counts", counts, vals, st)[0], "the model")
            finally:
                for x in (c_r, v_r, seg_r, n1_r, ka_r, a1_r, runs_r, a2_r, n2_r, ex, rbk, sr):
                    x.close()


def test_round_trip_through_expand(dev, T):
    """segreduce(sum, expand(values, counts), counts) == values * counts in wrapped arithmetic, empty segments included."""
    clo, ctx, q = dev
    counts = counts_of("geometric", 3 * T + 77, T, 22)
    counts[::4] = 0
    m, n = counts.size, int(counts.sum())
    for ct, vt in (("uint", "uint"), ("ulong", "long")):
        vals = values_for(vt, m, 22)
        vs = vals.dtype.itemsize
        c_r, v_r = Region(dev, counts.size * np.dtype(CDT[ct]).itemsize, 0, counts.astype(CDT[ct]), 0), Region(dev, vals.nbytes, 0, vals, 1)
        rows_r, n1_r, a_r, n2_r = Region(dev, vs * n, 0, None, 2), Region(dev, 8, 0, None, 0), Region(dev, vs * m, 0, None, 1), Region(dev, 8, 0, None, 2)
        ex, sr = clo.Expand("counts", ctx, vt, ct), clo.SegReduce("sum", "counts", ctx, vt, vt, ct)
        try:
            assert ex.with_device_data(q, c_r.view, None, v_r.view, rows_r.view, None, None, n1_r.view, m, n)
            assert sr.with_device_data(q, c_r.view, None, rows_r.view, a_r.view, n2_r.view, m, n)
            q.finish()
            n2_r.check(np.array([n], np.uint64), "num_out")
            a_r.check((vals.view("u%d" % vs) * counts.astype("u%d" % vs)).view(vals.dtype), "values * counts")
        finally:
            for x in (c_r, v_r, rows_r, n1_r, a_r, n2_r, ex, sr):
                x.close()


def test_chain_behind_reduce_by_key(dev, T):
    """Reduce by key collapses keys into (key, run length) rows; its num_runs_out is the segment reduce's num_in and its
    run lengths are the counts, numel_seg being the buffers' row count: the maximum of every run's values. One queue, no
    host wait in between."""
    clo, ctx, q = dev
    n = 3 * T + 5
    keys = np.sort(np.random.default_rng(30).integers(0, 500, n).astype(np.uint32))
    vals = values_for("int", n, 30)
    k_r, v_r = Region(dev, 4 * n, 0, keys, 0), Region(dev, 4 * n, 0, vals, 1)
    rk_r, len_r, runs_r = Region(dev, 4 * n, 0, None, 0), Region(dev, 4 * n, 0, None, 1), Region(dev, 8, 0, None, 2)
    a_r, num_r = Region(dev, 8 * n, 0, None, 0), Region(dev, 8, 0, None, 1)
    rbk, sr = clo.ReduceByKey(ctx, "uint", None, "uint"), clo.SegReduce("max", "counts", ctx, "int", "long", "uint")
    try:
        assert rbk.with_device_data(q, k_r.view, None, rk_r.view, len_r.view, runs_r.view, n)
        assert sr.with_device_data(q, len_r.view, runs_r.view, v_r.view, a_r.view, num_r.view, n, n)
        q.finish()
        uniq, first = np.unique(keys, return_index=True)
        runs_r.check(np.array([uniq.size], np.uint64), "num_runs_out")
        num_r.check(np.array([n], np.uint64), "num_out")
        a_r.check(np.maximum.reduceat(vals.astype(np.int64), first), "the maximum of every run")      # rows >= num_runs_out untouched
    finally:
        for x in (k_r, v_r, rk_r, len_r, runs_r, a_r, num_r, rbk, sr):
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
        run_seg(dev, OPS[i % 3], form, ct, vt, st, counts, n, "views at %s" % (offs,), offs=offs, base=9, seed=i)


def test_two_objects_on_two_queues_and_one_object_moved(dev, T):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds; then
    one object used on the first queue, the second and the first again (its workspace follows the queue)."""
    clo, ctx, _ = dev
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("sum", "counts", "uint", "uint", "uint"), ("min", "offsets", "ulong", "int", "long"))
    objs = [clo.SegReduce(op, form, ctx, vt, st, ct) for op, form, ct, vt, st in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (op, form, ct, vt, st) in enumerate(specs):
                counts = counts_of("geometric", 40 * T + 9 + rnd, T, 10 * rnd + i)
                counts[::9] = 0
                n = int(counts.sum())
                src, vals = source(form, ct, counts, 7), values_for(vt, n, rnd)
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, src.nbytes, 0, src, 0), Region(rdev, vals.nbytes, 0, vals, 1),
                        Region(rdev, counts.size * np.dtype(NP[st]).itemsize, 0, None, 2), Region(rdev, 8, 0, None, 0)]
                sent.append((src, vals, counts.size, n, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (src, vals, m_h, n, regs) in enumerate(sent):
                assert objs[i].with_device_data(qs[i], regs[0].view, None, regs[1].view, regs[2].view, regs[3].view, m_h, n)
            for i in range(2):
                qs[i].finish()
            for i, (src, vals, m_h, n, regs) in enumerate(sent):
                aggr, t = segreduce(specs[i][0], specs[i][1], src, vals, specs[i][4])
                what = "round %d, %s" % (rnd, specs[i][1])
                regs[3].check(np.array([t], np.uint64), what + ": num_out")
                regs[2].check(aggr, what + ": aggr_out")
                for r in regs:
                    r.close()
        for j, qi in enumerate((0, 1, 0, 1)):
            total = (5, 60, 2, 30)[j] * T + j                               # small, large, small, large
            counts = counts_of("geometric", total, T, 40 + j)
            run_seg((clo, ctx, qs[qi]), "sum", "counts", "uint", "uint", "uint", counts, total, "moved, call %d" % j, obj=objs[0], q=qs[qi], seed=j)
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
            for op, ct, vt, st in (("sum", "uint", "int", "long"), ("min", "ulong", "uint", "uint"), ("max", "uint", "long", "long")):
                src = source(form, ct, counts, 4321)
                sr = clo.SegReduce(op, form, ctx, vt, st, ct)
                for n in (0, total - 5, total, total + 7):
                    vals = values_for(vt, n, n)
                    for num_in, qe, qcomm in ((None, q, qc), (counts.size // 2, None, None), (counts.size + 9, q, None)):
                        aggr, t = segreduce(op, form, src, vals, st, num_in)
                        a, got = sr.with_host_data(src, vals, num_in=num_in, q_exec=qe, q_comm=qcomm)
                        assert got == t and a.dtype == aggr.dtype and np.array_equal(a, aggr), (form, op, ct, vt, st, n, num_in)
                sr.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev, T):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    INT, UINT, LONG, ULONG = (clo.CLO_TYPES[t] for t in ("int", "uint", "long", "ulong"))
    m_h, n = 1000, 3 * T
    need = lib.clo_hip_segreduce_workspace_bytes(m_h, n)
    assert need > 0 and need % 256 == 0
    counts = np.random.default_rng(5).integers(0, 9, 2 * m_h + 4, dtype=np.uint32)
    vals = values_for("uint", 2 * n + 4, 5)
    cn, vi, ni = Region(dev, counts.nbytes, 0, counts, 0), Region(dev, vals.nbytes, 0, vals, 1), Region(dev, 16, 0, np.array([m_h // 2, 0], np.uint64), 2)
    ao, num = Region(dev, 8 * m_h + 16, 0, None, 0), Region(dev, 16, 0, None, 1)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(c_p, v_p, a_p, op=0, form=0, cs=4, n_p=None, num_p=num.ptr, numel_seg=m_h, numel=n, vt=UINT, st=UINT, w=ws.ptr, wb=need):
        return lib.clo_hip_segreduce(op, form, c_p, cs, n_p, v_p, a_p, num_p, numel_seg, numel, vt, st, w, wb, s)

    try:
        full = (cn.ptr, vi.ptr, ao.ptr)
        for op in (-1, 3, 100):
            assert call(*full, op=op) == EARGS
        for form in (-1, 2, 100):
            assert call(*full, form=form) == EARGS
        for cs in (0, 1, 2, 3, 16):
            assert call(*full, cs=cs) == EUNSUPPORTED, cs
        for vt, st in ((LONG, UINT), (ULONG, INT), (clo.CLO_TYPES["float"], UINT), (UINT, clo.CLO_TYPES["double"]), (clo.CLO_TYPES["ushort"], UINT), (-1, UINT)):
            assert call(*full, vt=vt, st=st) == EUNSUPPORTED, (vt, st)
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(*full, n_p=ni.ptr + 4) == EARGS                                                     # num_in misaligned
        assert call(*full, numel_seg=1 << 32) == EARGS and call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, ao.ptr) == EARGS and call(None, None, None, form=1, numel_seg=0, numel=0) == EARGS
        assert call(cn.ptr, None, ao.ptr) == EARGS and call(cn.ptr, vi.ptr, None) == EARGS              # values_in, aggr_out missing
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
        for r in (ao, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; num_in; views at an odd element; numel_seg 0
        # needs no workspace, no input
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        rows = lambda dt, k: ao.base.read(q, np.uint8, ao.host.size)[ao.at:ao.at + k * np.dtype(dt).itemsize].copy().view(dt)
        assert call(*full) == 0
        q.finish()
        want, t = segreduce("sum", "counts", counts[:m_h], vals[:n], "uint")
        assert first() == t and np.array_equal(rows(np.uint32, m_h), want)
        assert call(*full, op=2, n_p=ni.ptr, st=ULONG) == 0
        q.finish()
        want, t = segreduce("max", "counts", counts[:m_h], vals[:n], "ulong", m_h // 2)
        assert first() == t and np.array_equal(rows(np.uint64, m_h // 2), want)
        assert call(cn.ptr + 4, vi.ptr + 4, ao.ptr + 4, op=1, vt=INT, st=INT) == 0
        q.finish()
        want, t = segreduce("min", "counts", counts[1:m_h + 1], vals[1:n + 1].view(np.int32), "int")
        assert first() == t and np.array_equal(rows(np.int32, m_h + 1)[1:], want)
        assert call(None, vi.ptr, None, numel_seg=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (cn, vi, ni, ao, num):
            r.close()


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, T, form):
    """clo_hip_segreduce captured from one client stream (a linear graph) after one eager warm-up and replayed three
    times, the counts, num_in and the values rewritten and aggr_out and num_out refilled with a canary before each replay
    (the protocol of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the rows."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, n = 900, 4 * T + 3
    need = lib.clo_hip_segreduce_workspace_bytes(m_h, n)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, 4 * n, 8 * m_h, 8, need)]
    src_m, nin_m, vi, ao, num, ws = made
    means = [16, 3, 40, 9, 16]                                              # 900 segments of mean 40: above the rows
    totals = set()
    INT, LONG = clo.CLO_TYPES["int"], clo.CLO_TYPES["long"]

    def load(r):
        counts = np.random.default_rng(300 + r).geometric(1 / means[r], m_h) - (np.arange(m_h) % 4 == r % 4)
        src, num_in, vals = source(form, "uint", counts, 50 * r), m_h - 100 * (r % 3), values_for("int", n, r)
        for m in (ao, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (vi, vals)):
            mem_.put(arr)
        want = segreduce("min", form, src, vals, "long", num_in)
        totals.add(want[1])
        return want, vals

    def enqueue():
        return lib.clo_hip_segreduce(1, FORMS.index(form), src_m.ptr, 4, nin_m.ptr, vi.ptr, ao.ptr, num.ptr, m_h, n, INT, LONG, ws.ptr, need, q.stream)

    def verify(r, want):
        (aggr, total), vals = want
        tag = "%s round %d" % (form, r)
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        GC.same(ao.get(np.int64, m_h), np.concatenate((aggr, GC.canary(np.int64, m_h - aggr.size))), tag + ": aggr_out")
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
    the canaries and the inputs are intact. Contents are not compared: DESIGN.md section 21 gives the argument that this
    holds by construction, and this run shows it once."""
    rng = np.random.default_rng(90)
    m_h, n = 3 * T + 700, 3 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 2).astype(np.uint32)
    unordered = rng.integers(0, 2 * n, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for i, (form, ct, src) in enumerate((("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping))):
        for op in OPS:
            run_seg(dev, op, form, ct, "int", "long", None, n, "broken preconditions", num_in=m_h + 1000, src=src, compare=False, seed=i)


def test_rows_above_2p31(dev, T):
    """n = 2^31 + 2^20 + 5 rows of int values summed in int: segments of 5 rows and one of 3 T + 1 rows laid across row
    2^31 (the run structure of test_gpu_above_2p31.py). Counts and values are made on the device, value i being i & 0xff,
    and the sums are checked there in chunks against the closed form over the rows' indices."""
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
    ao = torch.full((m + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")                           # bytes A5 A5 A5 A5
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (counts, vals, ao, cnt)]
    sr = clo.SegReduce("sum", "counts", ctx, "int", "int", "uint")
    try:
        assert sr.with_device_data(q, bufs[0], None, bufs[1], bufs[2], bufs[3], m, N)
        q.finish()
        assert int(cnt[0]) == N
        for lo, hi in chunks(m):
            r = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
            b = torch.where(r < runs.r0, 5 * r, runs.after + 5 * (r - runs.r0 - 1))                     # the segment's first row
            want = sum(((b + k) & 0xff) for k in range(5))
            if hi == m:
                want[-1] = sum(((int(b[-1]) + k) & 0xff) for k in range(runs.last))
            if lo <= runs.r0 < hi:
                want[runs.r0 - lo] = int((torch.arange(runs.s0, runs.after, dtype=torch.int64, device="cuda") & 0xff).sum())
            assert bool((ao[lo:hi].to(torch.int64) == want).all()), "aggr_out differs in segments [%d, %d)" % (lo, hi)
        assert bool((ao[m:] == -0x5A5A5A5B).all()), "rows >= m were written"
    finally:
        for x in bufs + [sr]:
            x.close()
        del counts, vals, ao
        torch.cuda.empty_cache()
