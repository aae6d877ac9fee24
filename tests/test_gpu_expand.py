"""CloExpand (include/clo_expand.h) on the GPU against the numpy model of tests/expand_model.py, bit for bit. Every array
is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs and num_out are pre-filled with the pattern, and after every call num_out is the
model's unclamped total, the rows written equal the model's, and the guards, every input and every row at index >=
min(total, capacity) are unchanged. With T = clo_hip_expand_tile and L = clo_hip_expand_lds_segments: totals around the
tile edges x count patterns; tiles with L - 1, L and L + 1 segment ends and a run of 2 L + 5 empty segments (both sides
of the switch between the LDS marks and the per-row search); both forms, both count types, every value size and every
subset of the outputs; num_in and capacity below, at and above; rebased offsets and uint offsets that end at 2^32 - 1;
chains with the by-key sort, reduce by key and the histogram without a host wait; element-aligned views, two queues, the
host form, the thin ABI's status codes, a captured graph replayed on other counts; offsets that do not ascend and sums
that wrap (in bounds, contents not compared); rows above 2^31 against a closed form; and 2^24 + 5 counts, three trips of
the shared ends' scan, through all three operations that use it."""
import itertools

import numpy as np
import pytest

from expand_model import FORMS, expand
from test_gpu_histogram import Region

pytestmark = pytest.mark.gpu

CDT = {"uint": np.uint32, "ulong": np.uint64}
VTYPE = {1: "char", 2: "half", 4: "float", 8: "double"}      # the values are opaque: only the size matters
SUBSETS = [s for s in itertools.product((False, True), repeat=3) if any(s)]    # (values, seg, rank)


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def TL(dev):
    clo = dev[0]
    T, L = clo.expand_tile(4), clo.expand_lds_segments()
    assert T >= 1024 and T % 1024 == 0 and L > 0 and all(clo.expand_tile(vs) == T for vs in (0, 1, 2, 8))
    return T, L


def values_for(vs, n):
    """n words of vs bytes that differ from their neighbours in every byte, the high ones included."""
    i = np.arange(n, dtype=np.uint64)
    x = (i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    return (x >> np.uint64(64 - 8 * vs)).astype("u%d" % vs)


def source(form, ct, counts, base=0):
    counts = np.asarray(counts, dtype=np.uint64)
    if form == "counts":
        return counts.astype(CDT[ct])
    return (np.concatenate((np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64))) + np.uint64(base)).astype(CDT[ct])


def run_expand(dev, form, ct, vs, outs, counts, what, capacity=None, num_in=None, base=0, offs=(0, 0, 0, 0, 0), obj=None, q=None, src=None,
               compare=True):
    """One call on views at byte offsets offs = (counts_or_offsets, values_in, values_out, seg_out, rank_out); checks
    everything and returns (total, seg). outs = (values, seg, rank). capacity None: the total. src: the input as it is
    (broken preconditions); compare False: the rows' contents are not compared."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = source(form, ct, counts, base)
    m_h = src.size - (1 if form == "offsets" else 0)
    seg, rank, total = expand(form, src, (1 << 32) - 1 if capacity is None else capacity, num_in)
    if capacity is None:
        capacity = total
    what = "%s %s value size %d outs %s, %s" % (form, ct, vs, outs, what)
    vals = values_for(vs, m_h) if vs else None                            # (value size 0: an object without a value type)
    ex = obj or clo.Expand(form, ctx, VTYPE.get(vs), ct)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0)
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if outs[0] else None
    vo_r = Region(rdev, capacity * vs, offs[2], None, 2) if outs[0] else None
    so_r = Region(rdev, capacity * 4, offs[3], None, 2) if outs[1] else None
    ro_r = Region(rdev, capacity * 4, offs[4], None, 0) if outs[2] else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert ex.with_device_data(q, s_r.view, view(n_r), view(v_r), view(vo_r), view(so_r), view(ro_r), num_r.view, m_h, capacity), what
        q.finish()
        got = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        got_seg = None
        if compare:
            assert got == total, "%s: num_out = %d, the model's total is %d" % (what, got, total)
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            if vo_r:
                vo_r.check(vals[seg], what + ": values_out")               # ... and nothing behind the rows written
            if so_r:
                so_r.check(seg, what + ": seg_out")
            if ro_r:
                ro_r.check(rank, what + ": rank_out")
        else:                                                              # in bounds: the guards, and every segment id below m_h
            rows = min(got, capacity)
            for r, size in ((vo_r, vs), (so_r, 4), (ro_r, 4)):
                if r:
                    now = r.base.read(q, np.uint8, r.host.size)
                    r.check(now[r.at:r.at + rows * size], what)
                    if r is so_r:
                        got_seg = now[r.at:r.at + rows * 4].copy().view(np.uint32)
                        assert rows == 0 or int(got_seg.max()) < m_h, what
        s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return got, (seg if compare else got_seg)
    finally:
        for r in (s_r, n_r, v_r, vo_r, so_r, ro_r, num_r):
            if r:
                r.close()
        if obj is None:
            ex.close()


PATTERNS = ("ones", "sevens", "one segment", "long between ones", "alternating 0 and 3", "zeros at the start", "zeros at the end",
            "around every tile edge", "geometric")


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
    if pattern == "long between ones":
        long = min(3 * T + 1, max(total - 2, 0))
        before = (total - long) // 2
        return np.concatenate((np.ones(before, np.int64), [long], np.ones(total - long - before, np.int64)))
    if pattern == "alternating 0 and 3":
        return fit(np.tile([0, 3], total // 3 + 1))
    if pattern == "zeros at the start":
        return np.concatenate((np.zeros(41, np.int64), fit(np.full(total // 5 + 1, 5))))
    if pattern == "zeros at the end":
        return np.concatenate((fit(np.full(total // 5 + 1, 5)), np.zeros(41, np.int64)))
    if pattern == "around every tile edge":                               # an end one row before, on and one row after every edge
        ends = sorted({e for k in range(1, total // T + 2) for e in (k * T - 1, k * T, k * T + 1) if 0 < e < total} | {total})
        return np.diff(np.concatenate(([0], ends))) if total else np.zeros(1, np.int64)
    return fit(np.random.default_rng(seed).geometric(1 / 16, total // 8 + 8))


def test_sizes_and_count_patterns(dev, TL):
    T, _ = TL
    case = 0
    for total in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 5 * T + 1):
        for pattern in PATTERNS:
            form, ct = FORMS[case % 2], ("uint", "ulong")[case // 2 % 2]
            vs, outs = (1, 2, 4, 8)[case // 4 % 4], SUBSETS[case % len(SUBSETS)]
            case += 1
            counts = counts_of(pattern, total, T, case)
            got, _ = run_expand(dev, form, ct, vs, outs, counts, "%s, total %d" % (pattern, total), base=case * 1000)
            assert got == total


def ends_scan_counts():
    """2^24 + 5 counts, all 0 but a 1 at a random 1 in 64 of the positions and at every position within 2 of a multiple of
    2^20. clo_hip_op_device.h: the one work-group of the shared ends' scan (clo_op_ends_sums_scan) takes CLO_OP_SUMS_TRIP
    = 2048 tile sums of CLO_OP_ENDS_TILE = 4096 counts per trip, 2^23 counts (no getter): this is three trips, and still
    two if a trip were doubled."""
    m = (1 << 24) + 5
    c = (np.random.default_rng(24).random(m) < 1 / 64).astype(np.int64)
    for k in range(0, m, 1 << 20):
        c[max(k - 2, 0):k + 3] = 1
    return c


def test_the_ends_scan_takes_three_trips(dev, TL):
    """The exclusive sums of the tiles of counts carried from trip to trip, in the counts form of all three operations
    that share the scan's body (each has __global__ wrappers of its own): seg_out and rank_out of CloExpand with uint and
    ulong counts and with a num_in just behind the first trip, the sum of ones per segment in CloSegReduce (the counts
    themselves), and CloSegSort in the keys mode."""
    from test_gpu_segreduce import run_seg
    from test_gpu_segsort import run_sort
    counts = ends_scan_counts()
    total = int(counts.sum())
    assert counts.size > 2 << 23 and 200000 < total < 300000
    for ct in ("uint", "ulong"):
        got, _ = run_expand(dev, "counts", ct, 4, (False, True, True), counts, "2^24 + 5 counts")
        assert got == total
    num_in = (1 << 23) + 3
    got, _ = run_expand(dev, "counts", "uint", 4, (False, True, True), counts, "num_in just behind 2^23", num_in=num_in, capacity=total)
    assert got == int(counts[:num_in].sum())
    got, aggr = run_seg(dev, "sum", "counts", "uint", "uint", "uint", counts, total, "2^24 + 5 counts", vals=np.ones(total, np.uint32))
    assert got == total and np.array_equal(aggr, counts.astype(np.uint32))
    got, _, _ = run_sort(dev, "counts", "uint", "ushort", "keys", counts, total, "2^24 + 5 counts", seed=24)
    assert got == total


def test_the_lds_edge(dev, TL):
    """A tile (the second one) with exactly L - 1, L and L + 1 segment ends, of lengths 0 and 1 mixed so that it still
    has T rows; and a run of 2 L + 5 empty segments that ends in the middle of the first tile."""
    T, L = TL
    assert L >= T
    rng = np.random.default_rng(20)
    for i, k in enumerate((L - 1, L, L + 1)):
        mix = np.concatenate((np.ones(T - 2, np.int64), np.zeros(k - T, np.int64)))
        mix = np.concatenate(([1], rng.permutation(mix), [1]))             # its first end lies behind row T, its last on row 2 T
        counts = np.concatenate(([T], mix, [7]))
        for form in FORMS:
            got, _ = run_expand(dev, form, "uint", 4, (True, True, True), counts, "%d ends in one tile" % k, base=77)
            assert got == 2 * T + 7
    counts = np.concatenate(([T // 2 + 3], np.zeros(2 * L + 5, np.int64), [T]))
    for form, ct in (("counts", "ulong"), ("offsets", "uint")):
        run_expand(dev, form, ct, 8, (True, True, True), counts, "2 L + 5 empty segments")
        run_expand(dev, form, ct, 1, (False, True, False), counts, "2 L + 5 empty segments")


@pytest.mark.parametrize("ct", ["uint", "ulong"])
@pytest.mark.parametrize("form", FORMS)
def test_forms_and_sizes(dev, TL, form, ct):
    """Both forms x both count types x value sizes 1, 2, 4, 8 x every non-empty subset of the outputs."""
    T, _ = TL
    counts = counts_of("geometric", 2 * T + 3, T, 5)
    counts[::7] = 0
    for vs in (1, 2, 4, 8):
        for outs in SUBSETS:
            run_expand(dev, form, ct, vs, outs, counts, "every form", base=3)


def test_num_in(dev, TL):
    T, _ = TL
    counts = counts_of("geometric", 3 * T + 9, T, 6)
    m_h = counts.size
    for i, num_in in enumerate((0, 1, m_h // 2, m_h - 1, m_h, m_h + 1, 1 << 40)):
        for form in FORMS:
            want = int(counts[:min(num_in, m_h)].sum())
            got, _ = run_expand(dev, form, ("uint", "ulong")[i % 2], 4, (True, True, True), counts, "num_in %d of %d" % (num_in, m_h),
                                num_in=num_in, capacity=3 * T + 9, base=5 * i)
            assert got == want


def test_capacity(dev, TL):
    """num_out always receives the unclamped total; rows from the capacity on are not written."""
    T, _ = TL
    for total in (T + 1, 3 * T):
        counts = counts_of("sevens", total, T, 0)
        for cap in (0, 1, total - 1, total, total + T):
            for form in FORMS:
                got, seg = run_expand(dev, form, "uint", 2, (True, True, True), counts, "capacity %d of %d" % (cap, total), capacity=cap)
                assert got == total and seg.size == min(cap, total)


def test_offsets_with_a_base(dev, TL):
    T, _ = TL
    counts = counts_of("geometric", 2 * T + 100, T, 8)
    total = int(counts.sum())
    run_expand(dev, "offsets", "uint", 4, (True, True, True), counts, "offsets[0] = 12345", base=12345)
    run_expand(dev, "offsets", "ulong", 4, (True, True, True), counts, "offsets[0] = 2^40 + 12345", base=(1 << 40) + 12345)
    src = source("offsets", "uint", counts, (1 << 32) - 1 - total)
    assert int(src[-1]) == (1 << 32) - 1
    run_expand(dev, "offsets", "uint", 4, (True, True, True), counts, "uint offsets that end at 2^32 - 1", src=src)


def test_chain_sort_reduce_expand(dev, TL):
    """Sort by key, reduce the sorted keys to (key, run length) rows, expand them again with num_in = num_runs_out and
    numel_in = the number of keys: the sorted keys come back. Nothing waits between the three calls."""
    clo, ctx, q = dev
    T, _ = TL
    n = 3 * T + 5
    keys = np.random.default_rng(30).integers(0, 500, n).astype(np.uint32)
    k_r, ks_r, idx_r = Region(dev, 4 * n, 0, keys, 0), Region(dev, 4 * n, 0, None, 1), Region(dev, 4 * n, 0, None, 2)
    rk_r, len_r, runs_r = Region(dev, 4 * n, 0, None, 0), Region(dev, 4 * n, 0, None, 1), Region(dev, 8, 0, None, 2)
    out_r, seg_r, num_r = Region(dev, 4 * n, 0, None, 0), Region(dev, 4 * n, 0, None, 1), Region(dev, 8, 0, None, 2)
    sorter, rbk, ex = clo.Sorter("satradix", ctx, "uint"), clo.ReduceByKey(ctx, "uint", None, "uint"), clo.Expand("counts", ctx, "uint", "uint")
    try:
        assert sorter.by_key_with_device_data(q, k_r.view, None, ks_r.view, idx_r.view, n)
        assert rbk.with_device_data(q, ks_r.view, None, rk_r.view, len_r.view, runs_r.view, n)
        assert ex.with_device_data(q, len_r.view, runs_r.view, rk_r.view, out_r.view, seg_r.view, None, num_r.view, n, n)
        q.finish()
        want = np.sort(keys)
        uniq, first = np.unique(want, return_index=True)
        num_r.check(np.array([n], np.uint64), "num_out")
        runs_r.check(np.array([uniq.size], np.uint64), "num_runs_out")
        out_r.check(want, "run-length decode of the reduced keys")
        seg_r.check(np.searchsorted(uniq, want).astype(np.uint32), "seg_out")
    finally:
        for x in (k_r, ks_r, idx_r, rk_r, len_r, runs_r, out_r, seg_r, num_r, sorter, rbk, ex):
            x.close()


def test_chain_histogram_expand_is_a_counting_sort(dev, TL):
    """The histogram's counts of keys in [0, 4096) expanded over values_in = arange(4096) are the sorted keys: equal to
    clo_sort_* of the same keys."""
    clo, ctx, q = dev
    T, _ = TL
    n, bins = 4 * T + 11, 4096
    keys = (np.random.default_rng(31).integers(0, bins, n) // 3 * 3).astype(np.uint32)     # two of three bins stay empty
    k_r, h_r, v_r = Region(dev, 4 * n, 0, keys, 0), Region(dev, 4 * bins, 0, None, 1), Region(dev, 4 * bins, 0, np.arange(bins, dtype=np.uint32), 2)
    out_r, num_r, sorted_r = Region(dev, 4 * n, 0, None, 0), Region(dev, 8, 0, None, 1), Region(dev, 4 * n, 0, None, 2)
    hist, ex, sorter = clo.Histogram(ctx, "uint"), clo.Expand("counts", ctx, "uint", "uint"), clo.Sorter("satradix", ctx, "uint")
    try:
        assert hist.with_device_data(q, k_r.view, None, h_r.view, n, num_bins=bins)
        assert ex.with_device_data(q, h_r.view, None, v_r.view, out_r.view, None, None, num_r.view, bins, n)
        assert sorter.with_device_data(q, k_r.view, sorted_r.view, n)
        q.finish()
        num_r.check(np.array([n], np.uint64), "num_out")
        got = out_r.base.read(q, np.uint8, out_r.host.size)[out_r.at:out_r.at + 4 * n].copy().view(np.uint32)
        sorted_r.check(got, "the library's sort against the counting sort")
        out_r.check(np.sort(keys), "the counting sort")
    finally:
        for x in (k_r, h_r, v_r, out_r, num_r, sorted_r, hist, ex, sorter):
            x.close()


def test_chain_seg_out_as_keys(dev, TL):
    """seg_out is a key for the by-key operations: its run lengths are the counts that are not 0."""
    clo, ctx, q = dev
    T, _ = TL
    counts = counts_of("geometric", 2 * T + 50, T, 32)
    counts[::3] = 0
    total = int(counts.sum())
    c_r, seg_r, num_r = Region(dev, 4 * counts.size, 0, counts.astype(np.uint32), 0), Region(dev, 4 * total, 0, None, 1), Region(dev, 8, 0, None, 2)
    rk_r, len_r, runs_r = Region(dev, 4 * total, 0, None, 0), Region(dev, 4 * total, 0, None, 1), Region(dev, 8, 0, None, 2)
    ex, rbk = clo.Expand("counts", ctx, None, "uint"), clo.ReduceByKey(ctx, "uint", None, "uint")
    try:
        assert ex.with_device_data(q, c_r.view, None, None, None, seg_r.view, None, num_r.view, counts.size, total)
        assert rbk.with_device_data(q, seg_r.view, None, rk_r.view, len_r.view, runs_r.view, total)
        q.finish()
        kept = np.flatnonzero(counts)
        runs_r.check(np.array([kept.size], np.uint64), "num_runs_out")
        rk_r.check(kept.astype(np.uint32), "the segments that own rows")
        len_r.check(counts[kept].astype(np.uint32), "their counts")
    finally:
        for x in (c_r, seg_r, num_r, rk_r, len_r, runs_r, ex, rbk):
            x.close()


def test_element_aligned_views(dev, TL):
    """Every array one (or three) elements past a 16-byte boundary: nothing may assume more than the element's
    alignment."""
    T, _ = TL
    counts = counts_of("geometric", 2 * T + 37, T, 9)
    counts[5:9] = 0
    cases = (("counts", "uint", 1, (4, 1, 1, 4, 12)), ("offsets", "uint", 2, (12, 2, 6, 12, 4)), ("counts", "ulong", 4, (8, 4, 4, 4, 4)),
             ("offsets", "ulong", 8, (8, 8, 8, 12, 12)), ("counts", "uint", 1, (4, 3, 15, 4, 4)), ("offsets", "uint", 2, (4, 2, 14, 8, 12)))
    for form, ct, vs, offs in cases:
        run_expand(dev, form, ct, vs, (True, True, True), counts, "views at %s" % (offs,), offs=offs, base=9)


def test_two_objects_on_two_queues_and_one_object_moved(dev, TL):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds; then
    one object used on the first queue, the second and the first again (its workspace follows the queue)."""
    clo, ctx, _ = dev
    T, _ = TL
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("counts", "uint", 4), ("offsets", "ulong", 8))
    objs = [clo.Expand(form, ctx, VTYPE[vs], ct) for form, ct, vs in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (form, ct, vs) in enumerate(specs):
                counts = counts_of("geometric", 40 * T + 9 + rnd, T, 10 * rnd + i)
                src, vals = source(form, ct, counts, 7), values_for(vs, counts.size)
                total = int(counts.sum())
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, src.nbytes, 0, src, 0), Region(rdev, vals.nbytes, 0, vals, 1), Region(rdev, total * vs, 0, None, 2),
                        Region(rdev, 4 * total, 0, None, 0), Region(rdev, 4 * total, 0, None, 1), Region(rdev, 8, 0, None, 2)]
                sent.append((src, vals, counts.size, total, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (src, vals, m_h, total, regs) in enumerate(sent):
                assert objs[i].with_device_data(qs[i], regs[0].view, None, regs[1].view, regs[2].view, regs[3].view, regs[4].view, regs[5].view, m_h, total)
            for i in range(2):
                qs[i].finish()
            for i, (src, vals, m_h, total, regs) in enumerate(sent):
                seg, rank, t = expand(specs[i][0], src, total)
                what = "round %d, %s" % (rnd, specs[i][0])
                regs[5].check(np.array([t], np.uint64), what + ": num_out")
                regs[2].check(vals[seg], what + ": values_out")
                regs[3].check(seg, what + ": seg_out")
                regs[4].check(rank, what + ": rank_out")
                for r in regs:
                    r.close()
        for j, qi in enumerate((0, 1, 0, 1)):
            counts = counts_of("geometric", (5, 60, 2, 30)[j] * T + j, T, 40 + j)       # small, large, small, large
            run_expand((clo, ctx, qs[qi]), "counts", "uint", 4, (True, True, True), counts, "moved, call %d" % j, obj=objs[0], q=qs[qi])
    finally:
        for x in objs + qs:
            x.close()


def test_host_data_form(dev, TL):
    clo, ctx, q = dev
    T, _ = TL
    counts = counts_of("geometric", 2 * T + 9, T, 11)
    counts[::5] = 0
    total, qc = int(counts.sum()), clo.Queue(ctx)
    try:
        for form in FORMS:
            for ct, vs in (("uint", 4), ("ulong", 1), ("uint", 8)):
                src, vals = source(form, ct, counts, 4321), values_for(vs, counts.size)
                ex = clo.Expand(form, ctx, VTYPE[vs], ct)
                for cap in (0, total - 5, total, total + 7):
                    for num_in, qe, qcomm in ((None, q, qc), (counts.size // 2, None, None), (counts.size + 9, q, None)):
                        seg, rank, t = expand(form, src, cap, num_in)
                        v, s, r, got = ex.with_host_data(src, cap, values=vals, num_in=num_in, rank=True, q_exec=qe, q_comm=qcomm)
                        what = (form, ct, vs, cap, num_in)
                        assert got == t and np.array_equal(v, vals[seg]) and np.array_equal(s, seg) and np.array_equal(r, rank), what
                v, s, r, got = ex.with_host_data(src, total, seg=False, rank=True, q_exec=q)         # the ranks alone
                assert v is None and s is None and got == total and np.array_equal(r, expand(form, src, total)[1])
                ex.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev, TL):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    T, _ = TL
    m_h, cap = 1000, 3 * T
    need = lib.clo_hip_expand_workspace_bytes(m_h, cap)
    assert need > 0 and need % 256 == 0
    counts = np.random.default_rng(5).integers(0, 9, 2 * m_h + 4, dtype=np.uint32)
    cn, vi, ni = Region(dev, counts.nbytes, 0, counts, 0), Region(dev, 16 * m_h, 0, values_for(8, 2 * m_h), 1), Region(dev, 16, 0, np.array([m_h // 2, 0], np.uint64), 2)
    vo, so, ro = (Region(dev, 8 * cap + 16, 0, None, i) for i in range(3))
    num = Region(dev, 16, 0, None, 0)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(c_p, v_p, vo_p, so_p, ro_p, form=0, cs=4, n_p=None, num_p=num.ptr, numel=m_h, capacity=cap, vs=4, w=ws.ptr, wb=need):
        return lib.clo_hip_expand(form, c_p, cs, n_p, v_p, vo_p, so_p, ro_p, num_p, numel, capacity, vs, w, wb, s)

    try:
        full = (cn.ptr, vi.ptr, vo.ptr, so.ptr, ro.ptr)
        for form in (-1, 2, 100):
            assert call(*full, form=form) == EARGS
        for cs in (0, 1, 2, 3, 16):
            assert call(*full, cs=cs) == EUNSUPPORTED, cs
        for vs in (3, 5, 16, -1):
            assert call(*full, vs=vs) == EUNSUPPORTED, vs
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(*full, n_p=ni.ptr + 4) == EARGS                                                     # num_in misaligned
        assert call(*full, numel=1 << 32) == EARGS and call(*full, capacity=1 << 32) == EARGS
        assert call(None, vi.ptr, vo.ptr, so.ptr, ro.ptr) == EARGS and call(None, None, None, so.ptr, None, form=1, numel=0) == EARGS
        assert call(cn.ptr, None, None, None, None) == EARGS                                            # no output
        assert call(cn.ptr, vi.ptr, None, so.ptr, None) == EARGS and call(cn.ptr, None, vo.ptr, so.ptr, None) == EARGS
        assert call(*full, vs=0) == EARGS                                                               # values with value_size 0
        for i in range(5):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        args = list(full)
        args[0] += 4
        assert call(*args, cs=8) == EARGS                                                               # 4-aligned is not 8-aligned
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        q.finish()
        for r in (vo, so, ro, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; num_in; 8-byte counts over the same bytes read
        # as offsets are not ascending, so that only the status is looked at; numel_in 0 needs no workspace, no input
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        assert call(*full) == 0
        q.finish()
        assert first() == int(counts[:m_h].sum())
        assert call(cn.ptr, None, None, so.ptr, None, n_p=ni.ptr, vs=0) == 0
        q.finish()
        assert first() == int(counts[:m_h // 2].sum())
        assert call(cn.ptr + 4, vi.ptr, vo.ptr, None, None, vs=8, capacity=0) == 0                      # the size query, counts at an odd element
        q.finish()
        assert first() == int(counts[1:m_h + 1].sum())
        assert call(None, None, None, so.ptr, None, numel=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (cn, vi, ni, vo, so, ro, num):
            r.close()


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, TL, form):
    """clo_hip_expand captured from one client stream (a linear graph) after one eager warm-up and replayed three times,
    the counts and num_in rewritten and the outputs and num_out refilled with a canary before each replay (the protocol
    of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the capacity."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    T, _ = TL
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, cap, vs = 900, 4 * T + 3, 4
    need = lib.clo_hip_expand_workspace_bytes(m_h, cap)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, vs * m_h, vs * cap, 4 * cap, 4 * cap, 8, need)]
    src_m, nin_m, vi, vo, so, ro, num, ws = made
    vals = values_for(vs, m_h)
    means = [16, 3, 40, 9, 16]                                              # 900 segments of mean 40: above the capacity
    totals = set()

    def load(r):
        counts = np.random.default_rng(300 + r).geometric(1 / means[r], m_h) - (np.arange(m_h) % 4 == r % 4)
        src, num_in = source(form, "uint", counts, 50 * r), m_h - 100 * (r % 3)
        for m in (vo, so, ro, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (vi, vals)):
            mem_.put(arr)
        want = expand(form, src, cap, num_in)
        totals.add(want[2])
        return want

    def enqueue():
        return lib.clo_hip_expand(FORMS.index(form), src_m.ptr, 4, nin_m.ptr, vi.ptr, vo.ptr, so.ptr, ro.ptr, num.ptr, m_h, cap, vs, ws.ptr, need, q.stream)

    def verify(r, want):
        seg, rank, total = want
        tag = "%s round %d" % (form, r)
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        rest = GC.canary(np.uint32, cap - seg.size)
        GC.same(vo.get(np.uint32, cap), np.concatenate((vals[seg], rest)), tag + ": values_out")
        GC.same(so.get(np.uint32, cap), np.concatenate((seg, rest)), tag + ": seg_out")
        GC.same(ro.get(np.uint32, cap), np.concatenate((rank, rest)), tag + ": rank_out")
        GC.same(vi.get(np.uint32, m_h), vals, "values_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(totals) >= 4 and max(totals) > cap > min(totals), totals
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def test_broken_preconditions_stay_in_bounds(dev, TL):
    """Offsets that descend or are unordered, counts whose sums wrap 2^64, a num_in above numel_in: the call completes,
    the canaries and the inputs are intact, every seg_out value is below numel_in. Contents are not compared: DESIGN.md
    section 20 gives the argument that this holds by construction, and this run shows it once."""
    T, _ = TL
    rng = np.random.default_rng(90)
    m_h, cap = 700, 3 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 20).astype(np.uint32)
    unordered = rng.integers(0, cap, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for form, ct, src in (("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping)):
        run_expand(dev, form, ct, 4, (True, True, True), None, "broken preconditions", capacity=cap, num_in=m_h + 1000, src=src, compare=False)


def test_rows_above_2p31(dev, TL):
    """total = 2^31 + 2^20 + 5 rows of uchar values and seg_out: segments of 5 rows and one of 3 T + 1 rows laid across row
    2^31 (the run structure of test_gpu_above_2p31.py). Counts and values are made on the device, the rows are checked
    there in chunks against the closed form."""
    import torch
    from test_gpu_above_2p31 import CHUNK, N, Runs, as_buffer, chunks
    clo, ctx, q = dev
    if torch.cuda.get_device_properties(0).total_memory < (96 << 30):
        pytest.skip("needs ~60 GiB of device memory")
    T, _ = TL
    runs = Runs(T)
    m = runs.rows
    counts = torch.full((m,), 5, dtype=torch.int32, device="cuda")
    counts[runs.r0] = runs.long
    counts[m - 1] = runs.last
    vals = torch.empty(m, dtype=torch.uint8, device="cuda")
    for lo, hi in chunks(m):
        vals[lo:hi] = (torch.arange(lo, hi, dtype=torch.int64, device="cuda") & 0xff).to(torch.uint8)
    vo = torch.full((N + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    so = torch.full((N + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")                           # bytes A5 A5 A5 A5
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (counts, vals, vo, so, cnt)]
    ex = clo.Expand("counts", ctx, "uchar", "uint")
    try:
        assert ex.with_device_data(q, bufs[0], None, bufs[1], bufs[2], bufs[3], None, bufs[4], m, N)
        q.finish()
        assert int(cnt[0]) == N
        for lo, hi in chunks(N, CHUNK):
            _, r, _ = runs.run_and_start(torch, lo, hi)
            assert bool(((so[lo:hi].to(torch.int64) & 0xFFFFFFFF) == r).all()), "seg_out differs in rows [%d, %d)" % (lo, hi)
            assert bool((vo[lo:hi] == (r & 0xff).to(torch.uint8)).all()), "values_out differs in rows [%d, %d)" % (lo, hi)
        assert bool((vo[N:] == 0xA5).all()) and bool((so[N:] == -0x5A5A5A5B).all()), "rows >= total were written"
    finally:
        for x in bufs + [ex]:
            x.close()
        del counts, vals, vo, so
        torch.cuda.empty_cache()
