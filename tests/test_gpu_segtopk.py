"""CloSegTopK (include/clo_segtopk.h) on the GPU against the numpy model of tests/segtopk_model.py, bit for bit. Every
array is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); keys_out, values_out, counts_out and num_out are pre-filled with the pattern, and after every call
num_out is the model's unclamped total, counts_out[r < m] the model's, the slots j < counts[r] of the rows r < m hold the
model's rows, and the guards, every input, every slot j >= counts[r], every row r >= m and counts_out[r >= m] are
unchanged. Shapes are expressed in T = clo_hip_segtopk_tile and the cap clo_hip_segtopk_k_max: a segment inside one tile
is finished by the tile sort, one that crosses a tile boundary by the combine levels, so the cases are lengths around k,
segments laid on and across tile boundaries with the winners planted on either side, one segment over 2 .. 17 tiles from
tile 0 and from an odd tile with the winners in chosen tiles, two long segments meeting in one tile, ties across tiles,
empty segments (a million of them between two heads), every key type at its extremes x every value mode, clipped totals
and num_in, cross-checks against CloSegSort, CloSegArg and CloTopK, element-aligned views, queues, the host form, the thin
ABI's status codes, a captured graph, broken preconditions (in bounds, contents not compared) and a scribbled workspace."""
import numpy as np
import pytest

from segtopk_model import FORMS, KEY_NP, WHICH, dense, segtopk
from test_gpu_histogram import Region
from test_gpu_segsort import CDT, MODES, VS, geometric_fill, keys_for, rotate, source

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def T(dev):
    clo = dev[0]
    t = clo.segtopk_tile(4, 0)
    assert t >= 1024 and all(clo.segtopk_tile(k, v) == t for k in (1, 2, 4, 8) for v in (0, 4, 8))
    return t


@pytest.fixture(scope="module")
def CAP(dev, T):
    clo = dev[0]
    cap = clo.segtopk_k_max(4, 0)
    assert 256 <= cap <= T and all(clo.segtopk_k_max(k, v) == cap for k in (1, 2, 4, 8) for v in (0, 4, 8))
    return cap


def run_topk(dev, which, form, ct, kt, mode, counts, n, k, what, num_in=None, base=0, offs=(0, 0, 0, 0, 0, 0), obj=None, q=None, src=None,
             compare=True, seed=0, keys=None, distinct=None):
    """One call on views at byte offsets offs = (counts_or_offsets, keys_in, values_in, keys_out, values_out, counts_out)
    with n rows; checks everything and returns (total, idx, counts): the model's rows. src: the input as it is (broken
    preconditions); compare False: the contents are not compared."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = source(form, ct, counts, base)
    m_h = src.size - (1 if form == "offsets" else 0)
    if keys is None:
        keys = keys_for(kt, n, seed, distinct)
    assert keys.size == n and keys.dtype == KEY_NP[kt]
    vs = VS[mode]
    vdt = np.uint64 if vs == 8 else np.uint32
    vals = np.random.default_rng(3000 + seed).integers(0, np.iinfo(vdt).max, n, dtype=vdt) if mode in ("v4", "v8") else None
    idx, cnt, total = segtopk(which, form, src, keys, k, num_in) if compare else (None, None, None)
    what = "%s %d %s %s %s %s n %d, %s" % (which, k, form, ct, kt, mode, n, what)
    ks = keys.dtype.itemsize
    st = obj or clo.SegTopK(which, form, ctx, kt, vs, ct)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0)
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    k_r = Region(rdev, n * ks, offs[1], keys, 1) if n else None
    v_r = Region(rdev, n * vs, offs[2], vals, 2) if vals is not None else None
    ko_r = Region(rdev, m_h * k * ks, offs[3], None, 2) if mode != "arg without keys_out" else None
    vo_r = Region(rdev, m_h * k * vs, offs[4], None, 0) if vs else None
    co_r = Region(rdev, m_h * 4, offs[5], None, 1)
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert st.with_device_data(q, s_r.view, view(n_r), view(k_r), view(v_r), view(ko_r), view(vo_r), co_r.view, num_r.view, m_h, n, k), what
        q.finish()
        if compare:
            m = idx.shape[0]
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            want_c = co_r.contents(np.uint32)
            want_c[:m] = cnt
            co_r.check(want_c, what + ": counts_out")
            for r, col, name in ((ko_r, keys, "keys_out"), (vo_r, np.arange(n, dtype=np.uint32) if vals is None else vals, "values_out")):
                if r is None:
                    continue
                want = r.contents(col.dtype).reshape(m_h, k)                 # what is not written keeps the pattern
                want[:m] = dense(idx, col, want[:m])
                got = r.base.read(q, np.uint8, r.host.size)[r.at:r.at + r.n].view(col.dtype).reshape(m_h, k)
                bad = np.flatnonzero((got.view("u%d" % col.dtype.itemsize) != want.view("u%d" % col.dtype.itemsize)).any(axis=1))
                assert bad.size == 0, "%s: %d of %d segments of %s differ, first %d: got %s, want %s (model rows %s)" % (
                    what, bad.size, m_h, name, bad[0], got[bad[0]][:8], want[bad[0]][:8], idx[bad[0]][:8] if bad[0] < m else None)
                r.check(want.reshape(-1), what + ": " + name)                # ... and the guards
        else:                                                                # in bounds: the guards
            for r in (ko_r, vo_r, co_r, num_r):
                if r is not None:
                    now = r.base.read(q, np.uint8, r.host.size)[r.at:r.at + r.n].copy()
                    r.check(now, what)
        s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if k_r:
            k_r.check(keys, what + ": keys_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return total, idx, cnt
    finally:
        for r in (s_r, n_r, k_r, v_r, ko_r, vo_r, co_r, num_r):
            if r:
                r.close()
        if obj is None:
            st.close()


def planted(which, n, rows, seed=0):
    """n uint keys whose winners for `which` are exactly `rows` (any order among them): the others lie in the middle of
    the range, the planted rows at its end."""
    rng = np.random.default_rng(5000 + seed)
    keys = rng.integers(1 << 20, 1 << 31, n, dtype=np.uint32)
    rows = np.asarray(rows, np.int64)
    win = rng.integers(0, 1 << 20, rows.size, dtype=np.uint32)
    keys[rows] = ~win if which == "largest" else win
    return keys


@pytest.mark.parametrize("k_name", ("1", "2", "3", "8", "63", "64", "65", "cap"))
def test_lengths_around_k(dev, T, CAP, k_name):
    """Segments of 0, 1, k - 1, k, k + 1 and 2 k rows, twice and in two orders, at every which, form and count type: the
    count written is min(k, len) and the slots behind it keep the pattern. With k = cap the twelve segments span several
    tiles, so that segments of k + 1 and 2 k rows cross tile boundaries."""
    k = CAP if k_name == "cap" else int(k_name)
    lens = [0, 1, k - 1, k, k + 1, 2 * k]
    counts = np.array(lens + lens[::-1])
    n = int(counts.sum())
    case = 0
    for which in WHICH:
        for form in FORMS:
            for ct in CDT:
                kt, mode = rotate(case + k)[2:]
                run_topk(dev, which, form, ct, kt, mode, counts, n, k, "lengths around k", base=case, seed=case, distinct=(None, 5)[case % 2])
                case += 1


def test_segments_that_end_around_a_tile_boundary(dev, T):
    """A segment that ends at T - 1, T and T + 1 (and the next one starting there), and a tile that is wholly the inside
    of one segment."""
    for case, end in enumerate((T - 1, T, T + 1)):
        counts = np.array([end - 40, 40, 9, T - 9])
        for which in WHICH:
            run_topk(dev, which, "counts", "uint", "int", "v4", counts, int(counts.sum()), 16, "a segment ends at %d" % end, seed=case, distinct=6)
    counts = np.array([T // 2, 2 * T, T // 2])                               # tile 1 lies inside the second segment
    for which in WHICH:
        run_topk(dev, which, "offsets", "uint", "float", "arg", counts, 3 * T, 8, "a tile inside a segment", base=5, seed=7)


@pytest.mark.parametrize("where", ("left", "right", "split"))
def test_one_boundary_with_the_winners_on_either_side(dev, T, where):
    """A segment [T - 300, T + 200) among short ones; its k = 12 best rows are all left of the boundary, all right of
    it, or six and six."""
    rng = np.random.default_rng(21)
    counts = np.concatenate((geometric_fill(rng, T - 300), [500], geometric_fill(rng, T - 200)))
    n = 2 * T
    left, right = np.arange(T - 290, T - 10, 23)[:12], np.arange(T + 3, T + 190, 15)[:12]
    rows = {"left": left, "right": right, "split": np.concatenate((left[:6], right[:6]))}[where]
    for which in WHICH:
        keys = planted(which, n, rows, 3)
        total, idx, cnt = run_topk(dev, which, "counts", "uint", "uint", "v4", counts, n, 12, "winners " + where, keys=keys)
        r = int(np.flatnonzero(counts == 500)[0])
        assert sorted(idx[r]) == sorted(rows) and cnt[r] == 12


LONG_TILES = (2, 3, 4, 5, 7, 8, 9, 17)


def long_counts(T, a, w, seed=0, full=False):
    """Short segments, then ONE segment from the middle of tile a over w tiles — to a third of tile a + w - 1, or (full)
    to its very end, so that the segment ends on a tile boundary — then short segments for the rest of that tile and
    half of the next: (counts, the segment's number, its first row, its end)."""
    rng = np.random.default_rng(6000 + seed)
    s, e = a * T + T // 2, (a + w - 1) * T + (T if full else T // 3)
    before, after = geometric_fill(rng, s, 40), geometric_fill(rng, (a + w) * T + T // 2 - e, 40)
    return np.concatenate((before, [e - s], after)), before.size, s, e


@pytest.mark.parametrize("w", LONG_TILES)
@pytest.mark.parametrize("a", (0, 3))
@pytest.mark.parametrize("last", ("partial", "full"))
def test_the_combine_tree(dev, T, CAP, last, a, w):
    """One segment over w tiles starting in tile a, short segments before and after it; its last tile is partial, or
    full (the segment ends on a tile boundary). Its k = 8 winners lie all in the last tile, all in one middle tile, or
    anywhere (k = cap, random keys); and with k = max(8, w) one winner lies in every tile of the tree, the deepest too."""
    counts, r, s, e = long_counts(T, a, w, seed=w, full=last == "full")
    n = int(counts.sum())
    tiles = np.arange(a, a + w)
    assert (e - 1) // T - s // T + 1 == w and (e % T == 0) == (last == "full")
    lo = lambda t: max(s, t * T)
    hi = lambda t: min(e, (t + 1) * T)
    spots = {"the last tile": (8, np.arange(lo(tiles[-1]) + 1, hi(tiles[-1]), 7)[:8]),
             "one middle tile": (8, np.arange(lo(tiles[w // 2]) + 5, hi(tiles[w // 2]), 11)[:8]),
             "one per tile": (max(8, w), np.array([lo(t) + (37 * i) % (hi(t) - lo(t)) for i, t in enumerate(tiles)]))}
    case = 0
    for name, (k, rows) in spots.items():
        for which in WHICH:
            form, ct, _, mode = rotate(case + w)
            keys = planted(which, n, rows, case)
            total, idx, cnt = run_topk(dev, which, form, ct, "uint", mode, counts, n, k, "%d tiles from tile %d, last %s, winners in %s" % (w, a, last, name),
                                       keys=keys, base=case)
            assert total == n and rows.size <= k and sorted(idx[r][:rows.size]) == sorted(rows), name
            case += 1
    for which in WHICH:                                                       # lists of the full length, ties among them
        run_topk(dev, which, "counts", "uint", ("ushort", "double")[a > 0], "v8", counts, n, CAP, "%d tiles from tile %d, k = cap" % (w, a), seed=w, distinct=(900, None)[w % 2])


def test_two_long_segments_meet_in_one_tile(dev, T):
    """Segment X ends and segment Y begins in the middle of tile 4: both candidate slots of that tile are used, and in
    level 0 it is a source for X and a destination for Y."""
    counts = np.array([10, 4 * T + T // 2 - 10, 3 * T + 100, T // 2 - 100])
    n = int(counts.sum())
    for case, which in enumerate(WHICH):
        for k, kt in ((5, "int"), (300, "uchar"), (64, "long")):
            run_topk(dev, which, ("counts", "offsets")[case], "uint", kt, MODES[(case + k) % len(MODES)], counts, n, k, "two long segments", seed=k, base=3)
    counts = np.array([T // 2, T, T, T, T // 2])                              # every boundary inside a segment, every tile with A and B
    for which in WHICH:
        run_topk(dev, which, "counts", "ulong", "float", "arg", counts, 4 * T, 33, "segments of T rows, half a tile off", seed=2)


def test_ties_across_tiles(dev, T):
    """All keys equal over 5 tiles, and 8 distinct keys over 9 tiles: for both which the rows chosen are the lowest
    indices, in ascending index order."""
    for which in WHICH:
        n = 5 * T - 17
        keys = np.full(n, 77, np.uint32)
        total, idx, cnt = run_topk(dev, which, "counts", "uint", "uint", "arg", [3, n - 3], n, 100, "one key", keys=keys)
        assert list(idx[0][:3]) == [0, 1, 2] and np.array_equal(idx[1], np.arange(3, 103))
        n = 9 * T
        keys = keys_for("int", n, 4, distinct=8)
        total, idx, cnt = run_topk(dev, which, "counts", "uint", "int", "v4", [n], n, 700, "8 keys", keys=keys)
        best = keys.max() if which == "largest" else keys.min()
        first = np.flatnonzero(keys == best)[:700]
        assert np.array_equal(idx[0][:first.size], first) and (np.diff(idx[0][:first.size]) > 0).all()


def test_empty_segments(dev, T):
    """Empty segments inside one tile (the segment number of every piece), leading and trailing ones, half of all, and
    2^20 of them between two heads."""
    pat = np.array([3, 0, 0, 5, 0, 1, 0, 0, 0, 7, 2, 0])
    for case, counts in enumerate((pat, np.tile(pat, 40), np.concatenate((np.zeros(9, np.int64), pat, np.zeros(300, np.int64))),
                                   np.concatenate(([0, 0, T + 5, 0], pat, [0, 2 * T, 0, 0])))):
        for which in WHICH:
            form, ct, kt, mode = rotate(case + 3)
            run_topk(dev, which, form, ct, kt, mode, counts, int(counts.sum()), 4, "empty segments, pattern %d" % case, seed=case, base=case)
    rng = np.random.default_rng(31)
    counts = rng.geometric(1 / 20, 700)
    counts[rng.random(700) < 0.5] = 0
    run_topk(dev, "smallest", "counts", "uint", "half", "v4", counts, int(counts.sum()), 6, "half of the segments empty", seed=5)
    counts = np.concatenate(([9], np.zeros(1 << 20, np.int64), [T + 3]))
    for form in FORMS:
        total, idx, cnt = run_topk(dev, "largest", form, "uint", "uint", "arg", counts, T + 12, 2, "2^20 empty segments", seed=6)
        assert cnt[0] == 2 and cnt[-1] == 2 and not cnt[1:-1].any()


def special_keys(kt, n, seed):
    """Any bit patterns, with the type's extremes (floats: both zeros, both infinities, NaNs of both signs with several
    payloads) in a quarter of the rows."""
    rng = np.random.default_rng(7000 + seed)
    dt = np.dtype(KEY_NP[kt])
    ut = np.dtype("u%d" % dt.itemsize)
    keys = keys_for(kt, n, seed).view(ut).copy()
    top = np.iinfo(ut).max
    sign = ut.type(1 << (8 * dt.itemsize - 1))
    if dt.kind == "f":
        inf = np.array([np.inf], dt).view(ut)[0]
        special = np.array([0, sign, inf, inf | sign, inf + 1, (inf + 1) | sign, inf + 5, (inf + 5) | sign, top, top >> 1], ut)
    else:
        special = np.array([0, top, sign, sign - 1, 1, top - 1], ut)
    at = rng.random(n) < 0.25
    keys[at] = special[rng.integers(0, special.size, int(at.sum()))]
    return keys.view(dt)


@pytest.mark.parametrize("kt", tuple(KEY_NP))
def test_key_types_at_their_extremes_and_every_value_mode(dev, T, kt):
    """Every key type x every value mode x both which: segments of mean 30 with one of 2 T + 9 rows among them, the
    extremes of the type in a quarter of the rows, so that ties at the ends of the order are frequent."""
    rng = np.random.default_rng(41)
    counts = np.concatenate((geometric_fill(rng, T - 50, 30), [2 * T + 9], geometric_fill(rng, 600, 30)))
    n = int(counts.sum())
    for i, mode in enumerate(MODES):
        for j, which in enumerate(WHICH):
            keys = special_keys(kt, n, i)
            run_topk(dev, which, FORMS[(i + j) % 2], ("uint", "ulong")[i % 2], kt, mode, counts, n, (7, 40)[j], "extremes", keys=keys, base=i, seed=i)


def test_totals_and_num_in(dev, T):
    """total > numel (clipping, reported in num_out), rows behind the total, num_in below, at and above numel_seg, and
    offsets whose first entry is not 0."""
    rng = np.random.default_rng(51)
    counts = np.concatenate((geometric_fill(rng, T + 300, 25), [T + 50], geometric_fill(rng, 500, 25)))
    total = int(counts.sum())
    case = 0
    for n in (total, total - 7, total - T, T // 2, total + 100, 0):
        for num_in in (None, counts.size // 2, counts.size, counts.size + 50, 1, 0):
            form, ct, kt, mode = rotate(case)
            got, idx, cnt = run_topk(dev, WHICH[case % 2], form, ct, kt, mode, counts, n, 9, "n %d of %d, num_in %s" % (n, total, num_in),
                                     num_in=num_in, base=1000 * case, seed=case)
            if num_in is None:
                assert got == total
            case += 1


def test_against_segsort_segarg_and_topk(dev, T):
    """The same input through what exists: CloSegSort sliced to k per segment on the host; CloSegArg ("first") at k = 1
    for both which; CloTopK with order "sorted" for a single segment."""
    clo, ctx, q = dev
    rng = np.random.default_rng(61)
    counts = np.concatenate((geometric_fill(rng, T, 20), [0, 3 * T + 1, 0], geometric_fill(rng, 900, 20)))
    n, k = int(counts.sum()), 5
    c32 = counts.astype(np.uint32)
    keys = keys_for("float", n, 3, distinct=40)
    ss, st = clo.SegSort("counts", ctx, "float", 4, "uint"), clo.SegTopK("smallest", "counts", ctx, "float", 4, "uint")
    try:
        sk, sv, total = ss.with_host_data(c32, keys)                          # the arg form: sv the row indices
        tk, tv, tc, total2 = st.with_host_data(c32, keys, k, fill=0xA5A5A5A5)
        assert total == total2 == n
        ends = np.cumsum(counts)
        for r in range(counts.size):
            c = min(k, int(counts[r]))
            s = int(ends[r] - counts[r])
            assert tc[r] == c and np.array_equal(tv[r, :c], sv[s:s + c]) and np.array_equal(tk[r, :c].view(np.uint32), sk[s:s + c].view(np.uint32)), r
            assert (tv[r, c:] == 0xA5A5A5A5).all()
    finally:
        ss.close()
        st.close()
    for which, op in zip(WHICH, ("argmin", "argmax")):
        sa, st = clo.SegArg(op, "first", "counts", ctx, "float", "uint"), clo.SegTopK(which, "counts", ctx, "float", 4, "uint")
        try:
            ai, av, _ = sa.with_host_data(c32, keys)
            tk, tv, tc, _ = st.with_host_data(c32, keys, 1)
            full = counts > 0
            assert np.array_equal(tc, full.astype(np.uint32)) and np.array_equal(tv[full, 0], ai[full]) and \
                np.array_equal(tk[full, 0].view(np.uint32), av[full].view(np.uint32)), which
        finally:
            sa.close()
            st.close()
    for which in WHICH:
        n1 = 6 * T + 11
        keys = keys_for("int", n1, 9, distinct=300)
        tp, st = clo.TopK(which, "sorted", ctx, "int", 4), clo.SegTopK(which, "offsets", ctx, "int", 4, "ulong")
        try:
            want_k, want_v = tp.with_host_data(keys, 200)[:2]
            tk, tv, tc, _ = st.with_host_data(np.array([70, 70 + n1], np.uint64), keys, 200)
            assert tc[0] == 200 and np.array_equal(tk[0], want_k) and np.array_equal(tv[0], want_v), which
        finally:
            tp.close()
            st.close()


def test_element_aligned_views(dev, T):
    """Every array one (or three) elements past a 16-byte boundary: nothing may assume more than the element's
    alignment."""
    c = np.random.default_rng(13).geometric(1 / 16, 90)
    c[5:9] = 0
    c[40] = 2 * T + 37
    n = int(c.sum())
    cases = (("counts", "uint", "uint", "v4", (4, 4, 4, 12, 4, 4)), ("offsets", "uint", "ushort", "arg", (12, 2, 0, 6, 12, 12)),
             ("counts", "ulong", "double", "v8", (8, 8, 8, 8, 8, 4)), ("offsets", "ulong", "uchar", "keys", (8, 1, 0, 3, 0, 8)),
             ("counts", "uint", "float", "arg without keys_out", (12, 12, 0, 0, 4, 12)), ("offsets", "uint", "long", "v4", (4, 8, 12, 8, 4, 4)))
    for i, (form, ct, kt, mode, offs) in enumerate(cases):
        run_topk(dev, WHICH[i % 2], form, ct, kt, mode, c, n, (3, 50)[i % 2], "views at %s" % (offs,), offs=offs, base=9, seed=i)


def test_two_runs_are_identical_and_the_object_moves_to_a_second_queue(dev, T):
    clo, ctx, q = dev
    q2 = clo.Queue(ctx)
    obj = clo.SegTopK("largest", "counts", ctx, "uint", 4, "uint")
    try:
        c = np.random.default_rng(12).geometric(1 / 700, 30)
        c[3], c[20] = 4 * T + 1, 0
        n = int(c.sum())
        first = run_topk(dev, "largest", "counts", "uint", "uint", "v4", c, n, 20, "first run", obj=obj, distinct=8)
        again = run_topk(dev, "largest", "counts", "uint", "uint", "v4", c, n, 20, "second run", obj=obj, distinct=8)
        assert np.array_equal(first[1], again[1])
        for j, qq in enumerate((q2, q, q2)):
            total = (9, 2, 6)[j] * T + j                                      # large, small, large: the workspace follows the queue
            cj = np.array([total // 3, 0, total - total // 3])
            run_topk((clo, ctx, qq), "largest", "counts", "uint", "uint", "v4", cj, total, (4, 900, 77)[j], "moved, call %d" % j, obj=obj, q=qq, seed=j)
    finally:
        obj.close()
        q2.close()


def test_two_objects_on_two_queues(dev, T):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds."""
    clo, ctx, _ = dev
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("smallest", "counts", "uint", "uint", 4, 10), ("largest", "offsets", "ulong", "double", 0, 130))
    objs = [clo.SegTopK(which, form, ctx, kt, vs, ct) for which, form, ct, kt, vs, k in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (which, form, ct, kt, vs, k) in enumerate(specs):
                rng = np.random.default_rng(50 + 10 * rnd + i)
                n = 12 * T + 9 + rnd
                counts = np.concatenate((geometric_fill(rng, 3 * T + 100 * i), [(3 + 2 * i + rnd) * T + 3], geometric_fill(rng, n, 300)))
                counts[::9] = 0
                src, keys = source(form, ct, counts, 7), keys_for(kt, n, rnd, (None, 8)[rnd % 2])
                m_h = src.size - (form == "offsets")
                rdev = (clo, ctx, qs[i])
                ks = keys.dtype.itemsize
                regs = [Region(rdev, src.nbytes, 0, src, 0), Region(rdev, keys.nbytes, 0, keys, 1), Region(rdev, m_h * k * ks, 0, None, 2),
                        Region(rdev, m_h * k * 4, 0, None, 0) if vs else None, Region(rdev, m_h * 4, 0, None, 2), Region(rdev, 8, 0, None, 1)]
                sent.append((src, keys, m_h, n, regs))
            for i in range(2):
                qs[i].finish()                                                # the uploads; from here on nothing waits
            for i, (src, keys, m_h, n, regs) in enumerate(sent):
                view = lambda r: r.view if r is not None else None
                assert objs[i].with_device_data(qs[i], regs[0].view, None, regs[1].view, None, regs[2].view, view(regs[3]), regs[4].view, regs[5].view,
                                                m_h, n, specs[i][5])
            for i in range(2):
                qs[i].finish()
            for i, (src, keys, m_h, n, regs) in enumerate(sent):
                which, form, ct, kt, vs, k = specs[i]
                idx, cnt, t = segtopk(which, form, src, keys, k)
                what = "round %d, %s" % (rnd, form)
                regs[5].check(np.array([t], np.uint64), what + ": num_out")
                regs[4].check(cnt, what + ": counts_out")
                regs[2].check(dense(idx, keys, regs[2].contents(keys.dtype).reshape(m_h, k)).reshape(-1), what + ": keys_out")
                if vs:
                    regs[3].check(dense(idx, np.arange(n, dtype=np.uint32), regs[3].contents(np.uint32).reshape(m_h, k)).reshape(-1), what + ": values_out")
                for r in regs:
                    if r:
                        r.close()
    finally:
        for x in objs + qs:
            x.close()


def test_host_data_form(dev, T):
    clo, ctx, q = dev
    c = np.random.default_rng(14).geometric(1 / 60, 50)
    c[::5] = 0
    c[11] = T + 77
    total = int(c.sum())
    for form in FORMS:
        for which, kt, vs, ct in (("smallest", "int", 0, "uint"), ("largest", "float", 4, "ulong"), ("smallest", "ulong", 8, "uint")):
            src = source(form, ct, c, 4321)
            st = clo.SegTopK(which, form, ctx, kt, vs, ct)
            try:
                for n in (0, total - 5, total, total + 7):
                    keys = keys_for(kt, n, n)
                    vals = np.arange(n, dtype=np.uint64 if vs == 8 else np.uint32) * 3 if vs else None
                    for k, num_in, qe in ((4, None, q), (70, c.size // 2, None), (1, c.size + 9, q), (0, None, q)):
                        idx, cnt, t = segtopk(which, form, src, keys, k, num_in)
                        ko, vo, co, got = st.with_host_data(src, keys, k, vals, num_in=num_in, q_exec=qe, fill=0x5A)
                        what = (form, kt, n, k, num_in)
                        assert got == t and ko.shape == idx.shape, what
                        assert np.array_equal(co, cnt) if k else True, what
                        assert np.array_equal(ko.view(np.uint8), dense(idx, keys, ko.dtype.type(0x5A) if ko.dtype.kind != "f" else np.array(0x5A).astype(ko.dtype)).view(np.uint8)), what
                        assert vo is None if not vs else np.array_equal(vo, dense(idx, vals, 0x5A)), what
                if vs == 4:                                                   # the arg form, with and without keys_out
                    keys = keys_for(kt, total, 1)
                    idx, cnt, t = segtopk(which, form, src, keys, 6)
                    for with_keys in (True, False):
                        ko, vo, co, got = st.with_host_data(src, keys, 6, keys_out=with_keys, fill=-1)   # all ones as uint32
                        assert got == t and (ko is None) == (not with_keys) and np.array_equal(co, cnt)
                        assert np.array_equal(vo.astype(np.int64), np.where(idx >= 0, idx, 0xFFFFFFFF)), (form, with_keys)
            finally:
                st.close()


def thin_table(T, CAP, INT):
    """(what, changes to the good call, status): every refusal of clo_hip_segtopk itself, one bad argument at a time."""
    E, U, W = -1, -2, -3
    return (("which 2", dict(which=2), E), ("which -1", dict(which=-1), E), ("form 2", dict(form=2), E),
            ("count size 2", dict(cs=2), U), ("key type 11", dict(kt=11), U), ("key type -1", dict(kt=-1), U), ("value size 2", dict(vs=2), U),
            ("numel_seg 2^32", dict(m_h=1 << 32), E), ("numel 2^32", dict(n=1 << 32), E), ("k above the cap", dict(k=CAP + 1), E),
            ("numel_seg * k = 2^32", dict(m_h=1 << 24, k=256), E),
            ("no counts", dict(cn=None), E), ("no keys_in", dict(ki=None), E), ("values with value size 0", dict(vs=0), E),
            ("no values_out", dict(vo=None), E), ("no values_in with 8-byte values", dict(vs=8, vi=None), E),
            ("no keys_out with values_in", dict(ko=None), E), ("no counts_out", dict(co=None), E), ("no num_out", dict(num=None), E),
            ("num_out misaligned", dict(num=4), E), ("num_in misaligned", dict(ni=4), E), ("counts_out misaligned", dict(co=2), E),
            ("counts misaligned", dict(cn=2), E), ("keys_in misaligned", dict(ki=2), E), ("keys_out misaligned", dict(ko=1), E),
            ("values_in misaligned", dict(vi=2), E), ("values_out misaligned", dict(vo=3), E),
            ("no workspace", dict(ws=None), E), ("workspace misaligned", dict(ws=128), E), ("workspace one byte short", dict(wsb=-1), W))


ORDER = ("which", "form", "cn", "cs", "ni", "ki", "vi", "ko", "vo", "co", "num", "m_h", "n", "k", "kt", "vs", "ws", "wsb")


def test_thin_abi_status_codes_and_a_scribbled_workspace(dev, T, CAP):
    """Every refusal of clo_hip_segtopk itself, one bad argument at a time (an integer for a pointer: that many bytes
    past the good one), leaves the outputs alone; then calls that must work, on a workspace filled with ones before
    each, against the model: nothing depends on what the workspace held."""
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    rng = np.random.default_rng(71)
    counts = np.concatenate((geometric_fill(rng, T - 9, 30), [0, 2 * T + 100, 0], geometric_fill(rng, 400, 30))).astype(np.uint32)
    m_h, n, k = counts.size, int(counts.sum()), 24
    keys, vals = keys_for("int", n, 1, 60), rng.integers(0, 1 << 32, n, dtype=np.uint32)
    offsets = source("offsets", "uint", counts, 77)
    need = lib.clo_hip_segtopk_workspace_bytes(m_h, n, k, 4, 4)
    assert need % 256 == 0 and need >= n * 5
    cn, of, ki, vi = Region(dev, counts.nbytes, 0, counts, 0), Region(dev, offsets.nbytes, 0, offsets, 0), Region(dev, keys.nbytes, 0, keys, 1), Region(dev, vals.nbytes, 0, vals, 2)
    ni = Region(dev, 16, 0, np.array([m_h - 3, 0], np.uint64), 2)
    ko, vo, co, num = Region(dev, m_h * k * 4, 0, None, 0), Region(dev, m_h * k * 4, 0, None, 1), Region(dev, m_h * 4, 0, None, 2), Region(dev, 16, 0, None, 2)
    ws = clo.Buffer(ctx, need + 512)
    INT = clo.CLO_TYPES["int"]
    good = dict(which=0, form=0, cn=cn.ptr, cs=4, ni=ni.ptr, ki=ki.ptr, vi=vi.ptr, ko=ko.ptr, vo=vo.ptr, co=co.ptr, num=num.ptr, m_h=m_h, n=n, k=k,
                kt=INT, vs=4, ws=ws.ptr, wsb=need)
    call = lambda kw: lib.clo_hip_segtopk(*[kw[x] for x in ORDER], q.stream)
    try:
        for what, change, status in thin_table(T, CAP, INT):
            kw = dict(good)
            for name, v in change.items():
                kw[name] = (good[name] + v if v is not None and name in ("cn", "ni", "ki", "vi", "ko", "vo", "co", "num", "ws", "wsb") else v)
            assert call(kw) == status, what
        q.finish()
        for r in (ko, vo, co, num):
            r.check(None, "a refused thin call wrote")
        case = 0
        for which in (0, 1):
            for form, src_r, src in ((0, cn, counts), (1, of, offsets)):
                for num_in in (None, ni.ptr):
                    for arg in (False, True):
                        ws.write(q, np.full(need + 512, 0xFF, np.uint8))     # scribbled
                        for r in (ko, vo, co, num):
                            r.base.write(q, r.host)
                        kw = dict(good, which=which, form=form, cn=src_r.ptr, ni=num_in, vi=None if arg else vi.ptr, ko=None if arg and case % 2 else ko.ptr)
                        assert call(kw) == 0, kw
                        q.finish()
                        idx, cnt, total = segtopk(WHICH[which], FORMS[form], src, keys, k, None if num_in is None else m_h - 3)
                        m = idx.shape[0]
                        num.check(np.array([total], np.uint64), "num_out")
                        want_c = co.contents(np.uint32)
                        want_c[:m] = cnt
                        co.check(want_c, "counts_out")
                        for r, col, on in ((ko, keys, kw["ko"] is not None), (vo, np.arange(n, dtype=np.uint32) if arg else vals, True)):
                            want = r.contents(col.dtype).reshape(m_h, k)
                            if on:
                                want[:m] = dense(idx, col, want[:m])
                            r.check(want.reshape(-1), "thin call %s" % (kw,))
                        case += 1
        # k = 0 writes num_out alone; numel_seg = 0 writes 0 and needs no workspace
        for r in (ko, vo, co, num):
            r.base.write(q, r.host)
        assert call(dict(good, k=0, co=None)) == 0
        q.finish()
        num.check(np.array([int(counts[:m_h - 3].sum())], np.uint64), "k = 0: num_out")   # (num_in leaves m_h - 3 segments)
        for r in (ko, vo, co):
            r.check(None, "k = 0 wrote an output")
        assert call(dict(good, m_h=0, ws=None, wsb=0, cn=None)) == 0
        q.finish()
        num.check(np.array([0], np.uint64), "numel_seg = 0: num_out")
        for r in (cn, of, ki, vi, ni):
            r.check(r.contents(np.uint8), "an input changed")
    finally:
        ws.close()
        for r in (cn, of, ki, vi, ni, ko, vo, co, num):
            r.close()


def test_broken_preconditions_stay_in_bounds(dev, T, CAP):
    """Offsets that descend or are unordered, counts whose sums wrap 2^64, a num_in above numel_seg: the call completes,
    the canaries and the inputs are intact. Contents are not compared: the header of clo_hip_segtopk.hip gives the
    argument that this holds by construction (every index is clamped where it is used), and this run shows it once."""
    rng = np.random.default_rng(90)
    m_h, n = 3 * T + 700, 5 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 4).astype(np.uint32)
    unordered = rng.integers(0, 2 * n, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for i, (form, ct, src) in enumerate((("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping))):
        for mode, k in (("v4", 3), ("arg without keys_out", 100), ("v8", 17)):
            run_topk(dev, WHICH[i % 2], form, ct, "uint", mode, None, n, k, "broken preconditions", num_in=m_h + 1000, src=src, compare=False, seed=i)


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, T, form):
    """clo_hip_segtopk captured from one client stream (a linear graph) after one eager warm-up and replayed three times,
    the counts, num_in, the keys and the values rewritten and the outputs refilled with a canary before each replay (the
    protocol of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the rows."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, n, k = 60, 4 * T + 3, 10
    need = lib.clo_hip_segtopk_workspace_bytes(m_h, n, k, 4, 4)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, 4 * n, 4 * n, 4 * m_h * k, 4 * m_h * k, 4 * m_h, 8, need)]
    src_m, nin_m, ki, vi, ko, vo, co, num, ws = made
    means = [140, 30, 300, 90, 140]                                          # 60 segments of mean 300: above the rows
    totals = set()
    INT = clo.CLO_TYPES["int"]

    def load(r):
        counts = np.random.default_rng(300 + r).geometric(1 / means[r], m_h) * (np.arange(m_h) % 4 != r % 4)
        counts[(7 * r) % m_h] += 2 * T
        src, num_in = source(form, "uint", counts, 50 * r), m_h - 10 * (r % 3)
        keys = keys_for("int", n, r, 50)
        vals = np.random.default_rng(r).integers(0, 1 << 32, n, dtype=np.uint32)
        for m in (ko, vo, co, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (ki, keys), (vi, vals)):
            mem_.put(arr)
        want = segtopk("largest", form, src, keys, k, num_in)
        totals.add(want[2])
        return want, keys, vals

    def enqueue():
        return lib.clo_hip_segtopk(1, FORMS.index(form), src_m.ptr, 4, nin_m.ptr, ki.ptr, vi.ptr, ko.ptr, vo.ptr, co.ptr, num.ptr, m_h, n, k, INT, 4,
                                   ws.ptr, need, q.stream)

    def verify(r, want):
        (idx, cnt, total), keys, vals = want
        tag = "%s round %d" % (form, r)
        m = idx.shape[0]
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        GC.same(co.get(np.uint32, m_h), np.concatenate((cnt, GC.canary(np.uint32, m_h - m))), tag + ": counts_out")
        for mem_, col, name in ((ko, keys, "keys_out"), (vo, vals, "values_out")):
            want_rows = GC.canary(col.dtype, m_h * k).reshape(m_h, k)
            want_rows[:m] = dense(idx, col, want_rows[:m])
            GC.same(mem_.get(col.dtype, m_h * k), want_rows.reshape(-1), tag + ": " + name)
        GC.same(ki.get(np.int32, n), keys, "keys_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(totals) >= 4 and max(totals) > n > min(totals), totals
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()
