"""CloSegSort (include/clo_segsort.h) on the GPU against the numpy model of tests/segsort_model.py, bit for bit. Every
array is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); keys_out, values_out and num_out are pre-filled with the pattern, and after every call num_out is
the model's unclamped total, the min(total, n) rows written equal the model's, and the guards, every input and every row
at index >= min(total, n) are unchanged. Shapes are expressed in T = clo_hip_segsort_tile, the rows a work-group sorts on
chip: a segment inside one tile is finished by the tile sort, one that crosses a tile boundary by the merge passes, which
ping-pong between the outputs and the workspace, so the cases are single segments of tile counts of both parities,
segments laid on, before and across tile and pair boundaries, empty segments, clipped totals, num_in, both forms and count
types, every key type x every value mode, floating-point zeros and NaNs, few distinct keys (stability), offsets that do
not ascend (in bounds, contents not compared), repeated runs, two queues, element-aligned views, a captured graph, the
host form and a seeded fuzz. Above ten tiles: single segments of 16 to 513 tiles (4 to 10 merge passes), 33 T + 5 rows of one
key, segments whose move masks are pinned (gaps of one to six passes at rest; tests/test_segsort_cpu.py shows the masks on
the CPU), 300 T rows of long segments end to end; the thin ABI's refusals in the order clo_hip_segsort makes them (the
table the host stub answers too); two objects on two queues; the chain expand -> segmented sort -> segmented min and max
without a host wait; and rows above 2^31 checked on the device."""
import numpy as np
import pytest

from segsort_model import FORMS, KEY_NP, segsort
from test_gpu_histogram import Region

pytestmark = pytest.mark.gpu

CDT = {"uint": np.uint32, "ulong": np.uint64}
MODES = ("keys", "v4", "v8", "arg", "arg without keys_out")
VS = {"keys": 0, "v4": 4, "v8": 8, "arg": 4, "arg without keys_out": 4}


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def T(dev):
    clo = dev[0]
    t = clo.segsort_tile(4, 0)
    assert t >= 1024 and all(clo.segsort_tile(k, v) == t for k in (1, 2, 4, 8) for v in (0, 4, 8))
    return t


def keys_for(kt, n, seed=0, distinct=None):
    """n keys of type kt: any bit pattern (floating point: NaNs, infinities and both zeros among them), or `distinct`
    different ones drawn at random, so that most neighbours in a sorted segment are ties."""
    rng = np.random.default_rng(2000 + seed)
    dt = np.dtype(KEY_NP[kt])
    bits = rng.integers(0, 256, (n if distinct is None else distinct) * dt.itemsize, dtype=np.uint8).view(dt)
    return bits if distinct is None else bits[rng.integers(0, distinct, n)]


def source(form, ct, counts, base=0):
    counts = np.asarray(counts, dtype=np.uint64)
    if form == "counts":
        return counts.astype(CDT[ct])
    return (np.concatenate((np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64))) + np.uint64(base)).astype(CDT[ct])


def run_sort(dev, form, ct, kt, mode, counts, n, what, num_in=None, base=0, offs=(0, 0, 0, 0, 0), obj=None, q=None, src=None, compare=True,
             seed=0, keys=None, distinct=None):
    """One call on views at byte offsets offs = (counts_or_offsets, keys_in, values_in, keys_out, values_out) with n rows;
    checks everything and returns (total, keys_out bytes, values_out bytes) as read back. src: the input as it is (broken
    preconditions); compare False: the rows' contents are not compared."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = source(form, ct, counts, base)
    m_h = src.size - (1 if form == "offsets" else 0)
    if keys is None:
        keys = keys_for(kt, n, seed, distinct)
    vs = VS[mode]
    vdt = np.uint64 if vs == 8 else np.uint32
    vals = np.random.default_rng(3000 + seed).integers(0, np.iinfo(vdt).max, n, dtype=vdt) if mode in ("v4", "v8") else None
    p, total = segsort(form, src, keys, num_in) if compare else (None, None)
    what = "%s %s %s %s n %d, %s" % (form, ct, kt, mode, n, what)
    ks = keys.dtype.itemsize
    ss = obj or clo.SegSort(form, ctx, kt, vs, ct)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0)
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    k_r = Region(rdev, n * ks, offs[1], keys, 1) if n else None
    v_r = Region(rdev, n * vs, offs[2], vals, 2) if vals is not None else None   # (n 0: still present, 8-byte values have no arg form)
    ko_r = Region(rdev, n * ks, offs[3], None, 2) if mode != "arg without keys_out" else None
    vo_r = Region(rdev, n * vs, offs[4], None, 0) if vs else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert ss.with_device_data(q, s_r.view, view(n_r), view(k_r), view(v_r), view(ko_r), view(vo_r), num_r.view, m_h, n), what
        q.finish()
        got = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        body = lambda r: r.base.read(q, np.uint8, r.host.size)[r.at:r.at + r.n].copy() if r is not None else None
        ko, vo = body(ko_r), body(vo_r)
        if compare:
            assert got == total, "%s: num_out = %d, the model's total is %d" % (what, got, total)
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            want_v = None if not vs else p if vals is None else vals[p]
            for r, now, want, name in ((ko_r, ko, keys[p], "keys_out"), (vo_r, vo, want_v, "values_out")):
                if r is None:
                    continue
                w = np.ascontiguousarray(want).view(np.uint8)
                rows = now[:w.size].reshape(p.size, -1) if p.size else now[:0].reshape(0, 1)
                bad = np.flatnonzero((rows != w.reshape(rows.shape)).any(axis=1))
                assert bad.size == 0, "%s: %d of %d rows of %s differ, first row %d" % (what, bad.size, p.size, name, bad[0] if bad.size else -1)
                r.check(want, what + ": " + name)                            # ... and nothing behind the rows written
        else:                                                                # in bounds: the guards
            for r, now in ((ko_r, ko), (vo_r, vo)):
                if r is not None:
                    r.check(now, what)
        s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if k_r:
            k_r.check(keys, what + ": keys_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return got, ko, vo
    finally:
        for r in (s_r, n_r, k_r, v_r, ko_r, vo_r, num_r):
            if r:
                r.close()
        if obj is None:
            ss.close()


def rotate(case):
    """A form, a count type, a key type and a mode for case number `case`."""
    kts = tuple(KEY_NP)
    return FORMS[case % 2], ("uint", "ulong")[case // 2 % 2], kts[case % len(kts)], MODES[case % len(MODES)]


def ones(k):
    return np.ones(int(k), np.int64)


def test_one_segment_of_n_rows(dev, T):
    """Tile counts 1, 2, 3, 6, 8 and 9: P = 0 .. 4 merge passes, both parities, tile counts that are no powers of two."""
    for case, n in enumerate((1, T - 1, T, T + 1, 2 * T, 2 * T + 1, 3 * T, 5 * T + 3, 8 * T, 8 * T + 1)):
        form, ct, kt, mode = rotate(case)
        got, _, _ = run_sort(dev, form, ct, kt, mode, [n], n, "one segment", base=case * 100, seed=case)
        assert got == n
        got, _, _ = run_sort(dev, "counts", "uint", "uint", "v4", [n], n, "one segment, few keys", seed=case, distinct=8)
        assert got == n


def big_sizes(T):
    """Single segments of 16, 17, 17, 34, 64 and (T = 2048) 513 tiles: P = 4, 5, 5, 6, 6 and 10 merge passes."""
    return (16 * T, 16 * T + 1, 17 * T - 1, 33 * T + 5, 64 * T, (1 << 20) + 3)


def geometric_fill(rng, rows, mean=16):
    """Counts of geometric length whose sum is exactly `rows`."""
    if rows <= 0:
        return np.zeros(0, np.int64)
    c = rng.geometric(1 / mean, rows // mean + 64)
    while int(c.sum()) < rows:
        c = np.concatenate((c, rng.geometric(1 / mean, 64)))
    c = c[:int(np.searchsorted(np.cumsum(c), rows, "left")) + 1].copy()
    c[-1] -= int(c.sum()) - rows
    return c


# long segments in HALF tiles and the move masks DESIGN.md section 22's rule gives them (tests/test_segsort_cpu.py
# restates the rule and asserts these): both parities, one to four resting passes between two moves, and one move at pass 6
# after six passes at rest
PINNED = ((5, 9), (13, 17), (25, 33), (61, 67), (127, 129))
PINNED_MASKS = (0b101, 0b1001, 0b10011, 0b100001, 0b1000000)
PINNED_TILES = 66
SINGLE_BIT = (8, 16, 32)                                                      # [(k - 1/2) T, (k + 1/2) T) in (k + 2) T rows: mask k


def pinned_counts(T, tiles, longs, seed=0):
    """`tiles` T rows: the long segments [a T / 2, b T / 2) of `longs`, segments of geometric length, mean 16, elsewhere."""
    rng = np.random.default_rng(4000 + seed)
    parts, at = [], 0
    for a, b in longs:
        s, e = a * T // 2, b * T // 2
        parts += [geometric_fill(rng, s - at), np.array([e - s])]
        at = e
    parts.append(geometric_fill(rng, tiles * T - at))
    return np.concatenate(parts).astype(np.int64)


END_TO_END_TILES, END_TO_END_SEED = 300, 3


def end_to_end_counts(T):
    """300 T rows cut into segments of T / 2 .. 40 T rows: every tile boundary but a few lies inside a long segment, and
    the tile where two of them meet holds the end of one and the start of the next."""
    rng = np.random.default_rng(END_TO_END_SEED)
    c = rng.integers(T // 2, 40 * T + 1, END_TO_END_TILES)
    c = c[:int(np.searchsorted(np.cumsum(c), END_TO_END_TILES * T, "left")) + 1].copy()
    c[-1] -= int(c.sum()) - END_TO_END_TILES * T
    return c


def test_one_segment_above_ten_tiles(dev, T):
    """P = 4, 5, 6 and (2^20 + 3 rows) the everyday pass count: merges whose parts are up to 2^19 rows long."""
    for case, n in enumerate(big_sizes(T)):
        for k in (case, case + 5):                                            # (case + 5: the 8-byte keys and the floats meet the large sizes too)
            form, ct, kt, mode = rotate(k)
            got, _, _ = run_sort(dev, form, ct, kt, mode, [n], n, "one segment", base=case * 100, seed=case)
            assert got == n
        got, _, _ = run_sort(dev, "counts", "uint", "uint", "v4", [n], n, "one segment, few keys", seed=case, distinct=8)
        assert got == n


def test_six_passes_of_nothing_but_ties(dev, T):
    """33 T + 5 rows of ONE key in the arg form: every comparison of every merge is a tie, and the row indices must come
    out as they went in."""
    n = 33 * T + 5
    for kt, form in (("uint", "offsets"), ("double", "counts"), ("uchar", "counts")):
        keys = np.full(n, 0x5A, np.uint8).repeat(np.dtype(KEY_NP[kt]).itemsize).view(KEY_NP[kt])
        got, _, vo = run_sort(dev, form, "uint", kt, "arg", [n], n, "one distinct key", keys=keys)
        assert got == n and np.array_equal(vo.view(np.uint32), np.arange(n, dtype=np.uint32))


@pytest.mark.parametrize("kt", ("uchar", "half", "int", "double"))
def test_pinned_move_masks_with_gaps(dev, T, kt):
    """The masks 0b101, 0b1001, 0b10011, 0b100001 and 0b1000000 in one array of 66 T rows: a segment rests in the
    workspace or in the outputs for one to six passes between its moves. Key sizes 1, 2, 4, 8 x four modes x random bits
    and 8 distinct keys."""
    counts = pinned_counts(T, PINNED_TILES, PINNED)
    n = PINNED_TILES * T
    for i, mode in enumerate(("keys", "v8", "arg", "arg without keys_out")):
        for distinct in (None, 8):
            run_sort(dev, FORMS[i % 2], ("uint", "ulong")[i // 2], kt, mode, counts, n, "pinned masks", base=i, seed=i, distinct=distinct)


def test_a_single_move_at_pass_3_4_and_5(dev, T):
    """[(k - 1/2) T, (k + 1/2) T) for k = 8, 16, 32: mask k, one move after log2(k) passes at rest in the workspace."""
    for i, k in enumerate(SINGLE_BIT):
        counts = pinned_counts(T, k + 2, ((2 * k - 1, 2 * k + 1),), seed=k)
        for j, mode in enumerate(("v4", "arg without keys_out")):
            form, ct, kt, _ = rotate(2 * i + j + 4)
            run_sort(dev, form, ct, kt, mode, counts, (k + 2) * T, "mask %d" % k, seed=i, distinct=(None, 8)[j])


def test_long_segments_end_to_end_in_300_tiles(dev, T):
    """Segments of T / 2 .. 40 T rows end to end: A and B of one tile move in opposite directions in one pass."""
    counts = end_to_end_counts(T)
    n = END_TO_END_TILES * T
    run_sort(dev, "counts", "uint", "uint", "v4", counts, n, "end to end")
    run_sort(dev, "offsets", "ulong", "double", "arg", counts, n, "end to end", base=77, seed=1)


def boundary_cases(T):
    h = T // 2
    return (
        ("a segment ending exactly at T", np.concatenate(([T], ones(9))), T + 9),
        ("a segment starting exactly at T", np.concatenate((ones(7), [T - 7, 2 * T], ones(3))), 3 * T + 3),
        ("the two rows [T - 1, T + 1)", np.concatenate(([T - 1, 2], ones(10))), T + 11),
        ("[3.5 T, 4.5 T) in 6 T: crosses a level-2 boundary only, merged at pass 2 alone", np.concatenate((ones(3 * T + h), [T], ones(T + h))), 6 * T),
        ("[1.5 T, 4.5 T): crosses lo, mid and hi of the pair [2 T, 4 T)", np.concatenate((ones(T + h), [3 * T], ones(T + h))), 6 * T),
        ("an end on every tile boundary: no merges", np.array([T, h, h, T, 3, T - 3, T]), 5 * T),
        ("two long segments in one tile", np.array([T + h, 2 * T, h]), 4 * T),
        ("long segments end to end", np.array([h, 3 * T, 2 * T + 1, 4 * T - 1, h]), 10 * T),
    )


def test_segments_on_and_across_tile_boundaries(dev, T):
    for case, (what, counts, n) in enumerate(boundary_cases(T)):
        assert int(counts.sum()) == n
        for k in range(2):
            form, ct, kt, mode = rotate(2 * case + k)
            run_sort(dev, form, ct, kt, mode, counts, n, what, base=17 * case, seed=case)
        run_sort(dev, "offsets", "uint", "uint", "arg", counts, n, what + ", few keys", seed=case, distinct=8)


def test_empty_segments(dev, T):
    z = lambda k: np.zeros(k, np.int64)
    run_sort(dev, "counts", "uint", "uint", "v4", np.concatenate(([T], z(3 * T), [T + 5])), 2 * T + 5, "3 T empty segments on a tile boundary")
    run_sort(dev, "offsets", "ulong", "int", "arg", np.concatenate((z(3 * T), [T + 5], z(T))), T + 5, "3 T empty segments at row 0", base=99)
    c = np.random.default_rng(5).geometric(1 / 40, 300)
    c[::2] = 0
    c[101] = 2 * T + 1
    run_sort(dev, "counts", "ulong", "float", "v8", c, int(c.sum()), "every other segment empty")
    for form in FORMS:
        got, ko, vo = run_sort(dev, form, "uint", "uint", "v4", z(50), 100, "all segments empty", base=5)
        assert got == 0                                                      # (run_sort checked that nothing was written)


def test_clipped_totals_and_num_in(dev, T):
    c = np.concatenate((ones(40), [T + 100, 7, 2 * T, 50, 50], ones(30)))
    total = int(c.sum())
    for case, n in enumerate((T + 143, 2 * T + 200, total - 85, 45, 25, 0)):    # the cut inside the 7, the 2 T, a 50, the T + 100, the ones
        form, ct, kt, mode = rotate(case)
        got, _, _ = run_sort(dev, form, ct, kt, mode, c, n, "total > n", base=3, seed=case)
        assert got == total > n
    for case, extra in enumerate((1, T // 2, 3 * T)):
        form, ct, kt, mode = rotate(case + 5)
        got, _, _ = run_sort(dev, form, ct, kt, mode, c, total + extra, "total < n", seed=case)
        assert got == total
    for case, num_in in enumerate((0, 1, 41, 43, c.size - 1, c.size, c.size + 1000)):
        form, ct, kt, mode = rotate(case + 1)
        got, _, _ = run_sort(dev, form, ct, kt, mode, c, total, "num_in %d of %d" % (num_in, c.size), num_in=num_in, seed=case)
        assert got == int(c[:num_in].sum())


def test_forms_and_count_types(dev, T):
    c = np.random.default_rng(6).geometric(1 / 300, 40)
    c[7] = 3 * T
    n = int(c.sum())
    for form, ct, base in (("offsets", "uint", 123456), ("offsets", "ulong", (1 << 40) + 5), ("counts", "ulong", 0), ("counts", "uint", 0)):
        run_sort(dev, form, ct, "uint", "v4", c, n, "base %d" % base, base=base)
    big = np.array([5, 2 * T + 1, (1 << 32) - 1, (1 << 32) - 1, 7], np.uint64)     # uint counts whose sum passes 2^32
    got, _, _ = run_sort(dev, "counts", "uint", "uint", "arg", big, 4 * T, "the sum passes 2^32")
    assert got == int(big.sum()) > 1 << 33


@pytest.mark.parametrize("kt", tuple(KEY_NP))
def test_key_and_value_matrix(dev, T, kt):
    c = np.concatenate((ones(20), [T + 3, 0, 0, 300, T, 5], np.full(10, (T - 348) // 10), ones(25 + (T - 348) % 10)))
    n = 3 * T + 5
    assert int(c.sum()) == n
    for i, mode in enumerate(MODES):
        run_sort(dev, FORMS[i % 2], ("uint", "ulong")[i // 2 % 2], kt, mode, c, n, "matrix", base=i, seed=i)
        run_sort(dev, FORMS[(i + 1) % 2], "uint", kt, mode, c, n, "matrix, few keys", seed=i, distinct=5)


@pytest.mark.parametrize("kt", ("half", "float", "double"))
def test_float_zeros_and_nans_keep_their_bits(dev, T, kt):
    dt = np.dtype(KEY_NP[kt])
    ut = np.dtype("u%d" % dt.itemsize)
    nan = np.array([np.nan], dt).view(ut)[0]
    sign = ut.type(1 << (8 * dt.itemsize - 1))
    special = np.array([0, sign, nan, nan | ut.type(1), nan | sign, (nan | sign) | ut.type(2)], ut).view(dt)
    pool = np.concatenate((special, np.array([1.0, -1.0, np.inf, -np.inf, 0.5], dt)))
    n = 2 * T + 9
    keys = pool[np.random.default_rng(8).integers(0, pool.size, n)]
    c = np.array([50, T, 3, T - 44, n - 2 * T - 9])
    for mode in ("keys", "arg"):
        _, ko, _ = run_sort(dev, "counts", "uint", kt, mode, c, n, "zeros and NaNs", keys=keys)
        out = ko.view(ut)
        assert all(np.array_equal(np.sort(out[a:b]), np.sort(keys.view(ut)[a:b])) for a, b in ((0, 50), (50, 50 + T)))   # the same bit patterns


def test_stability_with_8_distinct_keys(dev, T):
    c = np.concatenate(([3 * T + 1], np.full(20, 37), [T], ones(11), [2 * T - 5]))
    n = int(c.sum())
    for kt in ("uchar", "int", "double"):
        _, _, vo = run_sort(dev, "counts", "uint", kt, "arg", c, n, "8 distinct keys", distinct=8, seed=3)
        idx = vo.view(np.uint32)
        keys = keys_for(kt, n, 3, 8)
        ends = np.cumsum(c)
        for a, b in zip(np.concatenate(([0], ends[:-1])), ends):              # inside a segment, equal keys ascend by row
            seg = idx[a:b].astype(np.int64)
            same = keys.view("u%d" % keys.dtype.itemsize)[seg][1:] == keys.view("u%d" % keys.dtype.itemsize)[seg][:-1]
            assert (np.diff(seg)[same] > 0).all()


def test_broken_preconditions_stay_in_bounds(dev, T):
    """Offsets that descend or are unordered, counts whose sums wrap 2^64, a num_in above numel_seg: the call completes,
    the canaries and the inputs are intact. Contents are not compared: DESIGN.md section 22 gives the argument that this
    holds by construction, and this run shows it once."""
    rng = np.random.default_rng(90)
    m_h, n = 3 * T + 700, 5 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 4).astype(np.uint32)
    unordered = rng.integers(0, 2 * n, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for i, (form, ct, src) in enumerate((("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping))):
        for mode in ("v4", "arg without keys_out", "v8"):
            run_sort(dev, form, ct, "uint", mode, None, n, "broken preconditions", num_in=m_h + 1000, src=src, compare=False, seed=i)


def test_two_runs_are_identical_and_the_object_moves_to_a_second_queue(dev, T):
    clo, ctx, q = dev
    q2 = clo.Queue(ctx)
    obj = clo.SegSort("counts", ctx, "uint", 4, "uint")
    try:
        c = np.random.default_rng(12).geometric(1 / 700, 30)
        c[3], c[20] = 4 * T + 1, 0
        n = int(c.sum())
        first = run_sort(dev, "counts", "uint", "uint", "v4", c, n, "first run", obj=obj, distinct=8)
        again = run_sort(dev, "counts", "uint", "uint", "v4", c, n, "second run", obj=obj, distinct=8)
        assert first[0] == again[0] and np.array_equal(first[1], again[1]) and np.array_equal(first[2], again[2])
        for j, qq in enumerate((q2, q, q2)):
            total = (9, 2, 6)[j] * T + j                                      # large, small, large: the workspace follows the queue
            cj = np.array([total // 3, 0, total - total // 3])
            run_sort((clo, ctx, qq), "counts", "uint", "uint", "v4", cj, total, "moved, call %d" % j, obj=obj, q=qq, seed=j)
    finally:
        obj.close()
        q2.close()


def test_element_aligned_views(dev, T):
    """Every array one (or three) elements past a 16-byte boundary: nothing may assume more than the element's
    alignment."""
    c = np.random.default_rng(13).geometric(1 / 16, 90)
    c[5:9] = 0
    c[40] = 2 * T + 37
    n = int(c.sum())
    cases = (("counts", "uint", "uint", "v4", (4, 4, 4, 12, 4)), ("offsets", "uint", "ushort", "arg", (12, 2, 0, 6, 12)),
             ("counts", "ulong", "double", "v8", (8, 8, 8, 8, 8)), ("offsets", "ulong", "uchar", "keys", (8, 1, 0, 3, 0)),
             ("counts", "uint", "float", "arg without keys_out", (12, 12, 0, 0, 4)), ("offsets", "uint", "long", "v4", (4, 8, 12, 8, 4)))
    for i, (form, ct, kt, mode, offs) in enumerate(cases):
        run_sort(dev, form, ct, kt, mode, c, n, "views at %s" % (offs,), offs=offs, base=9, seed=i)


def test_host_data_form(dev, T):
    clo, ctx, q = dev
    c = np.random.default_rng(14).geometric(1 / 60, 50)
    c[::5] = 0
    c[11] = T + 77
    total = int(c.sum())
    for form in FORMS:
        for kt, vs, ct in (("int", 0, "uint"), ("float", 4, "ulong"), ("ulong", 8, "uint")):
            src = source(form, ct, c, 4321)
            ss = clo.SegSort(form, ctx, kt, vs, ct)
            for n in (0, total - 5, total, total + 7):
                keys = keys_for(kt, n, n)
                vals = np.arange(n, dtype=np.uint64 if vs == 8 else np.uint32) * 3 if vs else None
                for num_in, qe in ((None, q), (c.size // 2, None), (c.size + 9, q)):
                    p, t = segsort(form, src, keys, num_in)
                    ko, vo, got = ss.with_host_data(src, keys, vals, num_in=num_in, q_exec=qe)
                    assert got == t and ko.size == p.size and np.array_equal(ko.view(np.uint8), keys[p].view(np.uint8)), (form, kt, n, num_in)
                    assert vo is None if not vs else np.array_equal(vo, vals[p]), (form, kt, n, num_in)
            if vs == 4:                                                       # the arg form, with and without keys_out
                keys = keys_for(kt, total, 1)
                p, t = segsort(form, src, keys)
                for with_keys in (True, False):
                    ko, vo, got = ss.with_host_data(src, keys, None, keys_out=with_keys)
                    assert got == t and np.array_equal(vo, p) and (ko is None) != with_keys
            ss.close()


class ThinABI:
    """The argument tuples of clo_hip_segsort that must be refused, in the order the function makes its checks and with
    one bad argument at a time, and those that must work. They are given as keyword sets over addresses the caller
    supplies, so that the device code (test_thin_abi_status_codes here) and the host stub of tests/hoststub/
    (tests/test_segsort_cpu.py) answer the same table and the two copies of the rules cannot drift."""
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    ORDER = ("form", "c", "cs", "n_in", "ki", "vi", "ko", "vo", "num", "m", "n", "kt", "vs", "w", "wb")

    def __init__(self, T, types, workspace_bytes):
        self.types, self.m_h, self.n = types, 1000, 3 * T
        self.need = workspace_bytes(self.m_h, self.n, 4, 4)
        self.big = max(workspace_bytes(self.m_h + 1, self.n + 1, 8, vs) for vs in (0, 4, 8))   # enough for every accepted and refused shape
        assert 0 < self.need <= self.big and self.need % 256 == 0
        rng = np.random.default_rng(5)
        self.counts = rng.integers(0, 9, 2 * self.m_h + 4, dtype=np.uint32)
        self.counts[5] = T + 7                                                # one segment for the merge passes
        self.keys = rng.integers(0, 1 << 32, 2 * self.n + 4, dtype=np.uint32) & np.uint32(0x8000001f)   # ties; both signs as int
        self.vals = rng.integers(0, 1 << 32, 2 * self.n + 4, dtype=np.uint32)
        self.num_in = np.array([self.m_h // 2, 0], np.uint64)
        self.out_bytes = 8 * self.n + 16

    def defaults(self, P):
        return dict(form=0, c=P["cn"], cs=4, n_in=None, ki=P["ki"], vi=P["vi"], ko=P["ko"], vo=P["vo"], num=P["num"], m=self.m_h, n=self.n,
                    kt=self.types["uint"], vs=4, w=P["ws"], wb=self.big)

    def refusals(self, P):
        """[(what, keywords, status, the host stub can check it)]"""
        A, U, W = self.EARGS, self.EUNSUPPORTED, self.EWORKSPACE
        LONG = self.types["long"]
        out = []
        add = lambda what, status, stub=True, **kw: out.append((what, dict(self.defaults(P), **kw), status, stub))
        for form in (-1, 2, 100):
            add("form %d" % form, A, form=form)
        for cs in (0, 1, 2, 3, 16):
            add("count size %d" % cs, U, cs=cs)
        for kt in (-1, 11, 100):
            add("key type %d" % kt, U, kt=kt)
        for vs in (1, 2, 3, 16, -1):
            add("value size %d" % vs, U, vs=vs)
        add("numel_seg 2^32", A, m=1 << 32)
        add("numel 2^32", A, n=1 << 32)
        add("no counts", A, c=None)
        add("no offsets, numel_seg 0", A, c=None, form=1, m=0, n=0)
        add("no keys_in", A, ki=None)
        add("values_in with value_size 0", A, vs=0, vo=None)
        add("values_out with value_size 0", A, vs=0, vi=None)
        add("no values_out", A, vo=None)
        add("no values_out in the arg form", A, vi=None, vo=None)
        add("8-byte values without values_in", A, vs=8, vi=None)
        add("no keys_out with values", A, ko=None)
        add("no keys_out, keys only", A, vs=0, vi=None, vo=None, ko=None)
        add("no keys_out with 8-byte values", A, vs=8, ko=None)
        add("no num_out", A, num=None)
        add("num_out at 4 mod 8", A, num=P["num"] + 4)
        add("num_in at 4 mod 8", A, n_in=P["ni"] + 4)
        for name, key in (("counts_or_offsets", "c"), ("keys_in", "ki"), ("keys_out", "ko"), ("values_in", "vi"), ("values_out", "vo")):
            add(name + " off by 2", A, **{key: P[{"c": "cn"}.get(key, key)] + 2})
        add("ulong counts at 4 mod 8", A, c=P["cn"] + 4, cs=8)
        add("long keys_in at 4 mod 8", A, ki=P["ki"] + 4, kt=LONG)
        add("long keys_out at 4 mod 8", A, ko=P["ko"] + 4, kt=LONG)
        add("8-byte values_in at 4 mod 8", A, vi=P["vi"] + 4, vs=8)
        add("8-byte values_out at 4 mod 8", A, vo=P["vo"] + 4, vs=8)
        add("no workspace", A, w=None)
        add("the workspace off by 64", A, stub=False, w=P["ws"] + 64)       # (the stub's workspaces come from malloc: it has no such rule)
        add("the workspace one byte short", W, wb=self.need - 1)
        add("a workspace of 0 bytes", W, wb=0)
        return out

    def accepted(self, P):
        """[(what, keywords, (shift in elements, key type, mode, num_in, segments, rows))]"""
        INT = self.types["int"]
        d = lambda **kw: dict(self.defaults(P), **kw)
        m, n = self.m_h, self.n
        return [
            ("a workspace of exactly the bytes asked for", d(wb=self.need), (0, "uint", "v4", None, m, n)),
            ("num_in", d(n_in=P["ni"]), (0, "uint", "v4", self.m_h // 2, m, n)),
            ("every view one element past a 16-byte boundary", d(c=P["cn"] + 4, ki=P["ki"] + 4, vi=P["vi"] + 4, ko=P["ko"] + 4, vo=P["vo"] + 4, kt=INT),
             (1, "int", "v4", None, m, n)),
            ("the arg form without keys_out", d(vi=None, ko=None), (0, "uint", "arg without keys_out", None, m, n)),
            ("numel_seg 0: no workspace, no inputs", d(c=None, ki=None, vi=None, vo=None, vs=0, m=0, n=0, w=None, wb=0), (0, "uint", "keys", None, 0, 0)),
        ]

    def want(self, spec, form):
        """(keys_out rows, values_out rows, total) of the model for an accepted call."""
        shift, kt, mode, num_in, m, n = spec
        c = self.counts[shift:shift + m]
        keys = self.keys[shift:shift + n].view(KEY_NP[kt])
        p, total = segsort(FORMS[form], c, keys, num_in)
        return keys[p], p if mode.startswith("arg") else self.vals[shift:shift + n][p], total


def test_thin_abi_status_codes(dev, T):
    """Every refusal of clo_hip_segsort itself, one bad argument at a time, leaves the outputs and num_out alone; then
    the calls that must work, each against the model (the table of ThinABI, which the host stub answers too)."""
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    abi = ThinABI(T, clo.CLO_TYPES, lib.clo_hip_segsort_workspace_bytes)
    cn, ki, vi = Region(dev, abi.counts.nbytes, 0, abi.counts, 0), Region(dev, abi.keys.nbytes, 0, abi.keys, 1), Region(dev, abi.vals.nbytes, 0, abi.vals, 2)
    ni = Region(dev, 16, 0, abi.num_in, 2)
    ko, vo, num = Region(dev, abi.out_bytes, 0, None, 0), Region(dev, abi.out_bytes, 0, None, 1), Region(dev, 16, 0, None, 2)
    ws = clo.Buffer(ctx, abi.big + 256)
    P = dict(cn=cn.ptr, ki=ki.ptr, vi=vi.ptr, ni=ni.ptr, ko=ko.ptr, vo=vo.ptr, num=num.ptr, ws=ws.ptr)
    call = lambda kw: lib.clo_hip_segsort(*[kw[k] for k in ThinABI.ORDER], q.stream)
    try:
        for what, kw, status, _ in abi.refusals(P):
            assert call(kw) == status, what
        q.finish()
        for r in (ko, vo, num):
            r.check(None, "a refused thin call wrote")
        for what, kw, spec in abi.accepted(P):
            assert call(kw) == 0, what
            q.finish()
            want_k, want_v, total = abi.want(spec, kw["form"]) if spec[4] else (None, None, 0)
            assert int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0]) == total, what
            for r, ptr, want in ((ko, kw["ko"], want_k), (vo, kw["vo"], want_v)):
                if ptr is not None and want is not None:
                    at = r.at + 4 * spec[0]
                    got = r.base.read(q, np.uint8, r.host.size)[at:at + want.nbytes]
                    assert np.array_equal(got, want.view(np.uint8)), what
        for r in (cn, ki, vi, ni):
            r.check(r.contents(np.uint8), "an input changed")
    finally:
        ws.close()
        for r in (cn, ki, vi, ni, ko, vo, num):
            r.close()


def test_two_objects_on_two_queues(dev, T):
    """Two sorters, each with its own workspace, enqueued on two queues without a wait in between, three rounds of
    about 40 T rows with one long segment each."""
    clo, ctx, _ = dev
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("counts", "uint", "uint", 4), ("offsets", "ulong", "double", 0))
    objs = [clo.SegSort(form, ctx, kt, vs, ct) for form, ct, kt, vs in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (form, ct, kt, vs) in enumerate(specs):
                rng = np.random.default_rng(50 + 10 * rnd + i)
                n = 40 * T + 9 + rnd
                counts = np.concatenate((geometric_fill(rng, 7 * T + 100 * i), [(5 + 8 * i + rnd) * T + 3], geometric_fill(rng, n, 300)))
                counts[::9] = 0
                src, keys = source(form, ct, counts, 7), keys_for(kt, n, rnd, (None, 8)[rnd % 2])
                vals = rng.integers(0, 1 << 32, n, dtype=np.uint32) if vs else None
                rdev = (clo, ctx, qs[i])
                ks = keys.dtype.itemsize
                regs = [Region(rdev, src.nbytes, 0, src, 0), Region(rdev, keys.nbytes, 0, keys, 1), Region(rdev, 4 * n, 0, vals, 2) if vs else None,
                        Region(rdev, ks * n, 0, None, 2), Region(rdev, 4 * n, 0, None, 0) if vs else None, Region(rdev, 8, 0, None, 1)]
                sent.append((src, keys, vals, src.size - (form == "offsets"), n, regs))
            for i in range(2):
                qs[i].finish()                                                # the uploads; from here on nothing waits
            for i, (src, keys, vals, m_h, n, regs) in enumerate(sent):
                view = lambda r: r.view if r is not None else None
                assert objs[i].with_device_data(qs[i], regs[0].view, None, regs[1].view, view(regs[2]), regs[3].view, view(regs[4]), regs[5].view, m_h, n)
            for i in range(2):
                qs[i].finish()
            for i, (src, keys, vals, m_h, n, regs) in enumerate(sent):
                p, t = segsort(specs[i][0], src, keys)
                what = "round %d, %s" % (rnd, specs[i][0])
                assert t > n > 0 or p.size == min(t, n)
                regs[5].check(np.array([t], np.uint64), what + ": num_out")
                regs[3].check(keys[p], what + ": keys_out")
                if vals is not None:
                    regs[4].check(vals[p], what + ": values_out")
                for r in regs:
                    if r:
                        r.close()
    finally:
        for x in objs + qs:
            x.close()


def test_chain_expand_sort_reduce_without_a_host_wait(dev, T):
    """CloExpand's seg_out, the segmented sort of int keys and the segmented min and max of keys_out over the same
    counts, on one queue without a wait: the minima are the first and the maxima the last row of every non-empty sorted
    segment, empty segments receive the identities, and the sort of the composites seg_out << 32 | order key gives the same
    rows."""
    clo, ctx, q = dev
    rng = np.random.default_rng(60)
    counts = np.concatenate((geometric_fill(rng, 2 * T + 50), [3 * T + 1], geometric_fill(rng, 3 * T, 200)))
    counts[::4] = 0
    m, n = counts.size, int(counts.sum())
    keys = rng.integers(-1 << 31, 1 << 31, n).astype(np.int32)
    keys[rng.random(n) < 0.3] = 7                                            # ties
    c_r, k_r = Region(dev, 4 * m, 0, counts.astype(np.uint32), 0), Region(dev, 4 * n, 0, keys, 1)
    seg_r, ko_r = Region(dev, 4 * n, 0, None, 2), Region(dev, 4 * n, 0, None, 0)
    mn_r, mx_r, sk_r, sv_r = Region(dev, 4 * m, 0, None, 0), Region(dev, 4 * m, 0, None, 1), None, None
    nums = [Region(dev, 8, 0, None, i % 3) for i in range(4)]
    ex, ss = clo.Expand("counts", ctx, None, "uint"), clo.SegSort("counts", ctx, "int", 0, "uint")
    lo, hi = clo.SegReduce("min", "counts", ctx, "int", "int", "uint"), clo.SegReduce("max", "counts", ctx, "int", "int", "uint")
    kv = clo.Sorter("satradix", ctx, "ulong")
    try:
        assert ex.with_device_data(q, c_r.view, None, None, None, seg_r.view, None, nums[0].view, m, n)
        assert ss.with_device_data(q, c_r.view, None, k_r.view, None, ko_r.view, None, nums[1].view, m, n)
        assert lo.with_device_data(q, c_r.view, None, ko_r.view, mn_r.view, nums[2].view, m, n)
        assert hi.with_device_data(q, c_r.view, None, ko_r.view, mx_r.view, nums[3].view, m, n)
        q.finish()
        p, total = segsort("counts", counts.astype(np.uint32), keys)
        assert total == n
        for r in nums:
            r.check(np.array([n], np.uint64), "num_out")
        ko_r.check(keys[p], "keys_out")
        ends = np.cumsum(counts)
        starts = ends - counts
        full = counts > 0
        want_min = np.where(full, keys[p][np.minimum(starts, n - 1)], np.iinfo(np.int32).max).astype(np.int32)
        want_max = np.where(full, keys[p][np.maximum(ends, 1) - 1], np.iinfo(np.int32).min).astype(np.int32)
        mn_r.check(want_min, "the minimum is the first row of every sorted segment")
        mx_r.check(want_max, "the maximum is the last row")
        seg = np.repeat(np.arange(m, dtype=np.uint32), counts)
        seg_r.check(seg, "seg_out")
        composite = (seg.astype(np.uint64) << np.uint64(32)) | (keys.view(np.uint32) ^ np.uint32(1 << 31)).astype(np.uint64)
        sk_r, sv_r = Region(dev, 8 * n, 0, composite, 0), Region(dev, 8 * n, 0, None, 1)
        kv.with_device_data(q, sk_r.view, sv_r.view, n)                       # (sorting by key takes no 8-byte keys: the whole element)
        q.finish()
        sv_r.check((composite[p]), "the sort of the composite (segment, key) gives other rows")
    finally:
        for x in [c_r, k_r, seg_r, ko_r, mn_r, mx_r, sk_r, sv_r] + nums + [ex, ss, lo, hi, kv]:
            if x is not None:
                x.close()


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, T, form):
    """clo_hip_segsort captured from one client stream (a linear graph) after one eager warm-up and replayed three
    times, the counts, num_in, the keys and the values rewritten and the outputs refilled with a canary before each replay
    (the protocol of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the rows."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, n = 60, 4 * T + 3
    need = lib.clo_hip_segsort_workspace_bytes(m_h, n, 4, 4)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, 4 * n, 4 * n, 4 * n, 4 * n, 8, need)]
    src_m, nin_m, ki, vi, ko, vo, num, ws = made
    means = [140, 30, 300, 90, 140]                                          # 60 segments of mean 300: above the rows
    totals = set()
    INT = clo.CLO_TYPES["int"]

    def load(r):
        counts = np.random.default_rng(300 + r).geometric(1 / means[r], m_h) * (np.arange(m_h) % 4 != r % 4)
        counts[(7 * r) % m_h] += 2 * T
        src, num_in = source(form, "uint", counts, 50 * r), m_h - 10 * (r % 3)
        keys = keys_for("int", n, r, 50)
        vals = np.random.default_rng(r).integers(0, 1 << 32, n, dtype=np.uint32)
        for m in (ko, vo, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (ki, keys), (vi, vals)):
            mem_.put(arr)
        want = segsort(form, src, keys, num_in)
        totals.add(want[1])
        return want, keys, vals

    def enqueue():
        return lib.clo_hip_segsort(FORMS.index(form), src_m.ptr, 4, nin_m.ptr, ki.ptr, vi.ptr, ko.ptr, vo.ptr, num.ptr, m_h, n, INT, 4,
                                   ws.ptr, need, q.stream)

    def verify(r, want):
        (p, total), keys, vals = want
        tag = "%s round %d" % (form, r)
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        GC.same(ko.get(np.int32, n), np.concatenate((keys[p], GC.canary(np.int32, n - p.size))), tag + ": keys_out")
        GC.same(vo.get(np.uint32, n), np.concatenate((vals[p], GC.canary(np.uint32, n - p.size))), tag + ": values_out")
        GC.same(ki.get(np.int32, n), keys, "keys_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(totals) >= 4 and max(totals) > n > min(totals), totals
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def fuzz_counts(rng, kind, T):
    n = int(rng.integers(1, 9 * T + 1))
    if kind == "single":
        return np.array([n])
    mean = {"1": 1, "16": 16, "T/2": T // 2, "3T": 3 * T, "half empty": 24}[kind]
    c = rng.geometric(1 / mean, n // mean + 2) if mean > 1 else np.ones(n + 2, np.int64)
    if kind == "half empty":
        c[rng.random(c.size) < 0.5] = 0
    return c[:max(int(np.searchsorted(np.cumsum(c), n)), 1)]


def test_fuzz(dev, T):
    """240 seeded cases with n <= 9 T over the length distributions mean 1, 16, T / 2 and 3 T, a single segment and half
    of the segments empty; the form, count type, key type and mode rotate, the row count is at, below or above the
    total, a third of the cases have few distinct keys. One object per configuration, so that workspaces are reused
    between shapes."""
    clo, ctx, q = dev
    rng = np.random.default_rng(2026)
    kinds = ("1", "16", "T/2", "3T", "single", "half empty")
    objs = {}
    try:
        for case in range(240):
            form, ct, kt, mode = rotate(case)
            c = fuzz_counts(rng, kinds[case % len(kinds)], T)
            total = int(c.sum())
            n = (total, max(total - int(rng.integers(1, T)), 0), total + int(rng.integers(1, T)))[case // 6 % 3]
            key = (form, ct, kt, VS[mode])
            if key not in objs:
                objs[key] = clo.SegSort(form, ctx, kt, VS[mode], ct)
            num_in = None if case % 7 else int(rng.integers(0, c.size + 3))
            run_sort(dev, form, ct, kt, mode, c, n, "fuzz case %d (%s)" % (case, kinds[case % len(kinds)]), num_in=num_in, base=case, obj=objs[key],
                     seed=case, distinct=7 if case % 3 == 0 else None)
    finally:
        for o in objs.values():
            o.close()


def test_rows_above_2p31(dev, T):
    """n = 2^31 + 2^20 + 5 uchar keys in the arg form with keys_out: segments of 5 rows and one of 3 T + 1 rows laid
    across row 2^31 (the run structure of test_gpu_above_2p31.py), so that the 32-bit row indices written need bit 31.
    Counts and keys are made on the device, key i being a hash of i with 64 values (frequent ties, not sorted), and the
    result is checked there in chunks without a host model: keys_out[j] == keys_in[values_out[j]], values_out[j] lies
    inside the segment of row j, and within a segment (key, index) ascends strictly from row to row. Together: a stable
    sort of exactly the segment's rows."""
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
    key_of = lambda i: (((i * 2654435761) >> 13) & 0x3f).to(torch.uint8)
    keys = torch.empty(N, dtype=torch.uint8, device="cuda")
    for lo, hi in chunks(N):
        keys[lo:hi] = key_of(torch.arange(lo, hi, dtype=torch.int64, device="cuda"))
    ko = torch.full((N + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    vo = torch.full((N + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")                           # bytes A5 A5 A5 A5
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (counts, keys, ko, vo, cnt)]
    ss = clo.SegSort("counts", ctx, "uchar", 4, "uint")
    try:
        assert ss.with_device_data(q, bufs[0], None, bufs[1], None, bufs[2], bufs[3], bufs[4], m, N)
        q.finish()
        assert int(cnt[0]) == N
        step = 1 << 27
        for lo, hi in chunks(N, step):
            top = min(hi + 1, N)                                                                        # one row of the next chunk: the pair across the cut
            i, _, b = runs.run_and_start(torch, lo, top)
            e = torch.where(i < runs.s0, b + 5, torch.where(i < runs.after, torch.full_like(b, runs.after), torch.clamp(b + 5, max=N)))
            v = vo[lo:top].to(torch.int64) & 0xffffffff
            assert bool(((v >= b) & (v < e)).all()), "values_out leaves the segment in rows [%d, %d)" % (lo, top)
            k = ko[lo:top]
            assert bool((k == keys[v]).all()), "keys_out[j] != keys_in[values_out[j]] in rows [%d, %d)" % (lo, top)
            comp = (k.to(torch.int64) << 32) | v
            same = b[1:] == b[:-1]
            assert bool((comp[1:] > comp[:-1])[same].all()), "(key, index) does not ascend strictly inside a segment in rows [%d, %d)" % (lo, top)
            del i, b, e, v, k, comp, same
        assert bool((ko[N:] == 0xA5).all()) and bool((vo[N:] == -0x5A5A5A5B).all()), "rows >= n were written"
        for lo, hi in chunks(N):
            assert bool((keys[lo:hi] == key_of(torch.arange(lo, hi, dtype=torch.int64, device="cuda"))).all()), "keys_in changed"
    finally:
        for x in bufs + [ss]:
            x.close()
        del counts, keys, ko, vo
        torch.cuda.empty_cache()
