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
host form and a seeded fuzz."""
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
