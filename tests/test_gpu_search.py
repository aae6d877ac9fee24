"""CloSearch (include/clo_search.h) on the GPU against the numpy model of tests/search_model.py, bit for bit. Every array
is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); pos_out is pre-filled with the pattern, and after every call it equals the model while the
guards and both inputs are unchanged. With T = search_tile, L = search_lds_keys, P = search_pivots: sizes around every
edge at which a kernel changes form, on both sides and both paths, the grid-stride loop walked with 1, 2 and 3
work-groups; where the answer lies (below, above, on every key, between neighbours, ties around pivot positions and
around the LDS-range edge, long and empty ranges of a sorted tile); every key type with its special values; the
library's own sort, argmerge and histogram as second oracles; element-aligned views; more tiles than the chip holds
at once; one object used large -> small -> large; the host-data form; the thin ABI's status codes; clo_hip_search
captured into a graph and replayed; and inputs that break a precondition (the bounds contract only)."""
import numpy as np
import pytest

from search_model import search, sort_keys
from test_gpu_histogram import Region
from test_gpu_merge import keys_of_type

pytestmark = pytest.mark.gpu

_NP = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
       "long": np.int64, "ulong": np.uint64, "half": np.float16, "float": np.float32, "double": np.float64}
KEY_TYPES = list(_NP)
_KIND = {"i": 1, "u": 0, "f": 2}
UPPER, SORTED = 1, 2
BOTH_SIDES = ((False, False), (True, False))          # (upper, sorted flag): the general path
BOTH_SIDES_SORTED = ((False, True), (True, True))     # the sorted-needles path


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def sizes_of(dev, kt="uint"):
    ks = np.dtype(_NP[kt]).itemsize
    T, L, P = dev[0].search_tile(ks), dev[0].search_lds_keys(ks), dev[0].search_pivots(ks)
    assert T > 0 and T % 64 == 0 and 2 <= P <= L
    return T, L, P


def run_search(dev, kt, hay, ndl, forms, what, offs=(0, 0, 0), obj=None, compare=True, max_groups=None):
    """One call per form = (upper, sorted flag) on the same views at byte offsets offs = (haystack, needles, pos_out);
    checks everything after each. max_groups given: through the thin ABI with that bound. compare False (a broken
    precondition): success, guards, inputs and every position <= numel_h only."""
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    dt = np.dtype(_NP[kt])
    hay, ndl = np.ascontiguousarray(hay, dtype=dt), np.ascontiguousarray(ndl, dtype=dt)
    nh, nn = hay.size, ndl.size
    s = obj or clo.Search(ctx, kt)
    h_r, n_r = Region(dev, hay.nbytes, offs[0], hay, 0), Region(dev, ndl.nbytes, offs[1], ndl, 1)
    p_r = Region(dev, 4 * nn, offs[2], None, 2)
    ws = None
    try:
        for i, (upper, flag) in enumerate(forms):
            tag = "%s: %s, %s" % (what, "upper" if upper else "lower", "sorted flag" if flag else "general")
            if i:
                p_r.base.write(q, p_r.host)     # the canary again
            if max_groups is None:
                assert s.with_device_data(q, h_r.view if nh else None, nh, n_r.view, nn, p_r.view, upper=upper, needles_sorted=flag), tag
            else:
                flags = (UPPER if upper else 0) | (SORTED if flag else 0)
                need = lib.clo_hip_search_workspace_bytes(nh, nn, flags)
                if need and ws is None:
                    ws = clo.Buffer(ctx, need)
                st = lib.clo_hip_search(h_r.ptr, nh, n_r.ptr, nn, p_r.ptr, dt.itemsize, _KIND[dt.kind], flags, max_groups,
                                        ws.ptr if need else None, need, q.stream)
                assert st == 0, (tag, st)
            q.finish()
            if compare:
                p_r.check(search(hay, ndl, upper), tag + ": pos_out")
            else:
                got = p_r.base.read(q, np.uint8, p_r.host.size)
                for lo, hi, where in ((0, p_r.at, "below"), (p_r.at + p_r.n, p_r.host.size, "above")):
                    assert np.array_equal(got[lo:hi], p_r.host[lo:hi]), "%s: the guard %s pos_out was written" % (tag, where)
                pos = got[p_r.at:p_r.at + 4 * nn].copy().view(np.uint32)
                assert (pos <= nh).all(), "%s: a position above numel_h" % tag
            h_r.check(hay, tag + ": haystack")
            n_r.check(ndl, tag + ": needles")
    finally:
        for r in (h_r, n_r, p_r):
            r.close()
        if ws is not None:
            ws.close()
        if obj is None:
            s.close()


def sorted_uint(n, seed, span):
    """n ascending uint keys from [1, span]: ties occur, 0 lies below and span + 1 above every key."""
    return np.sort(np.random.default_rng(seed).integers(1, span + 1, n, dtype=np.uint32))


def needles_uint(n, seed, span):
    """n needles from [0, span + 1], unsorted."""
    return np.random.default_rng(seed).integers(0, span + 2, n, dtype=np.uint32)


@pytest.mark.parametrize("path", ["general", "sorted"])
def test_size_sweep(dev, path):
    clo, ctx, q = dev
    T, L, P = sizes_of(dev)
    obj = clo.Search(ctx, "uint")
    for nh in (0, 1, 2, 63, 64, 65, P - 1, P, P + 1, 2 * P + 3, L - 1, L, L + 1, 2 * L + 5):
        span = max(4, nh // 3)
        hay = sorted_uint(nh, nh + 1, span)
        for nn in (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3):
            ndl = needles_uint(nn, 7 * nh + nn, span)
            what = "%d needles in %d keys" % (nn, nh)
            if path == "general":
                run_search(dev, "uint", hay, ndl, BOTH_SIDES, what, obj=obj)
            else:
                run_search(dev, "uint", hay, np.sort(ndl), BOTH_SIDES_SORTED, what, obj=obj)
    obj.close()


@pytest.mark.parametrize("max_groups", [0, 1, 2, 3])
def test_grid_stride_loop(dev, max_groups):
    T, L, P = sizes_of(dev)
    for nh in (L - 1, 2 * L + 5):                                       # the staged haystack, the pivots
        hay = sorted_uint(nh, 3, nh // 3)
        for nn in (1, T + 1, 7 * T + 3):
            ndl = needles_uint(nn, nn + max_groups, nh // 3)
            run_search(dev, "uint", hay, ndl, BOTH_SIDES, "max_groups %d, %d in %d" % (max_groups, nn, nh), max_groups=max_groups)
            run_search(dev, "uint", hay, np.sort(ndl), BOTH_SIDES_SORTED, "max_groups %d, %d in %d" % (max_groups, nn, nh), max_groups=max_groups)


ALL_FORMS = BOTH_SIDES + BOTH_SIDES_SORTED


def test_below_above_on_and_between(dev):
    T, L, P = sizes_of(dev)
    u = lambda x: np.asarray(x, dtype=np.uint32)
    for nh in (L - 3, 2 * L + 5):
        hay = u(np.arange(nh) * 2 + 10)                                 # distinct even keys
        run_search(dev, "uint", hay, u([0, 3, 9, 9, 9]), ALL_FORMS, "below every key, %d" % nh)
        run_search(dev, "uint", hay, u([2 * nh + 10, 2 * nh + 11, 0xFFFFFFFF]), ALL_FORMS, "above every key, %d" % nh)
        run_search(dev, "uint", hay, hay, ALL_FORMS, "each key in turn, %d" % nh)
        run_search(dev, "uint", hay, hay + np.uint32(1), ALL_FORMS, "between neighbours, %d" % nh)
        run_search(dev, "uint", hay, u(np.full(T + 5, hay[nh // 2])), ALL_FORMS, "all needles equal, %d" % nh)
        run_search(dev, "uint", hay, u(np.full(T + 5, hay[nh // 2] + 1)), ALL_FORMS, "all needles equal and absent, %d" % nh)


def test_ties(dev):
    clo, ctx, q = dev
    T, L, P = sizes_of(dev)
    u = lambda *parts: np.concatenate([np.full(c, k, np.uint32) for k, c in parts])
    probes = np.array([6, 7, 8], np.uint32)
    for nh in (1, L, L + 1, 3 * L + 1):
        hay = u((7, nh))                                                # all equal: lower 0, upper numel_h
        run_search(dev, "uint", hay, probes, ALL_FORMS, "haystack all equal, %d" % nh)
        s = clo.Search(ctx, "uint")
        assert s.with_host_data(hay, probes[1:2], q_exec=q).tolist() == [0] and s.with_host_data(hay, probes[1:2], upper=True, q_exec=q).tolist() == [nh]
        s.close()
    r = L + L // 2                                                      # eight distinct keys in runs of 1.5 L
    hay = u(*[(3 * k + 1, r) for k in range(8)])
    ndl = np.arange(0, 26, dtype=np.uint32)
    run_search(dev, "uint", hay, np.resize(ndl, T + 9), BOTH_SIDES, "eight keys")
    run_search(dev, "uint", hay, np.sort(np.resize(ndl, T + 9)), BOTH_SIDES_SORTED, "eight keys")
    run_search(dev, "uint", hay, ndl, BOTH_SIDES_SORTED, "eight keys, few needles over 12 L")


def test_tie_runs_around_pivots_and_the_lds_edge(dev):
    T, L, P = sizes_of(dev)
    nh = 3 * L
    assert nh % P == 0
    step = nh // P
    base = np.arange(nh, dtype=np.uint32) * np.uint32(2) + np.uint32(100)
    piv = (P // 2) * step                                               # a pivot position of the general path
    for start in (piv - 1, piv, piv + 1):
        for run in (2, step, 3 * step + 1):                             # inside one pivot interval, over one, over several
            hay = base.copy()
            hay[start:start + run] = hay[start]
            v = hay[start]
            ndl = np.array([v - 2, v - 1, v, v + 1, v + 2, hay[start + run] - 1, hay[start + run], hay[start - 1]], np.uint32)
            run_search(dev, "uint", hay, ndl, BOTH_SIDES, "a run of %d from %d (pivot at %d)" % (run, start, piv))
            run_search(dev, "uint", hay, np.sort(ndl), BOTH_SIDES_SORTED, "a run of %d from %d (pivot at %d)" % (run, start, piv))
    # sorted needles: one tile whose range of the haystack is L - 1, L, L + 1 keys, with a run of ties that starts one
    # before, on and one after the end of that range
    a = 77
    for length in (L - 1, L, L + 1):
        for start in (a + length - 2, a + length - 1, a + length):
            hay = base.copy()
            hay[start:start + 5] = hay[start]
            inner = np.sort(np.random.default_rng(start).integers(a, a + length, 200))
            ndl = np.sort(np.concatenate((hay[inner], hay[inner] + np.uint32(1), [hay[a], hay[a + length - 1]])).astype(np.uint32))
            ndl = ndl[ndl <= hay[a + length - 1]]
            run_search(dev, "uint", hay, ndl, BOTH_SIDES_SORTED + BOTH_SIDES, "a range of %d, ties from %d" % (length, start))


def test_long_and_empty_ranges_of_a_sorted_tile(dev):
    T, L, P = sizes_of(dev)
    u = lambda x: np.asarray(x, dtype=np.uint32)
    hay = u(np.arange(3 * L) * 4 + 8)
    run_search(dev, "uint", hay, u([8, 9, 4 * L, 4 * L + 1, 8 * L + 3, 12 * L + 4]), BOTH_SIDES_SORTED, "six needles over 3 L keys")
    run_search(dev, "uint", hay, u(np.sort(np.resize([hay[5], hay[3 * L - 2], hay[L]], 2 * T + 3))), BOTH_SIDES_SORTED, "tiles over 3 L keys")
    # every needle of a tile between two neighbouring keys, below the first key, above the last: the range is empty
    for v in (hay[L] + 1, 3, hay[-1] + 2):
        run_search(dev, "uint", hay, u(np.full(T + 3, v)), BOTH_SIDES_SORTED, "an empty range at %d" % v)
        run_search(dev, "uint", hay, u(np.arange(3) + v), BOTH_SIDES_SORTED, "an empty range at %d, three needles" % v)


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types(dev, kt):
    """The types' extremes, +-0, +-inf and four NaN payloads of each sign (keys_of_type of test_gpu_merge.py) in both
    arrays; a short haystack (staged whole) and a long one (pivots; sorted tiles with long ranges)."""
    T, L, P = sizes_of(dev, kt)
    rng = np.random.default_rng(2)
    for nh in (L - 1, 2 * L + 5):
        hay = keys_of_type(kt, nh, 5)
        ndl = keys_of_type(kt, T + 37, 6)
        run_search(dev, kt, hay, ndl[rng.permutation(ndl.size)], BOTH_SIDES, "%s, %d keys" % (kt, nh))
        run_search(dev, kt, hay, ndl, BOTH_SIDES_SORTED, "%s, %d keys" % (kt, nh))
    # distinct keys over the type's whole range, so that the order itself (not only the ties) is exercised
    dt = np.dtype(_NP[kt])
    raw = np.unique(rng.integers(0, 1 << (8 * dt.itemsize), 2 * L + 5, dtype=np.uint64).astype("u%d" % dt.itemsize)).view(dt)
    hay = sort_keys(raw)
    ndl = sort_keys(np.concatenate((raw[::7], keys_of_type(kt, 40, 7))))
    run_search(dev, kt, hay, ndl[rng.permutation(ndl.size)], BOTH_SIDES, "%s, distinct keys" % kt)
    run_search(dev, kt, hay, ndl, BOTH_SIDES_SORTED, "%s, distinct keys" % kt)


@pytest.mark.parametrize("kt", ["uint", "int", "float"])
def test_against_the_librarys_own_sort(dev, kt):
    """Sort the haystack and the needles with clo_sort_by_key_* (whose order is the search's for signed and floating
    keys too), search on the same queue with no host synchronisation in between, and compare with the model of what
    the sorts gave."""
    clo, ctx, q = dev
    T, L, P = sizes_of(dev, kt)
    nh, nn = 3 * L + 7, 2 * T + 5
    rng = np.random.default_rng(3)
    dt = np.dtype(_NP[kt])

    def keys(n):
        k = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        k[::3] &= np.uint32(0x80000003)                                 # ties, of both signs
        if kt == "float":
            k[::17] = np.resize(np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc00002], np.uint32), k[::17].shape)
        return k.view(dt)

    hay, ndl = keys(nh), keys(nn)
    B = lambda nbytes: clo.Buffer(ctx, nbytes)
    hin, nin, hs, ns, lo, up, lo2 = B(4 * nh), B(4 * nn), B(4 * nh), B(4 * nn), B(4 * nn), B(4 * nn), B(4 * nn)
    hv, nv = B(4 * nh), B(4 * nn)                                       # the argsorts, not looked at
    sorter, s = clo.Sorter("satradix", ctx, kt), clo.Search(ctx, kt)
    try:
        hin.write(q, hay)
        nin.write(q, ndl)
        sorter.by_key_with_device_data(q, hin, None, hs, hv, nh)
        sorter.by_key_with_device_data(q, nin, None, ns, nv, nn)
        s.with_device_data(q, hs, nh, ns, nn, lo, needles_sorted=True)
        s.with_device_data(q, hs, nh, ns, nn, up, upper=True, needles_sorted=True)
        s.with_device_data(q, hs, nh, nin, nn, lo2)                     # the unsorted needles, general path
        q.finish()
        sh, sn = sort_keys(hay), sort_keys(ndl)
        assert np.array_equal(hs.read(q, np.uint32, nh), sh.view(np.uint32)) and np.array_equal(ns.read(q, np.uint32, nn), sn.view(np.uint32))
        assert np.array_equal(lo.read(q, np.uint32, nn), search(sh, sn, False))
        assert np.array_equal(up.read(q, np.uint32, nn), search(sh, sn, True))
        assert np.array_equal(lo2.read(q, np.uint32, nn), search(sh, ndl, False))
    finally:
        for x in (hin, nin, hs, ns, lo, up, lo2, hv, nv, sorter, s):
            x.close()


def test_against_the_argmerge(dev):
    """Output j of the argmerge of (haystack, needles) that comes from needle i = p[j] - numel_h has all haystack keys
    <= it before it (ties go to A) and i needles: j - i == upper[i]."""
    clo, ctx, q = dev
    T, L, P = sizes_of(dev)
    nh, nn = 2 * L + 5, T + 9
    hay, ndl = sorted_uint(nh, 1, nh // 4), np.sort(needles_uint(nn, 2, nh // 4))
    B = lambda nbytes: clo.Buffer(ctx, nbytes)
    hb, nb, pb, ub = B(4 * nh), B(4 * nn), B(4 * (nh + nn)), B(4 * nn)
    m, s = clo.Merge(ctx, "uint", 4), clo.Search(ctx, "uint")
    try:
        hb.write(q, hay)
        nb.write(q, ndl)
        m.with_device_data(q, hb, None, nh, nb, None, nn, None, pb)
        s.with_device_data(q, hb, nh, nb, nn, ub, upper=True, needles_sorted=True)
        q.finish()
        p, upper = pb.read(q, np.uint32, nh + nn).astype(np.int64), ub.read(q, np.uint32, nn).astype(np.int64)
        j = np.flatnonzero(p >= nh)
        i = p[j] - nh
        assert j.size == nn and np.array_equal(j - i, upper[i])
        assert np.array_equal(upper, search(hay, ndl, True))
    finally:
        for x in (hb, nb, pb, ub, m, s):
            x.close()


def test_against_the_histogram(dev):
    """Edges lower + (b << shift) as needles into sorted keys: differences of lower bounds are CloHistogram's counts of
    the same keys."""
    clo, ctx, q = dev
    T, L, P = sizes_of(dev)
    n, lower, shift, bins = 5 * L + 3, 1000, 5, 300
    rng = np.random.default_rng(4)
    keys = np.sort(rng.integers(lower - 500, lower + (bins << shift) + 500, n).astype(np.uint32))   # some outside every bin
    edges = (lower + (np.arange(bins + 1, dtype=np.uint64) << np.uint64(shift))).astype(np.uint32)
    B = lambda nbytes: clo.Buffer(ctx, nbytes)
    kb, eb, pb, cb = B(4 * n), B(4 * (bins + 1)), B(4 * (bins + 1)), B(4 * bins)
    h, s = clo.Histogram(ctx, "uint"), clo.Search(ctx, "uint")
    try:
        kb.write(q, keys)
        eb.write(q, edges)
        h.with_device_data(q, kb, None, cb, n, lower=lower, shift=shift, num_bins=bins)
        s.with_device_data(q, kb, n, eb, bins + 1, pb, needles_sorted=True)
        q.finish()
        pos, counts = pb.read(q, np.uint32, bins + 1), cb.read(q, np.uint32, bins)
        assert np.array_equal(np.diff(pos.astype(np.int64)), counts.astype(np.int64))
        assert counts.sum() == np.count_nonzero((keys >= edges[0]) & (keys < edges[-1]))
    finally:
        for x in (kb, eb, pb, cb, h, s):
            x.close()


def test_element_aligned_views(dev):
    """Views at odd element offsets inside their allocations: nothing may assume 16-byte alignment."""
    rng = np.random.default_rng(8)
    for kt, offs in (("uchar", (1, 1, 4)), ("char", (3, 13, 0)), ("ushort", (2, 6, 12)), ("uint", (4, 4, 4)), ("float", (12, 8, 4)),
                     ("ulong", (8, 8, 4)), ("double", (8, 0, 12))):
        T, L, P = sizes_of(dev, kt)
        for nh in (L - 5, 2 * L + 5):
            hay, ndl = keys_of_type(kt, nh, 8), keys_of_type(kt, T + 37, 9)
            run_search(dev, kt, hay, ndl[rng.permutation(ndl.size)], BOTH_SIDES, "%s at %s" % (kt, offs), offs=offs)
            run_search(dev, kt, hay, ndl, BOTH_SIDES_SORTED, "%s at %s" % (kt, offs), offs=offs)


def test_more_tiles_than_the_chip_holds(dev):
    T, L, P = sizes_of(dev)
    nh, nn = (1 << 22) + 5, (1 << 21) + 3
    assert nn // T > 256 * 4
    rng = np.random.default_rng(1)
    hay = np.sort(rng.integers(0, 1 << 32, nh, dtype=np.uint64).astype(np.uint32))
    ndl = rng.integers(0, 1 << 20, nn, dtype=np.uint64).astype(np.uint32) << np.uint32(12)    # ties among the needles
    ndl[::5] = hay[rng.integers(0, nh, ndl[::5].size)]                                       # and needles that are present
    run_search(dev, "uint", hay, ndl, ((False, False),), "2^21 + 3 in 2^22 + 5")
    run_search(dev, "uint", hay, np.sort(ndl), ((True, True),), "2^21 + 3 in 2^22 + 5")


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    T, L, P = sizes_of(dev)
    s = clo.Search(ctx, "uint")
    for k, (nh, nn) in enumerate(((9 * L + 3, 40 * T + 1), (5, 9), (0, 3), (3 * L, 60 * T + 7), (L, 3 * T))):
        hay = sorted_uint(nh, k, max(4, nh // 3))
        ndl = np.sort(needles_uint(nn, k + 50, max(4, nh // 3)))
        run_search(dev, "uint", hay, ndl, BOTH_SIDES_SORTED if k % 2 == 0 else ALL_FORMS, "call %d" % k, obj=s)
    s.close()


def test_host_data_form(dev):
    clo, ctx, q = dev
    T, L, P = sizes_of(dev, "int")
    hay, ndl = keys_of_type("int", 2 * L + 1, 1), keys_of_type("int", T + 9, 2)
    mixed = ndl[np.random.default_rng(5).permutation(ndl.size)]
    s = clo.Search(ctx, "int")
    try:
        for upper in (False, True):
            assert np.array_equal(s.with_host_data(hay, mixed, upper=upper, q_exec=q), search(hay, mixed, upper))
            assert np.array_equal(s.with_host_data(hay, ndl, upper=upper, needles_sorted=True), search(hay, ndl, upper))   # a queue of its own
        assert not s.with_host_data(hay[:0], mixed, upper=True, q_exec=q).any()                # an empty haystack: zeros
        assert s.with_host_data(hay, mixed[:0], q_exec=q).size == 0
    finally:
        s.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 needles; the transfers on a queue of their own, then no queue at all (the call makes and destroys
    one); with a haystack and with an empty one, which is not uploaded at all."""
    clo, ctx, q = dev
    T, L, P = sizes_of(dev, "int")
    hay, ndl = keys_of_type("int", 2 * L + 1, 3), keys_of_type("int", 2 * T + 1, 4)
    mixed = ndl[np.random.default_rng(6).permutation(ndl.size)]
    s = clo.Search(ctx, "int")
    qc = clo.Queue(ctx)
    try:
        for qe, qcomm in ((q, qc), (None, None)):
            for upper in (False, True):
                assert np.array_equal(s.with_host_data(hay, mixed, upper=upper, q_exec=qe, q_comm=qcomm), search(hay, mixed, upper)), (qe is None, qcomm is None, upper)
            assert np.array_equal(s.with_host_data(hay, ndl, needles_sorted=True, q_exec=qe, q_comm=qcomm), search(hay, ndl, False)), (qe is None, qcomm is None)
            assert not s.with_host_data(hay[:0], mixed, upper=True, q_exec=qe, q_comm=qcomm).any(), (qe is None, qcomm is None)
    finally:
        s.close()
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    nh, nn = 5000, 3000
    need = lib.clo_hip_search_workspace_bytes(nh, nn, SORTED)
    assert need > 0 and need % 256 == 0 and lib.clo_hip_search_workspace_bytes(nh, nn, 0) == 0
    hay = Region(dev, 4 * nh + 16, 0, sorted_uint(nh + 4, 1, 900), 0)
    ndl = Region(dev, 4 * nn + 16, 0, np.sort(needles_uint(nn + 4, 2, 900)), 1)
    pos = Region(dev, 4 * nn + 16, 0, None, 2)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(h, n_h, x, n_x, out, ks=4, kind=0, flags=SORTED, mg=0, w=ws.ptr, wb=need):
        return lib.clo_hip_search(h, n_h, x, n_x, out, ks, kind, flags, mg, w, wb, s)

    try:
        full = (hay.ptr, nh, ndl.ptr, nn, pos.ptr)
        for kind in (-1, 3):
            assert call(*full, kind=kind) == EARGS
        for ks in (3, 16, 0):
            assert call(*full, ks=ks) == EUNSUPPORTED, ks
        assert call(*full, ks=1, kind=2) == EUNSUPPORTED                                              # no 1-byte floats
        for flags in (4, 7, 1 << 31):
            assert call(*full, flags=flags) == EARGS
        assert call(hay.ptr, 1 << 32, ndl.ptr, nn, pos.ptr) == EARGS
        assert call(hay.ptr, nh, ndl.ptr, 1 << 32, pos.ptr) == EARGS
        assert call(None, nh, ndl.ptr, nn, pos.ptr) == EARGS                                          # a missing array
        assert call(hay.ptr, nh, None, nn, pos.ptr) == EARGS
        assert call(hay.ptr, nh, ndl.ptr, nn, None) == EARGS
        for i in (0, 2, 4):                                                                         # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        args = list(full)
        args[0] += 4
        assert call(*args, ks=8, kind=2) == EARGS                                                   # 4-aligned is not 8-aligned
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                 # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE           # short
        q.finish()
        pos.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; no workspace where none is needed; 8-byte keys
        # of kind 2 over the same bytes; no needles; an empty haystack with a NULL pointer
        assert call(*full) == 0
        assert call(*full, flags=UPPER, w=None, wb=0) == 0
        assert call(hay.ptr, nh // 2, ndl.ptr, nn // 2, pos.ptr, ks=8, kind=2, flags=0, w=None, wb=0) == 0
        assert call(hay.ptr, nh, None, 0, None, w=None, wb=0) == 0
        assert call(None, 0, ndl.ptr, nn, pos.ptr, flags=SORTED | UPPER, w=None, wb=0) == 0
        q.finish()
        pos.check(np.zeros(nn, np.uint32), "an empty haystack")
    finally:
        ws.close()
        for r in (hay, ndl, pos):
            r.close()


@pytest.mark.parametrize("path", ["general", "sorted"])
def test_graph_capture_and_replay(dev, path):
    """clo_hip_search captured from a client stream after one eager warm-up and replayed three times on new contents of
    the same buffers, pos_out refilled with a canary before each (the protocol of test_gpu_graph_capture.py)."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T, L, P = sizes_of(dev)
    nh, nn = 2 * L + 5, 2 * T + 3
    flags = UPPER | (SORTED if path == "sorted" else 0)
    need = lib.clo_hip_search_workspace_bytes(nh, nn, flags)
    assert (need > 0) == (path == "sorted")
    made = [GC.Mem(gdev, x) for x in (4 * nh, 4 * nn, 4 * nn, max(need, 256))]
    hb, nb, pb, ws = made
    kinds = ["uniform", "all equal", "needles below", "needles above", "uniform"]
    sent = {}

    def load(k):
        rng = np.random.default_rng(100 + k)
        if kinds[k] == "uniform":
            hay, ndl = np.sort(rng.integers(0, nh, nh).astype(np.uint32)), rng.integers(0, nh, nn).astype(np.uint32)
        elif kinds[k] == "all equal":
            hay, ndl = np.full(nh, 9 + k, np.uint32), np.full(nn, 9 + k, np.uint32)
        else:
            hay = np.arange(nh, dtype=np.uint32) + np.uint32(nn + 5)
            ndl = np.arange(nn, dtype=np.uint32) + (np.uint32(0) if kinds[k] == "needles below" else np.uint32(nh + nn + 9))
        if path == "sorted":
            ndl = np.sort(ndl)
        sent[k] = (hay, ndl)
        pb.fill()
        hb.put(hay)
        nb.put(ndl)
        return search(hay, ndl, True)

    def enqueue():
        return lib.clo_hip_search(hb.ptr, nh, nb.ptr, nn, pb.ptr, 4, 0, flags, 0, ws.ptr if need else None, need, q.stream)

    def verify(k, want):
        tag = "%s round %d (%s)" % (path, k, kinds[k])
        GC.same(pb.get(np.uint32, nn), want, tag + ": pos_out")
        GC.same(hb.get(np.uint32, nh), sent[k][0], tag + ": haystack")
        GC.same(nb.get(np.uint32, nn), sent[k][1], tag + ": needles")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


@pytest.mark.parametrize("broken", ["random haystack", "descending haystack", "random needles under the sorted flag"])
def test_broken_preconditions_stay_in_bounds(dev, broken):
    """The bounds contract: the precondition is broken, the contents are unspecified and not compared; the call
    succeeds, the guards around pos_out are intact, the inputs unchanged and every position <= numel_h. (Every search
    halves a range fixed by the sizes, and the sorted tiles clamp the ranges they read from the workspace.)"""
    T, L, P = sizes_of(dev)
    rng = np.random.default_rng(9)
    nh, nn = 2 * L + 5, 2 * T + 3
    rand = lambda n: rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    if broken == "random haystack":
        hay, ndl, forms = rand(nh), np.sort(rand(nn)), ALL_FORMS
    elif broken == "descending haystack":
        hay, ndl, forms = np.arange(nh, 0, -1, dtype=np.uint32) * np.uint32(3), np.sort(rand(nn) % np.uint32(3 * nh)), ALL_FORMS
    else:
        hay, ndl, forms = np.sort(rand(nh)), rand(nn), BOTH_SIDES_SORTED
    run_search(dev, "uint", hay, ndl, forms, broken, compare=False)
    for kt in ("uchar", "double"):
        run_search(dev, kt, hay.astype(_NP[kt]), ndl.astype(_NP[kt]), forms, "%s, %s" % (broken, kt), compare=False)
