"""CloTopK (include/clo_topk.h) on the GPU against the numpy model of tests/topk_model.py, bit for bit. Every array is a
view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs hold exactly m = min(k, numel) rows unless a test says otherwise, so a row >= m is a
guard byte; outputs and kth_out are pre-filled with the pattern, and after every call the m rows and kth_out equal the
model's and the guards and every input are unchanged. With T = clo_hip_topk_tile and S = clo_hip_topk_sorted_max: sizes
around the tile edges x k around the ends, both directions and both orders; ties cut at every kind of place; keys that
differ in one digit only; every key type with its special values; every value form; the cap of the sorted order;
element-aligned views; a tile count that sends the count scan through its loop a second time; kth_out feeding two
CloSelect objects on the same stream; the library's own argsort; one object large, small, large; two objects on two
streams; the host-data form; the thin ABI's status codes; clo_hip_topk captured into a linear graph and replayed after
the keys were rewritten; a seeded fuzz; two cases with element indices above 2^31; and, for keys of 2, 4 and 8 bytes of
a signed or floating kind, one tile more than the digit sweep has work-groups (clo_hip_topk_sweep_groups), every winner
in that tile. (tests/test_gpu_fuzz.py has the stratified fuzz over every kernel instantiation.)"""
import numpy as np
import pytest

from merge_model import sort_keys
from topk_model import WHICH, ORDERS, topk
from test_gpu_histogram import Region
from test_gpu_merge import KEY_TYPES, _NP, keys_of_type

pytestmark = pytest.mark.gpu

# value forms: keys only; 4-byte values; 8-byte values; indices with keys_out; indices alone; the k-th key alone
_VS = {"keys": 0, "v4": 4, "v8": 8, "arg": 4, "arg_only": 4, "kth_only": 0}
MODES = ("keys", "v4", "v8", "arg", "arg_only")


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def tile_of(dev, kt, mode="keys"):
    t = dev[0].topk_tile(np.dtype(_NP[kt]).itemsize, _VS[mode])
    assert t > 0 and t % 1024 == 0
    return t


def cap_of(dev, kt, mode="keys"):
    s = dev[0].topk_sorted_max(np.dtype(_NP[kt]).itemsize, _VS[mode])
    assert s >= 1024
    return s


def values_for(mode, n):
    """Values that carry the element's index; the 8-byte ones with a non-zero high word that differs per element."""
    if mode == "v4":
        return np.arange(n, dtype=np.uint32) ^ np.uint32(0x5A000000)
    if mode == "v8":
        i = np.arange(n, dtype=np.uint64)
        return ((np.uint64(0xC0DE0000) + (i * np.uint64(2654435761) & np.uint64(0xFFFF))) << np.uint64(32)) | i
    return None


def run_topk(dev, which, order, kt, keys, k, mode, what, offs=(0, 0, 0, 0, 0), obj=None, q=None, kth=True, spare_rows=0):
    """One call on views at byte offsets offs = (keys_in, values_in, keys_out, values_out, kth_out), the outputs of m +
    spare_rows rows; checks everything and returns (p, kth) of the model."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    dt = np.dtype(_NP[kt])
    keys = np.ascontiguousarray(keys, dtype=dt)
    n, vs = keys.size, _VS[mode]
    m = min(k, n)
    what = "%s %s %s %s, n = %d, k = %d, %s" % (which, order, kt, mode, n, k, what)
    vals = values_for(mode, n)
    s = obj or clo.TopK(which, order, ctx, kt, vs)
    k_r = Region(rdev, keys.nbytes, offs[0], keys, 0)
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if vals is not None else None
    ko_r = Region(rdev, (m + spare_rows) * dt.itemsize, offs[2], None, 2) if mode in ("keys", "v4", "v8", "arg") else None
    vo_r = Region(rdev, (m + spare_rows) * vs, offs[3], None, 2) if vs else None
    kth_r = Region(rdev, dt.itemsize, offs[4], None, 1) if kth or mode == "kth_only" else None
    view = lambda r: r.view if r is not None else None
    try:
        assert s.with_device_data(q, k_r.view, view(v_r), view(ko_r), view(vo_r), view(kth_r), n, k), what
        q.finish()
        p, want_kth = topk(which, order, keys, k)
        assert p.size == m
        if ko_r:
            ko_r.check(keys[p], what + ": keys_out")                   # ... and nothing behind the m rows
        if vo_r:
            vo_r.check(vals[p] if vals is not None else p, what + ": values_out")
        if kth_r:
            kth_r.check(want_kth if m else None, what + ": kth_out")
        k_r.check(keys, what + ": keys_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return p, want_kth
    finally:
        for r in (k_r, v_r, ko_r, vo_r, kth_r):
            if r:
                r.close()
        if obj is None:
            s.close()


def refused(dev, which, order, kt, n, k, mode="keys"):
    """The call comes back with CLO_ERROR_ARGS and writes nothing."""
    clo, ctx, q = dev
    from cl_ops_amd.api import CLO_ERROR_ARGS
    dt = np.dtype(_NP[kt])
    keys = np.zeros(n, dt)
    s = clo.TopK(which, order, ctx, kt, _VS[mode])
    k_r, ko_r, vo_r = Region(dev, keys.nbytes, 0, keys, 0), Region(dev, n * dt.itemsize, 0, None, 2), Region(dev, n * 4, 0, None, 2)
    try:
        with pytest.raises(clo.CloError) as e:
            s.with_device_data(q, k_r.view, None, ko_r.view, vo_r.view if _VS[mode] else None, None, n, k)
        assert e.value.code == CLO_ERROR_ARGS, e.value
        q.finish()
        ko_r.check(None, "a refused call wrote keys_out")
        vo_r.check(None, "a refused call wrote values_out")
        return e.value.message
    finally:
        for x in (k_r, ko_r, vo_r, s):
            x.close()


@pytest.mark.parametrize("order", ORDERS)
@pytest.mark.parametrize("which", WHICH)
def test_sizes(dev, which, order):
    """n in {1, 2, 63, 64, 65, T - 1, T, T + 1, 2 T + 3, 5 T + 17} x k in {1, 2, n / 2, n - 1, n, n + 1, 10 n}; "sorted"
    where m <= S; the value forms take turns. Few distinct keys: every cut falls inside a tie run."""
    case = 0
    for which_n in range(10):
        for which_k in range(7):
            mode = MODES[case % len(MODES)]
            case += 1
            T, S = tile_of(dev, "uint", mode), cap_of(dev, "uint", mode)
            n = (1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3, 5 * T + 17)[which_n]
            k = (1, 2, n // 2, n - 1, n, n + 1, 10 * n)[which_k]
            keys = np.random.default_rng(case).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
            keys[::2] &= np.uint32(0x30000007)
            if order == "sorted" and min(k, n) > S:
                assert "cap" in refused(dev, which, order, "uint", n, k)
                continue
            run_topk(dev, which, order, "uint", keys, k, mode, "sizes", kth=case % 3 != 0)


@pytest.mark.parametrize("which", WHICH)
def test_ties(dev, which):
    """Where the m-th key has ties the lowest indices are taken: all keys equal with k in the middle; two distinct keys
    with the cut inside a run of the k-th key that spans a tile edge; the k-th key's equal elements one per tile, at the
    first and at the last slot of the tile, with r = 1, the number of tiles minus 1, and all of them; the k-th key equal
    to the type's smallest and largest value."""
    T = tile_of(dev, "uint", "arg")
    tiles = 5
    n = tiles * T + 9
    best, kth_key, rest = (3, 50, 900) if which == "smallest" else (900, 50, 3)       # better than, equal to, worse than the k-th key
    for j, mode in enumerate(("arg", "v4", "keys")):
        keys = np.full(n, 77, np.uint32)
        p, _ = run_topk(dev, which, "input", "uint", keys, n // 2 + j, mode, "all keys equal")
        assert p.tolist() == list(range(n // 2 + j))
    # two distinct keys: a run of the k-th key from T - 100 to T + 100, the cut at every quarter of it
    keys = np.full(n, best, np.uint32)
    keys[T - 100:T + 100] = kth_key
    keys[3 * T:] = kth_key
    eq_at = np.flatnonzero(keys == kth_key)
    for cut in (1, 50, 100, 101, 199, 200, 201):
        p, kth = run_topk(dev, which, "input", "uint", keys, (3 * T - 200) + cut, "arg", "the cut %d into a run across a tile edge" % cut)
        assert kth[0] == kth_key and p[keys[p] == kth_key].tolist() == eq_at[:cut].tolist()
    T8 = tile_of(dev, "uint", "v8")
    n8 = tiles * T8 + 9
    for slot in (0, T8 - 1):
        keys = np.full(n8, rest, np.uint32)
        keys[1::11] = best
        at = np.arange(tiles) * T8 + slot
        keys[at] = kth_key
        nbest = int((keys == best).sum())
        assert nbest + tiles <= cap_of(dev, "uint", "v8")
        for r in (1, tiles - 1, tiles):
            for order in ORDERS:
                p, kth = run_topk(dev, which, order, "uint", keys, nbest + r, "v8", "one equal element per tile at slot %d, r = %d" % (slot, r))
                assert kth[0] == kth_key and sorted(set(p.tolist()) & set(at.tolist())) == at[:r].tolist()
    # the k-th key is the type's smallest / largest value (x = 0 and x = all ones, in both directions)
    for kt in ("uint", "int", "float", "uchar"):
        dt = np.dtype(_NP[kt])
        if dt.kind == "f":
            lo, hi = np.array([0xFFFFFFFF], np.uint32).view(dt)[0], np.array([0x7FFFFFFF], np.uint32).view(dt)[0]    # the NaNs at the ends
            mid = dt.type(1.5)
        else:
            lo, hi, mid = np.iinfo(dt).min, np.iinfo(dt).max, 7
        for end in (lo, hi):
            keys = np.full(2 * tile_of(dev, kt, "arg") + 5, mid, dt)
            keys[5::3] = end
            nend = int((keys.view("u%d" % dt.itemsize) == np.array([end], dt).view("u%d" % dt.itemsize)[0]).sum())
            is_best = (end == lo if dt.kind != "f" else bool(np.signbit(end))) == (which == "smallest")
            for k in ((1, nend - 1, nend) if is_best else (keys.size - nend + 1, keys.size - 1, keys.size)):
                _, kth = run_topk(dev, which, "input", kt, keys, k, "arg", "the k-th key is the type's end")
                assert kth.tobytes() == np.array([end], dt).tobytes()


@pytest.mark.parametrize("kt", ["uint", "ulong", "float", "long"])
def test_digits(dev, kt):
    """Keys that differ only in one 8-bit digit of the order key, for every digit position; keys that differ only in
    the top bit and only in bit 0. A wrong prefix or a rank off by one at any level shows here."""
    dt = np.dtype(_NP[kt])
    ut = np.dtype("u%d" % dt.itemsize)
    T = tile_of(dev, kt, "arg")
    n = T + 77
    rng = np.random.default_rng(dt.itemsize)
    base = int(rng.integers(0, 1 << 62)) & ((1 << (8 * dt.itemsize)) - 1) & ~(1 << (8 * dt.itemsize - 1)) & ~(0x7F8 << (8 * dt.itemsize - 12))
    case = 0
    for d in range(dt.itemsize):
        digit = rng.integers(0, 256, n).astype(np.uint64)
        bits = (np.uint64(base & ~(0xFF << (8 * d))) | (digit << np.uint64(8 * d))).astype(ut)
        if dt.kind == "f":
            bits[np.isnan(bits.view(dt))] = base                                  # (an all-ones exponent digit: keep the floats ordinary)
        for k in (1, 2, n // 3, n - 1):
            for which in WHICH:
                case += 1
                run_topk(dev, which, ORDERS[case % 2] if k <= cap_of(dev, kt, "arg") else "input", kt, bits.view(dt), k, MODES[case % 5], "digit %d varies" % d)
    for bit in (8 * dt.itemsize - 1, 0):
        bits = (np.uint64(base) ^ (rng.integers(0, 2, n).astype(np.uint64) << np.uint64(bit))).astype(ut)
        ones = int((bits != ut.type(base)).sum())
        for k in (1, ones, ones + 1, n - ones, n - ones + 1, n):
            for which in WHICH:
                run_topk(dev, which, "input", kt, bits.view(dt), k, "arg", "bit %d varies" % bit)


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_and_value_forms(dev, kt):
    """Every key type: few distinct keys that include the type's specials (+-0, +-inf, NaNs of both signs and several
    payloads, the integers' ends) in random order; both directions, both orders, every value form, kth_out NULL and
    given, the k-th key alone."""
    rng = np.random.default_rng(len(kt) * 131 + ord(kt[0]))
    case = 0
    for which in WHICH:
        for mode in MODES + ("kth_only",):
            T, S = tile_of(dev, kt, mode), cap_of(dev, kt, mode)
            keys = rng.permutation(keys_of_type(kt, 2 * T + 3, 5 + case))
            for order, k in (("input", int(rng.integers(1, keys.size))), ("sorted", int(rng.integers(1, S)))):
                case += 1
                run_topk(dev, which, order, kt, keys, k, mode, "specials", kth=case % 2 == 0)


def test_the_sorted_cap(dev):
    """"sorted" at m = S works and k = S + 1 is refused; "sorted largest" is descending with ties by ascending index."""
    for kt, mode in (("uint", "arg"), ("double", "v8"), ("ushort", "keys"), ("ulong", "v4")):
        S = cap_of(dev, kt, mode)
        n = 3 * S + 11
        keys = np.random.default_rng(S).permutation(keys_of_type(kt, n, 3))
        for which in WHICH:
            p, _ = run_topk(dev, which, "sorted", kt, keys, S, mode, "m = S")
            assert p.size == S
            assert "cap" in refused(dev, which, "sorted", kt, n, S + 1, mode if mode != "v8" and mode != "v4" else "arg")
        # k above the cap is fine where numel is not
        run_topk(dev, "largest", "sorted", kt, keys[:S], 10 * S, mode, "numel = S, k = 10 S")
    keys = np.random.default_rng(5).integers(0, 40, 5000).astype(np.int32) - 20
    p, _ = run_topk(dev, "largest", "sorted", "int", keys, 1000, "arg", "descending")
    got = keys[p].astype(np.int64)
    assert (np.diff(got) <= 0).all() and (np.diff(p.astype(np.int64))[np.diff(got) == 0] > 0).all()
    p, _ = run_topk(dev, "smallest", "sorted", "int", keys, 1000, "arg", "ascending")
    got = keys[p].astype(np.int64)
    assert (np.diff(got) >= 0).all() and (np.diff(p.astype(np.int64))[np.diff(got) == 0] > 0).all()


def test_element_aligned_views_and_exact_outputs(dev):
    """Every array one element past a 16-byte boundary: nothing may assume more than the element's alignment. The
    outputs hold exactly m rows (run_topk's default), and larger ones keep their rows >= m."""
    cases = (("uchar", "v8", (1, 8, 1, 8, 1)), ("char", "arg", (1, 0, 1, 4, 3)), ("ushort", "v4", (2, 4, 2, 4, 2)), ("uint", "keys", (4, 0, 4, 0, 4)),
             ("uint", "v4", (4, 4, 12, 4, 8)), ("float", "arg", (4, 0, 4, 4, 12)), ("ulong", "v8", (8, 8, 8, 8, 8)), ("double", "arg_only", (8, 0, 0, 4, 8)),
             ("half", "keys", (2, 0, 6, 0, 14)))
    for i, (kt, mode, offs) in enumerate(cases):
        T = tile_of(dev, kt, mode)
        keys = np.random.default_rng(i).permutation(keys_of_type(kt, 2 * T + 37, 8 + i))
        for j, which in enumerate(WHICH):
            run_topk(dev, which, "input", kt, keys, T + 13 + i, mode, "views at %s" % (offs,), offs=offs, spare_rows=j * 5)
            run_topk(dev, which, "sorted", kt, keys, 1000 + i, mode, "views at %s" % (offs,), offs=offs, spare_rows=(1 - j) * 3)


def test_the_scans_take_a_second_trip(dev):
    """One tile more than the count scan takes per trip of its loop, and 7 elements: the carry from trip to trip, for
    both counts (the keys before the k-th and the keys equal to it, spread over every tile)."""
    from cl_ops_amd.topk import TOPK_SCAN_TRIP
    T = tile_of(dev, "uint", "keys")
    n = (TOPK_SCAN_TRIP + 1) * T + 7
    assert -(-n // T) == TOPK_SCAN_TRIP + 2
    keys = np.random.default_rng(3).integers(0, 3, n).astype(np.uint32) * np.uint32(1000)      # 0, 1000, 2000: a third each
    below = int((keys < 1000).sum())
    run_topk(dev, "smallest", "input", "uint", keys, below + n // 6, "keys", "%d tiles" % (TOPK_SCAN_TRIP + 2))
    run_topk(dev, "largest", "input", "uint", keys, int((keys > 1000).sum()) + n // 5, "arg_only", "%d tiles" % (TOPK_SCAN_TRIP + 2))


@pytest.mark.parametrize("kt", ["ushort", "half", "int", "float", "long", "double"])
def test_the_digit_sweep_takes_a_second_trip(dev, kt):
    """The digit sweep launches G = clo_hip_topk_sweep_groups() work-groups at most, and a group adds the tiles blockIdx.x,
    blockIdx.x + G, ... into its LDS counters. n = (G + 1) Td + 5 (Td: the sweep's tile): tile G and the five elements
    behind it are the second trip of groups 0 and 1. The keys come from 300 distinct values in the library's order: the
    middle 100 before index G Td, the lowest 100 and the highest 100 mixed behind it, so that the k smallest and the k
    largest all lie in the second trip. A sweep that stops after its first trip counts none of them, and the k-th key
    and the rows come out wrong. "smallest, input" with keys_out, then "largest, sorted" in arg form below the cap."""
    dt = np.dtype(_NP[kt])
    G, Td = dev[0].topk_sweep_groups(), tile_of(dev, kt, "keys")
    assert G >= 1
    n = (G + 1) * Td + 5
    assert n > G * Td and -(-n // Td) == G + 2
    rng = np.random.default_rng(dt.itemsize * 7 + len(kt))
    words = np.unique(rng.integers(0, 1 << (8 * dt.itemsize - 1), 400, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 400, dtype=np.uint64))
    pool = sort_keys(rng.permutation(words.astype("u%d" % dt.itemsize))[:300].view(dt))
    assert pool.size == 300
    keys = np.empty(n, dt)
    keys[:G * Td] = pool[rng.integers(100, 200, G * Td)]
    ends = rng.integers(0, 200, n - G * Td)
    keys[G * Td:] = pool[np.where(ends < 100, ends, ends + 100)]
    nlow, nhigh = int((ends < 100).sum()), int((ends >= 100).sum())
    k1, k2 = nlow // 2, min(cap_of(dev, kt, "arg"), 2 * nhigh // 3)
    assert 0 < k1 < nlow and 0 < k2 < nhigh
    p, _ = run_topk(dev, "smallest", "input", kt, keys, k1, "keys", "every winner in the sweep's second trip")
    assert p.size == k1 and int(p.min()) >= G * Td
    p, _ = run_topk(dev, "largest", "sorted", kt, keys, k2, "arg", "every winner in the sweep's second trip")
    assert p.size == k2 and int(p.min()) >= G * Td


def test_kth_out_feeds_two_selects(dev):
    """kth_out is the threshold of two CloSelect objects on the same stream, with no host wait in between: the strict
    one keeps fewer than m elements, the other at least m."""
    clo, ctx, q = dev
    T = tile_of(dev, "int", "keys")
    n = 3 * T + 11
    keys = np.random.default_rng(77).integers(-300, 300, n).astype(np.int32)
    for which, strict, loose, k in (("smallest", "lt", "le", n // 3), ("largest", "gt", "ge", n // 5)):
        k_r, kth_r = Region(dev, keys.nbytes, 0, keys, 0), Region(dev, 4, 0, None, 1)
        o1, o2 = Region(dev, keys.nbytes, 0, None, 2), Region(dev, keys.nbytes, 0, None, 2)
        n1, n2 = Region(dev, 8, 0, None, 1), Region(dev, 8, 0, None, 1)
        t, s1, s2 = clo.TopK(which, "input", ctx, "int", 0), clo.Select("select", strict, ctx, "int", 0), clo.Select("select", loose, ctx, "int", 0)
        try:
            assert t.with_device_data(q, k_r.view, None, None, None, kth_r.view, n, k)
            assert s1.with_device_data(q, k_r.view, None, kth_r.view, o1.view, None, n1.view, n)
            assert s2.with_device_data(q, k_r.view, None, kth_r.view, o2.view, None, n2.view, n)
            q.finish()
            kth = topk(which, "input", keys, k)[1]
            kth_r.check(kth, "kth_out")
            count = lambda r: int(r.base.read(q, np.uint8, r.host.size)[r.at:r.at + 8].view(np.uint64)[0])
            c1, c2 = count(n1), count(n2)
            cmp_ = (lambda a, b: a < b) if which == "smallest" else (lambda a, b: a > b)
            assert c1 == int(cmp_(keys, kth[0]).sum()) and c2 == c1 + int((keys == kth[0]).sum())
            assert c1 < k <= c2, (which, c1, k, c2)
        finally:
            for x in (k_r, kth_r, o1, o2, n1, n2, t, s1, s2):
                x.close()


@pytest.mark.parametrize("kt", ["uint", "int", "float"])
def test_against_the_librarys_own_sort(dev, kt):
    """"smallest, sorted" in arg form equals the first m rows of the library's own argsort (clo_sort_by_key_*)."""
    clo, ctx, q = dev
    T = tile_of(dev, kt, "arg")
    n, m = 3 * T + 7, cap_of(dev, kt, "arg")
    keys = np.random.default_rng(3).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[::3] &= np.uint32(0x80000003)                                          # ties, of both signs
    if kt == "float":
        keys[::17] = np.resize(np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc00002], np.uint32), keys[::17].shape)
    B = lambda nbytes: clo.Buffer(ctx, nbytes)
    kin, sk, sv, tk, tv = B(4 * n), B(4 * n), B(4 * n), B(4 * m), B(4 * m)
    s, t = clo.Sorter("satradix", ctx, kt), clo.TopK("smallest", "sorted", ctx, kt, 4)
    try:
        kin.write(q, keys)
        s.by_key_with_device_data(q, kin, None, sk, sv, n)
        t.with_device_data(q, kin, None, tk, tv, None, n, m)
        q.finish()
        assert np.array_equal(tk.read(q, np.uint32, m), sk.read(q, np.uint32, n)[:m])
        assert np.array_equal(tv.read(q, np.uint32, m), sv.read(q, np.uint32, n)[:m])
    finally:
        for x in (kin, sk, sv, tk, tv, s, t):
            x.close()


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    for which, order in (("smallest", "input"), ("largest", "sorted")):
        s = clo.TopK(which, order, ctx, "uint", 4)
        for j, n in enumerate((40 * T + 3, 5, 0, 70 * T + 7, 3 * T)):
            keys = np.random.default_rng(30 + j).integers(0, 1 << 16, n).astype(np.uint32)
            run_topk(dev, which, order, "uint", keys, (777, 3, 4, 2000, 0)[j], "v4" if j % 2 == 0 else "arg", "call %d" % j, obj=s)
        s.close()


def test_two_objects_on_two_streams(dev):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds."""
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    n, k = 150 * T + 9, 3000
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("smallest", "input", "v4"), ("largest", "sorted", "arg"))
    objs = [clo.TopK(which, order, ctx, "uint", 4) for which, order, _ in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (which, order, mode) in enumerate(specs):
                keys = np.random.default_rng(50 + 10 * rnd + i).integers(0, 1 << 14, n).astype(np.uint32)
                vals = values_for(mode, n)
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, keys.nbytes, 0, keys, 0), Region(rdev, vals.nbytes, 0, vals, 1) if vals is not None else None,
                        Region(rdev, 4 * k, 0, None, 2), Region(rdev, 4 * k, 0, None, 2), Region(rdev, 4, 0, None, 1)]
                sent.append((keys, vals, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (keys, vals, regs) in enumerate(sent):
                view = lambda r: r.view if r is not None else None
                assert objs[i].with_device_data(qs[i], regs[0].view, view(regs[1]), regs[2].view, regs[3].view, regs[4].view, n, k)
            for i in range(2):
                qs[i].finish()
            for i, (keys, vals, regs) in enumerate(sent):
                which, order, mode = specs[i]
                p, kth = topk(which, order, keys, k)
                what = "round %d, %s %s" % (rnd, which, order)
                regs[2].check(keys[p], what + ": keys_out")
                regs[3].check(vals[p] if vals is not None else p, what + ": values_out")
                regs[4].check(kth, what + ": kth_out")
                for r in regs:
                    if r:
                        r.close()
    finally:
        for x in objs + qs:
            x.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "v8", "arg", "arg_only"])
def test_host_data_form(dev, mode):
    clo, ctx, q = dev
    T = tile_of(dev, "int", mode)
    keys = np.random.default_rng(1).permutation(keys_of_type("int", 2 * T + 9, 1))
    vals = values_for(mode, keys.size)
    for which in WHICH:
        for order, k in (("input", T + 5), ("sorted", 500), ("input", 10 * keys.size)):
            s = clo.TopK(which, order, ctx, "int", _VS[mode])
            ko, vo, kth = s.with_host_data(keys, k, vals, keys_out=mode != "arg_only", kth=which == "largest", q_exec=q if mode != "v4" else None)
            p, want_kth = topk(which, order, keys, k)
            assert (ko is None) == (mode == "arg_only") and (vo is None) == (mode == "keys")
            if ko is not None:
                assert np.array_equal(ko, keys[p]), (which, order)
            if vo is not None:
                assert np.array_equal(vo, vals[p] if vals is not None else p), (which, order)
            assert (kth is None) if which == "smallest" else kth == want_kth[0]
            s.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 elements; the transfers on a queue of their own, then no queue at all (the call makes and destroys
    one); both orders, with values."""
    clo, ctx, q = dev
    T = tile_of(dev, "int", "v4")
    keys = np.random.default_rng(2).permutation(keys_of_type("int", 2 * T + 1, 3))
    vals = values_for("v4", keys.size)
    qc = clo.Queue(ctx)
    try:
        for which in WHICH:
            for order, k in (("input", T + 5), ("sorted", 500)):
                s = clo.TopK(which, order, ctx, "int", 4)
                p, want_kth = topk(which, order, keys, k)
                for qe, qcomm in ((q, qc), (None, None)):
                    ko, vo, kth = s.with_host_data(keys, k, vals, q_exec=qe, q_comm=qcomm)
                    what = (which, order, qe is None, qcomm is None)
                    assert np.array_equal(ko, keys[p]) and np.array_equal(vo, vals[p]) and kth == want_kth[0], what
                s.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    n, k = 1000, 100
    need = lib.clo_hip_topk_workspace_bytes(n, 4, 4)
    assert need > 0 and need % 256 == 0
    S = lib.clo_hip_topk_sorted_max(4, 4)
    keys = np.random.default_rng(5).integers(0, 100, 2 * n + 4, dtype=np.uint32)
    ki = Region(dev, 8 * n + 16, 0, keys, 0)
    vi, ko, vo = (Region(dev, 16 * n + 16, 0, None, i) for i in range(3))
    kth = Region(dev, 16, 0, None, 0)
    big, vbig = Region(dev, 4 * (S + 50), 0, np.arange(S + 50, dtype=np.uint32), 1), Region(dev, 4 * S, 0, None, 2)
    ws = clo.Buffer(ctx, need + lib.clo_hip_topk_workspace_bytes(S + 50, 4, 4) + 256)
    s = q.stream

    def call(k_p, v_p, ko_p, vo_p, kth_p=None, which=0, order=0, numel=n, k_=k, ks=4, kind=0, vs=4, w=ws.ptr, wb=need):
        return lib.clo_hip_topk(which, order, k_p, v_p, ko_p, vo_p, kth_p, numel, k_, ks, kind, vs, w, wb, s)

    try:
        full = (ki.ptr, vi.ptr, ko.ptr, vo.ptr, kth.ptr)
        for which in (-1, 2, 100):
            assert call(*full, which=which) == EARGS
        for order in (-1, 2, 100):
            assert call(*full, order=order) == EARGS
        for kind in (-1, 3):
            assert call(*full, kind=kind) == EARGS
        for ks, vs in ((3, 4), (16, 4), (0, 0), (4, 2), (4, 16)):
            assert call(*full, ks=ks, vs=vs) == EUNSUPPORTED, (ks, vs)
        assert call(*full, ks=1, kind=2) == EUNSUPPORTED                                                # no 1-byte floating-point keys
        assert call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, ko.ptr, vo.ptr) == EARGS                                              # the keys are always read
        assert call(ki.ptr, vi.ptr, ko.ptr, None) == EARGS                                              # values_out with value_size 4
        assert call(ki.ptr, None, None, None, vs=0) == EARGS                                            # nothing to write
        assert call(ki.ptr, None, ko.ptr, vo.ptr, vs=8) == EARGS                                        # the arg form is 4-byte
        assert call(ki.ptr, vi.ptr, ko.ptr, None, vs=0) == EARGS                                        # values with value_size 0
        assert call(ki.ptr, None, ko.ptr, vo.ptr, vs=0) == EARGS
        for i in range(5):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        args = list(full)
        args[1] += 4
        assert call(*args, vs=8) == EARGS                                                               # 4-aligned is not 8-aligned
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        assert call(big.ptr, None, ko.ptr, vo.ptr, order=1, numel=S + 50, k_=S + 1, wb=need + 4096) == EARGS   # "sorted" above the cap
        q.finish()
        for r in (ko, vo, kth):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; numel 0 and k 0 need no workspace and write
        # nothing; the k-th key alone; 8-byte keys of kind 2 over the same bytes
        assert call(None, None, ko.ptr, vo.ptr, kth.ptr, numel=0, w=None, wb=0) == 0
        assert call(ki.ptr, None, ko.ptr, vo.ptr, kth.ptr, k_=0, w=None, wb=0) == 0
        q.finish()
        for r in (ko, vo, kth):
            r.check(None, "an empty thin call wrote")
        assert call(*full) == 0
        q.finish()
        p, want = topk("smallest", "input", keys[:n], k)
        vo.check(vi.contents(np.uint32)[p], "thin: values_out")
        ko.check(keys[p], "thin: keys_out")
        kth.check(want, "thin: kth_out")
        assert call(ki.ptr, None, None, None, kth.ptr, which=1, vs=0, k_=7) == 0
        q.finish()
        kth.check(topk("largest", "input", keys[:n], 7)[1], "thin: the k-th key alone")
        assert call(ki.ptr, None, None, None, kth.ptr, ks=8, kind=2, vs=0, numel=n // 2, k_=11) == 0
        q.finish()
        kth.check(topk("smallest", "input", keys.view(np.float64)[:n // 2], 11)[1], "thin: 8-byte keys")
        assert call(big.ptr, None, None, vbig.ptr, order=1, which=1, numel=S + 50, k_=S, wb=need + 4096) == 0   # the cap itself, no keys_out
        q.finish()
        vbig.check(topk("largest", "sorted", np.arange(S + 50, dtype=np.uint32), S)[0], "thin: sorted at the cap without keys_out")
    finally:
        ws.close()
        for r in (ki, vi, ko, vo, kth, big, vbig):
            r.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "arg"])
def test_graph_capture_and_replay(dev, mode):
    """Two calls of clo_hip_topk — "smallest, input" and "largest, sorted" — captured from one client stream (a linear
    graph) after one eager warm-up and replayed three times, the keys rewritten and the outputs refilled with a canary
    before each replay (the protocol of test_gpu_graph_capture.py): the rows and the k-th keys follow the buffers. k is
    baked into the captured launches."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T = tile_of(dev, "uint", mode)
    n, vs, k1, k2 = 3 * T + 5, _VS[mode], T + 9, 700
    valued = mode == "v4"
    need = lib.clo_hip_topk_workspace_bytes(n, 4, vs)
    made = [GC.Mem(gdev, x) for x in (4 * n, 4 * n, 4 * k1, 4 * k1, 4, 4 * k2, 4 * k2, 4, need, need)]
    ki, vi, ko1, vo1, kth1, ko2, vo2, kth2, ws1, ws2 = made
    vals = values_for("v4", n)
    spans = [1 << 32, 5, 1 << 10, 2, 1 << 20]
    seen = set()

    def load(r):
        keys = np.random.default_rng(200 + r).integers(0, spans[r], n, dtype=np.uint64).astype(np.uint32)
        for m in (ko1, vo1, kth1, ko2, vo2, kth2):
            m.fill()
        ki.put(keys)
        vi.put(vals)
        want = keys, topk("smallest", "input", keys, k1), topk("largest", "sorted", keys, k2)
        seen.add((int(want[1][1][0]), int(want[2][1][0])))
        return want

    def one(which, order, ko, vo, kth, k, ws):
        return lambda: lib.clo_hip_topk(which, order, ki.ptr, vi.ptr if valued else None, ko.ptr, vo.ptr if vs else None, kth.ptr, n, k,
                                        4, 0, vs, ws.ptr, need, q.stream)

    def enqueue():
        return GC.first(one(0, 0, ko1, vo1, kth1, k1, ws1), one(1, 1, ko2, vo2, kth2, k2, ws2))

    def verify(r, want):
        keys = want[0]
        for (p, kth_want), ko, vo, kth, k, name in ((want[1], ko1, vo1, kth1, k1, "smallest input"), (want[2], ko2, vo2, kth2, k2, "largest sorted")):
            tag = "%s %s round %d" % (name, mode, r)
            GC.same(kth.get(np.uint32, 1), kth_want, tag + ": kth_out")
            GC.same(ko.get(np.uint32, k), keys[p], tag + ": keys_out")
            GC.same(vo.get(np.uint32, k), (vals[p] if valued else p) if vs else GC.canary(np.uint32, k), tag + ": values_out")
        GC.same(ki.get(np.uint32, n), keys, "keys_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(seen) >= 4, seen                                     # the k-th keys differed between the replays
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


_DISTRIBUTIONS = ("uniform", "two values", "one byte used", "sorted", "reversed")


def fuzz_keys(rng, kt, n, dist):
    dt = np.dtype(_NP[kt])
    ut = np.dtype("u%d" % dt.itemsize)
    full = rng.integers(0, 1 << 63, n, dtype=np.uint64).astype(ut) ^ (rng.integers(0, 2, n).astype(ut) << ut.type(8 * dt.itemsize - 1))
    if dist == "two values":
        keys = full[:2][rng.integers(0, min(2, n), n)]
    elif dist == "one byte used":
        shift = 8 * int(rng.integers(0, dt.itemsize))
        keys = (full & ut.type(0xFF << shift)) | (full[:1] & ut.type(~(0xFF << shift) & ((1 << 8 * dt.itemsize) - 1)) if n else full)
    else:
        keys = full
    keys = keys.view(dt)
    if dist in ("sorted", "reversed"):
        keys = sort_keys(keys)
        if dist == "reversed":
            keys = keys[::-1]
    return np.ascontiguousarray(keys)


@pytest.mark.parametrize("chunk", range(4))
def test_seeded_fuzz(dev, chunk):
    """75 cases per chunk over n <= 6 T, k, direction, order, key type, value form and key distribution; the seed and the
    case are in every failure message."""
    seed = 20240 + chunk
    rng = np.random.default_rng(seed)
    for case in range(75):
        kt = KEY_TYPES[int(rng.integers(0, len(KEY_TYPES)))]
        mode = (MODES + ("kth_only",))[int(rng.integers(0, 6))]
        which, order = WHICH[int(rng.integers(0, 2))], ORDERS[int(rng.integers(0, 2))]
        T, S = tile_of(dev, kt, mode), cap_of(dev, kt, mode)
        n = int(rng.integers(1, 6 * T + 1)) if rng.random() < 0.7 else int(rng.integers(1, 200))
        dist = _DISTRIBUTIONS[int(rng.integers(0, 5))]
        k = int((1, 2, n // 2 + 1, n - 1, n, n + 1, int(rng.integers(1, n + 1)), int(rng.integers(1, n + 1)))[int(rng.integers(0, 8))])
        k = max(k, 1)
        if order == "sorted" and min(k, n) > S:
            k = int(rng.integers(1, S + 1))
        keys = fuzz_keys(rng, kt, n, dist)
        run_topk(dev, which, order, kt, keys, k, mode, "fuzz seed %d case %d, %s" % (seed, case, dist), kth=bool(rng.integers(0, 2)))


def test_indices_above_2p31(dev):
    """numel = 2^31 + T + 5 uchar keys, the 1000 smallest in arg form: about 1200 winners (values 0 .. 9, so that the
    cut falls inside a tie run) are planted among keys of 100 and more, at places that include the first element, both
    sides of index 2^31 and the last element. The expected rows are computed from the planted places alone."""
    import torch
    clo, ctx, q = dev
    T = tile_of(dev, "uchar", "arg_only")
    n, k = (1 << 31) + T + 5, 1000
    free = torch.cuda.mem_get_info()[0]
    if free < (6 << 30):
        pytest.skip("needs about 4 GiB of free device memory (2 GiB of keys, torch's scratch), %.1f GiB are free" % (free / 2 ** 30))
    g = torch.Generator(device="cuda").manual_seed(31)
    keys = torch.empty(n, dtype=torch.uint8, device="cuda").random_(100, 256, generator=g)
    near = torch.arange(-40, 40, dtype=torch.int64, device="cuda") * 3 + (1 << 31)
    planted = torch.cat((torch.randint(0, n, (1100,), dtype=torch.int64, device="cuda", generator=g), near,
                         torch.tensor([0, (1 << 31) - 1, 1 << 31, n - 1], dtype=torch.int64, device="cuda")))
    planted = torch.unique(planted)
    value = (planted * 7 + planted // 1000) % 10
    keys[planted] = value.to(torch.uint8)
    out = torch.full((k + 16,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")                          # bytes C3 C3 C3 C3
    kth = torch.full((4,), 0xC3, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    pos, val = planted.cpu().numpy(), value.cpu().numpy()
    assert pos.size > k
    chosen = np.lexsort((pos, val))[:k]
    want = np.sort(pos[chosen])
    assert (want < (1 << 31)).any() and (want >= (1 << 31)).any()
    as_buffer = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
    bufs = [as_buffer(keys), clo.Buffer(ctx, 4 * k, device_ptr=out.data_ptr()), clo.Buffer(ctx, 1, device_ptr=kth.data_ptr())]
    s = clo.TopK("smallest", "input", ctx, "uchar", 4)
    try:
        assert s.with_device_data(q, bufs[0], None, None, bufs[1], bufs[2], n, k)
        q.finish()
        got = out[:k].to(torch.int64).cpu().numpy() & 0xFFFFFFFF                                        # the indices are uint
        assert np.array_equal(got, want), "the indices differ from the planted winners"
        assert int(kth[0]) == int(val[chosen[-1]]) and bool((kth[1:] == 0xC3).all())
        assert bool((out[k:] == -0x3C3C3C3D).all()), "rows >= k were written"
    finally:
        for x in bufs + [s]:
            x.close()
        del keys, out
        torch.cuda.empty_cache()


def test_indices_above_2p31_largest_with_keys_out(dev):
    """The sibling in the other direction and with keys_out: numel = 2^31 + T + 5 ushort keys, the 1000 largest in input
    order with their indices. The losers are below 1000; about 1200 winners (60000 .. 60009, so that the cut falls
    inside a tie run) are planted at places that include the first element, both sides of index 2^31 and the last
    element, those four with the largest value, so that they are chosen. keys_out's row offsets pass 2^31 elements of input, the compacted rows come from tiles on both sides.
    The expected rows are computed from the planted places alone. (The keys are held as torch.int16: the bits count.)"""
    import torch
    clo, ctx, q = dev
    T = tile_of(dev, "ushort", "arg")
    n, k = (1 << 31) + T + 5, 1000
    free = torch.cuda.mem_get_info()[0]
    if free < (10 << 30):
        pytest.skip("needs about 8 GiB of free device memory (4 GiB of keys, torch's scratch), %.1f GiB are free" % (free / 2 ** 30))
    g = torch.Generator(device="cuda").manual_seed(32)
    keys = torch.empty(n, dtype=torch.int16, device="cuda").random_(0, 1000, generator=g)
    near = torch.arange(-40, 40, dtype=torch.int64, device="cuda") * 3 + (1 << 31)
    planted = torch.cat((torch.randint(0, n, (1100,), dtype=torch.int64, device="cuda", generator=g), near,
                         torch.tensor([0, (1 << 31) - 1, 1 << 31, n - 1], dtype=torch.int64, device="cuda")))
    planted = torch.unique(planted)
    ends = torch.tensor([0, (1 << 31) - 1, 1 << 31, n - 1], dtype=torch.int64, device="cuda")
    value = torch.where(torch.isin(planted, ends), 60009, 60000 + (planted * 7 + planted // 1000) % 10)   # the four ends are chosen
    keys[planted] = (value - 65536).to(torch.int16)                                                     # the bits of 60000 .. 60009
    rows = torch.full((k + 16,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")                         # bytes C3 C3 C3 C3
    kout = torch.full((k + 16,), -0x3C3D, dtype=torch.int16, device="cuda")
    kth = torch.full((4,), -0x3C3D, dtype=torch.int16, device="cuda")
    torch.cuda.synchronize()
    pos, val = planted.cpu().numpy(), value.cpu().numpy()
    assert pos.size > k
    chosen = np.lexsort((pos, -val))[:k]                                                                # the largest first, ties by index
    cut = int(val[chosen[-1]])
    assert int((val[chosen] == cut).sum()) < int((val == cut).sum())                                    # the cut falls inside a tie run
    in_order = np.sort(chosen)                                                                          # (pos is ascending)
    want, want_keys = pos[in_order], val[in_order].astype(np.uint16)
    assert want[0] == 0 and want[-1] == n - 1 and {(1 << 31) - 1, 1 << 31} <= set(want.tolist())
    bufs = [clo.Buffer(ctx, 2 * n, device_ptr=keys.data_ptr()), clo.Buffer(ctx, 2 * k, device_ptr=kout.data_ptr()),
            clo.Buffer(ctx, 4 * k, device_ptr=rows.data_ptr()), clo.Buffer(ctx, 2, device_ptr=kth.data_ptr())]
    s = clo.TopK("largest", "input", ctx, "ushort", 4)
    try:
        assert s.with_device_data(q, bufs[0], None, bufs[1], bufs[2], bufs[3], n, k)
        q.finish()
        got = rows[:k].to(torch.int64).cpu().numpy() & 0xFFFFFFFF                                       # the indices are uint
        got_keys, got_kth = kout.cpu().numpy().view(np.uint16), kth.cpu().numpy().view(np.uint16)
        assert np.array_equal(got, want), "the indices differ from the planted winners"
        assert np.array_equal(got_keys[:k], want_keys), "keys_out differs from the planted winners"
        assert int(got_kth[0]) == cut and bool((got_kth[1:] == 0xC3C3).all())
        assert bool((got_keys[k:] == 0xC3C3).all()) and bool((rows[k:] == -0x3C3C3C3D).all().item()), "rows >= k were written"
        assert keys[planted].to(torch.int64).cpu().numpy().tolist() == (val - 65536).tolist() and int(keys.max()) < 1000, "keys_in changed"
    finally:
        for x in bufs + [s]:
            x.close()
        del keys, rows, kout
        torch.cuda.empty_cache()
