"""CloJoin (include/clo_join.h) on the GPU against the numpy model of tests/join_model.py, bit for bit. Every array is a
view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs and num_out are pre-filled with the pattern, and after every call num_out is the
model's K, the first min(K, capacity) rows of idx_a_out, idx_b_out and keys_out equal the model's, and the guards, every
input and every entry beyond those rows are unchanged. With T = clo_hip_join_tile and R = clo_hip_join_out_tile: sizes
around the tile edges for every kind, one key m times in A and n times in B (rows that many work-groups write), long
stretches of A without a match, equal, disjoint and stacked inputs, capacities around K and around an output tile, the
count form, K above 2^32, every key type with its special values, element-aligned views, one object used large ->
small -> large, a seeded fuzz, identities with the library's own search and merge as second oracles, unsorted inputs
(the bounds contract only), the host-data form, the thin ABI's status codes, and clo_hip_join captured into a graph and
replayed on inputs that change K."""
import numpy as np
import pytest

from join_model import KINDS, NONE, join, max_rows
from merge_model import merge, sort_keys
from test_gpu_histogram import Region
from test_gpu_merge import KEY_TYPES, _NP, guards_intact, keys_of_type

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def tile_of(dev, kt):
    t = dev[0].join_tile(np.dtype(_NP[kt]).itemsize)
    assert t > 0 and t % 64 == 0
    return t


def read_num(q, num_r):
    return int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])


def run_join(dev, kind, kt, a, b, what, capacity=None, offs=(0, 0, 0, 0, 0), obj=None, compare=True, outs=(True, True, True)):
    """One call on views at byte offsets offs = (keys_a, keys_b, idx_a_out, idx_b_out, keys_out); checks everything and
    returns K. capacity None: K + 3 rows, so that there are entries beyond the result. outs: which of idx_a_out,
    idx_b_out, keys_out are given; none of them with capacity 0 is the count form. compare False (unsorted inputs):
    success, guards, inputs, nothing beyond min(K, capacity), and every index below its side's numel or NONE."""
    clo, ctx, q = dev
    dt = np.dtype(_NP[kt])
    a, b = np.ascontiguousarray(a, dtype=dt), np.ascontiguousarray(b, dtype=dt)
    na, nb = a.size, b.size
    what = "%s, %s" % (kind, what)
    if capacity is None:
        capacity = (join(kind, a, b, capacity=0)[3] if compare else max_rows(kind, na, nb)) + 3
    j = obj or clo.Join(kind, ctx, kt)
    assert j.max_numel_out(na, nb) == max_rows(kind, na, nb)
    ka_r, kb_r = Region(dev, a.nbytes, offs[0], a, 0), Region(dev, b.nbytes, offs[1], b, 1)
    ia_r = Region(dev, capacity * 4, offs[2], None, 2) if outs[0] else None
    ib_r = Region(dev, capacity * 4, offs[3], None, 1) if outs[1] else None
    ko_r = Region(dev, capacity * dt.itemsize, offs[4], None, 2) if outs[2] else None
    num_r = Region(dev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert j.with_device_data(q, ka_r.view if na else None, na, kb_r.view if nb else None, nb,
                                  view(ia_r), view(ib_r), view(ko_r), capacity, num_r.view), what
        q.finish()
        k = read_num(q, num_r)
        num_r.check(np.array([k], np.uint64), what + ": num_out")
        if compare:
            ia, ib, keys, K = join(kind, a, b, capacity=capacity)
            assert k == K, "%s: num_out = %d, the model has %d rows" % (what, k, K)
            for r, want, name in ((ia_r, ia, "idx_a_out"), (ib_r, ib, "idx_b_out"), (ko_r, keys, "keys_out")):
                if r:
                    r.check(want, "%s: %s (capacity %d, K %d)" % (what, name, capacity, K))   # ... and nothing beyond
        else:
            rows = min(k, capacity)
            for r, numel, width in ((ia_r, na, 4), (ib_r, nb, 4), (ko_r, None, dt.itemsize)):
                if not r:
                    continue
                guards_intact(r, what)
                got = r.base.read(q, np.uint8, r.host.size)[r.at:r.at + r.n]
                assert np.array_equal(got[rows * width:], r.host[r.at + rows * width:r.at + r.n]), what + ": written beyond min(K, capacity)"
                if numel is not None:
                    idx = got[:rows * 4].view(np.uint32)
                    assert ((idx < numel) | (idx == NONE)).all(), what + ": an index neither below numel nor NONE"
        ka_r.check(a, what + ": keys_a")
        kb_r.check(b, what + ": keys_b")
        return k
    finally:
        for r in (ka_r, kb_r, ia_r, ib_r, ko_r, num_r):
            if r:
                r.close()
        if obj is None:
            j.close()


def shared_keys(na, nb, seed):
    """Ascending uint keys, about one in four of them in both inputs, with some duplicates on either side."""
    rng = np.random.default_rng(seed)
    pool = np.sort(rng.choice(4 * (na + nb) + 8, size=na + nb + 2, replace=False)).astype(np.uint32)
    both = pool[rng.random(pool.size) < 0.25]
    only_a, only_b = pool[::2], pool[1::2]
    draw = lambda n, own: np.sort(rng.choice(np.concatenate((own, both, both)), size=n)) if n else np.zeros(0, np.uint32)
    return draw(na, only_a).astype(np.uint32), draw(nb, only_b).astype(np.uint32)


@pytest.mark.parametrize("kind", KINDS)
def test_sizes_around_the_tile_edges(dev, kind):
    clo, ctx, q = dev
    T = tile_of(dev, "uint")
    sizes = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)
    obj = clo.Join(kind, ctx, "uint")
    for na in sizes:
        for nb in sizes:
            a, b = shared_keys(na, nb, na * 31 + nb)
            run_join(dev, kind, "uint", a, b, "%d and %d" % (na, nb), obj=obj, outs=(True, True, (na + nb) % 2 == 0))
    obj.close()


def runs(*parts):
    return np.concatenate([np.full(c, k, np.uint32) for k, c in parts] + [np.zeros(0, np.uint32)])


@pytest.mark.parametrize("kind", KINDS)
def test_one_key_m_times_n(dev, kind):
    """One key m times in A and n times in B: m * n rows, written by more work-groups than the key has input tiles, the
    run bounds found outside the tile. Alone, behind smaller unmatched keys (the runs start mid-tile, at different places
    in A and in B), and two such runs back to back."""
    T = tile_of(dev, "uint")
    for m, n in ((3 * T + 5, 2), (2, 3 * T + 5), (2 * T + 1, 3), (1, 8 * T + 1), (T // 8, T // 8)):
        tag = "a key %d times in A and %d times in B" % (m, n)
        run_join(dev, kind, "uint", runs((7, m)), runs((7, n)), tag)
        run_join(dev, kind, "uint", runs((1, 3), (2, 1), (4, 37), (7, m)), runs((2, 2), (3, 70), (7, n)), tag + " behind smaller keys")
        run_join(dev, kind, "uint", runs((5, 11), (7, m), (9, n), (12, 4)), runs((7, n), (9, m), (11, 1)), tag + " and the reverse behind it")


@pytest.mark.parametrize("kind", KINDS)
def test_long_stretches_without_a_match(dev, kind):
    """>= 3 T rows of A without a partner between matched ones: elements that emit no row (inner, right) and leave no
    entry in the table, so that one output tile's emitters lie many merged tiles apart, or that emit one row each (left,
    full); the same for B; and a stretch several output tiles long."""
    T = tile_of(dev, "uint")
    R = dev[0].join_out_tile()
    gap = np.arange(3 * T + 7, dtype=np.uint32) * 2 + 101                  # odd keys
    a = np.concatenate((runs((10, 40)), gap, runs((2 * gap[-1] + 2, 3)), gap + np.uint32(2 * gap[-1] + 10), runs((8 * gap[-1], 50))))
    b = np.concatenate((runs((10, 70)), runs((2 * gap[-1] + 2, R + 5)), runs((8 * gap[-1], 90))))
    run_join(dev, kind, "uint", a, b, "two stretches of %d in A" % gap.size)
    run_join(dev, kind, "uint", b, a, "two stretches of %d in B" % gap.size)
    long_gap = np.arange(5 * R + 9, dtype=np.uint32) * 2 + 101             # five output tiles of single rows, or none at all
    a = np.concatenate((runs((10, 40)), long_gap, runs((4 * long_gap[-1], 50))))
    b = np.concatenate((runs((10, 70)), runs((4 * long_gap[-1], 90))))
    run_join(dev, kind, "uint", a, b, "a stretch of %d in A" % long_gap.size)
    run_join(dev, kind, "uint", b, a, "a stretch of %d in B" % long_gap.size)


@pytest.mark.parametrize("kind", KINDS)
def test_extreme_overlaps(dev, kind):
    clo, ctx, q = dev
    T = tile_of(dev, "uint")
    u = lambda x: np.asarray(x, dtype=np.uint32)
    same = u(np.arange(2 * T + 3))
    low, high = u(np.arange(2 * T + 3)), u(np.arange(T + 1) + 10 * T)
    even, odd = u(2 * np.arange(T + 40)), u(2 * np.arange(T + 41) + 1)
    assert run_join(dev, kind, "uint", same, same, "A == B without duplicates") == same.size
    for a, b, name in ((low, high, "A entirely below B"), (high, low, "B entirely below A"), (even, odd, "disjoint, interleaved")):
        k = run_join(dev, kind, "uint", a, b, name)
        assert k == {"inner": 0, "left": a.size, "right": b.size, "full": a.size + b.size}[kind], (kind, name, k)
    # the full join of disjoint inputs IS the argmerge, with NONE on the other side
    if kind == "full":
        ia, ib, keys, K = join("full", even, odd)
        want_keys, p = merge(even, odd)
        assert np.array_equal(keys, want_keys)
        assert np.array_equal(np.where(ia != NONE, ia, ib + np.uint32(even.size)), p) and ((ia == NONE) != (ib == NONE)).all()
        m = clo.Merge(ctx, "uint", 4)
        got_keys, got_p = m.with_host_data(even, odd, q_exec=q)
        m.close()
        assert np.array_equal(got_keys, keys) and np.array_equal(got_p, p)


def three_output_tiles(dev):
    R = dev[0].join_out_tile()
    a = np.repeat(np.arange(0, 3 * R // 8 + 5, dtype=np.uint32) * 3, 2)       # pairs of A against fours of B, some keys alone
    b = np.repeat(np.arange(0, 3 * R // 8 + 9, dtype=np.uint32) * 3, 4)
    a = np.sort(np.concatenate((a, np.arange(40, dtype=np.uint32) * 3 + 1)))
    b = np.sort(np.concatenate((b, np.arange(50, dtype=np.uint32) * 3 + 2)))
    return a, b, R


@pytest.mark.parametrize("kind", KINDS)
def test_capacities_around_k_and_an_output_tile(dev, kind):
    a, b, R = three_output_tiles(dev)
    K = join(kind, a, b, capacity=0)[3]
    assert 3 * R <= K < 4 * R, K
    for cap in (0, 1, K - 1, K, K + 1, R - 1, R, R + 1):
        assert run_join(dev, kind, "uint", a, b, "capacity %d of %d" % (cap, K), capacity=cap) == K
    assert run_join(dev, kind, "uint", a, b, "idx_b_out alone", capacity=K, outs=(False, True, False)) == K
    assert run_join(dev, kind, "uint", a, b, "keys_out alone", capacity=R + 1, outs=(False, False, True)) == K


@pytest.mark.parametrize("kind", KINDS)
def test_count_form(dev, kind):
    a, b, R = three_output_tiles(dev)
    K = join(kind, a, b, capacity=0)[3]
    assert run_join(dev, kind, "uint", a, b, "the count form", capacity=0, outs=(False, False, False)) == K
    assert run_join(dev, kind, "uint", a, b[:0], "the count form, B empty", capacity=0, outs=(False, False, False)) == (a.size if kind in ("left", "full") else 0)
    assert run_join(dev, kind, "uint", a[:0], b, "the count form, A empty", capacity=0, outs=(False, False, False)) == (b.size if kind in ("right", "full") else 0)


@pytest.mark.parametrize("kind", KINDS)
def test_k_above_2_to_the_32(dev, kind):
    m = 65537
    k = run_join(dev, kind, "uint", np.full(m, 7, np.uint32), np.full(m, 7, np.uint32), "65 537 x 65 537", capacity=1024)
    assert k == 2 ** 32 + 2 ** 17 + 1


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types(dev, kt):
    T = tile_of(dev, kt)
    a, b = keys_of_type(kt, T + 1, 5), keys_of_type(kt, 2 * T + 3, 6)      # few distinct keys, the type's specials: long runs
    cap = 3 * dev[0].join_out_tile() + 5                                    # the products of such runs are large: a prefix
    for i, kind in enumerate(KINDS):
        run_join(dev, kind, kt, a, b, kt, capacity=cap)
        run_join(dev, kind, kt, b[::7], a[::5], kt + ", thinned and reversed", capacity=cap + i)
    dt = np.dtype(_NP[kt])
    r = np.random.default_rng(7)
    span = min(4 * T, 1 << (8 * dt.itemsize - 1))
    draw = lambda n: sort_keys((r.integers(0, span, n) - span // 2).astype(np.int64).astype(dt) if dt.kind != "f" else (r.integers(0, span, n) - span // 2).astype(dt))
    for kind in KINDS:
        run_join(dev, kind, kt, draw(T + 9), draw(T // 2), kt + ", mostly distinct", capacity=cap)


def test_element_aligned_views(dev):
    """Views at odd element offsets inside their allocations: nothing may assume 16-byte alignment."""
    R = dev[0].join_out_tile()
    for i, (kt, offs) in enumerate((("uchar", (1, 3, 4, 12, 5)), ("char", (13, 2, 8, 4, 1)), ("ushort", (2, 6, 4, 8, 10)), ("uint", (4, 12, 8, 4, 4)),
                                    ("float", (4, 8, 12, 4, 8)), ("ulong", (8, 8, 4, 12, 8)), ("double", (8, 8, 12, 8, 8)))):
        T = tile_of(dev, kt)
        a, b = keys_of_type(kt, T + 37, 8), keys_of_type(kt, 2 * T + 3, 9)
        for kind in (KINDS[i % 4], KINDS[(i + 1) % 4]):
            run_join(dev, kind, kt, a[::3], b[::2], "%s at %s" % (kt, offs), capacity=2 * R + 3, offs=offs)


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "uint")
    for kind in ("inner", "full"):
        j = clo.Join(kind, ctx, "uint")
        for k, (na, nb) in enumerate(((40 * T + 3, 25 * T + 1), (5, 9), (0, 3), (60 * T + 7, 11), (3 * T, 3 * T))):
            a, b = shared_keys(na, nb, k)
            run_join(dev, kind, "uint", a, b, "call %d" % k, obj=j)
        j.close()


def test_seeded_fuzz(dev):
    """A hundred cases over kinds, key types, sizes, duplicate structure and capacity; a failure names its case."""
    rng = np.random.default_rng(20241021)
    R = dev[0].join_out_tile()
    for case in range(100):
        kind, kt = KINDS[rng.integers(4)], KEY_TYPES[rng.integers(len(KEY_TYPES))]
        T = tile_of(dev, kt)
        na, nb = (int(rng.integers(0, 3 * T)) if rng.integers(8) else 0 for _ in range(2))
        mix = ("specials", "short runs", "long runs", "mostly distinct")[rng.integers(4)]
        seed = int(rng.integers(1 << 30))
        if mix == "specials":
            a, b = keys_of_type(kt, na, seed), keys_of_type(kt, nb, seed + 1)
        else:
            dt = np.dtype(_NP[kt])
            distinct = {"short runs": max(2, (na + nb) // 4), "long runs": 3, "mostly distinct": 4 * (na + nb) + 2}[mix]
            distinct = min(distinct, 1 << (8 * dt.itemsize - 1))
            r = np.random.default_rng(seed)
            draw = lambda n: sort_keys((r.integers(0, distinct, n) - distinct // 2).astype(np.int64).astype(dt) if dt.kind != "f"
                                       else (r.integers(0, distinct, n) - distinct // 2).astype(dt))
            a, b = draw(na), draw(nb)
        K = join(kind, a, b, capacity=0)[3]
        cap = (0, 1, max(K - 1, 0), K, K + 1, R, 2 * R + 1, int(rng.integers(0, K + 2)))[rng.integers(8)]
        cap = min(cap, 6 * R)
        outs = tuple(bool(x) for x in rng.integers(0, 2, 3))
        if cap > 0 and not any(outs):
            outs = (True, False, False)
        run_join(dev, kind, kt, a, b, "fuzz case %d: %s %s %d and %d, capacity %d (seed %d)" % (case, kt, mix, na, nb, cap, seed), capacity=cap, outs=outs)


def test_identities_with_the_librarys_own_search(dev):
    """Second oracles that share nothing with the model: the columns of an inner join index equal keys; |left| = |inner|
    + the rows of A whose lower and upper bounds in B from CloSearch are equal; keys_out is ascending."""
    clo, ctx, q = dev
    T = tile_of(dev, "float")
    a, b = keys_of_type("float", 3 * T + 11, 21)[::3], keys_of_type("float", 2 * T + 5, 22)[::2]
    r = np.random.default_rng(3)
    a = sort_keys(np.concatenate((a, r.integers(-500, 500, 2 * T).astype(np.float32))))
    b = sort_keys(np.concatenate((b, r.integers(-500, 500, T).astype(np.float32))))
    ji, jl, s = clo.Join("inner", ctx, "float"), clo.Join("left", ctx, "float"), clo.Search(ctx, "float")
    try:
        cap = 40 * dev[0].join_out_tile()
        ia, ib, keys, K = ji.with_host_data(a, b, capacity=cap, keys_out=True, q_exec=q)
        assert 0 < ia.size == min(K, cap)
        assert np.array_equal(a[ia].view(np.uint32), b[ib].view(np.uint32)) and np.array_equal(keys.view(np.uint32), a[ia].view(np.uint32))
        from merge_model import order_key
        assert (np.diff(order_key(keys).astype(np.int64)) >= 0).all()
        lo = s.with_host_data(b, a, upper=False, needles_sorted=True, q_exec=q)
        hi = s.with_host_data(b, a, upper=True, needles_sorted=True, q_exec=q)
        assert ji.count(a, b, q_exec=q) == K == int((hi.astype(np.int64) - lo).sum())
        assert jl.count(a, b, q_exec=q) == K + int((lo == hi).sum())
        la, lb_, lkeys, LK = jl.with_host_data(a, b, capacity=cap, keys_out=True, q_exec=q)
        assert (np.diff(order_key(lkeys).astype(np.int64)) >= 0).all()
    finally:
        for x in (ji, jl, s):
            x.close()


@pytest.mark.parametrize("layout", ["random", "descending", "runs out of place", "a long run broken up"])
def test_unsorted_inputs_stay_inside_their_arrays(dev, layout):
    """The bounds contract: the precondition is broken, K and the contents are unspecified and not compared; the call
    succeeds, the guards around the outputs and num_out are intact, nothing is written beyond min(K, capacity), every
    index written is below its side's numel or NONE, and the inputs are unchanged."""
    T = tile_of(dev, "uint")
    R = dev[0].join_out_tile()
    rng = np.random.default_rng(9)
    na, nb = 2 * T + 3, T + 1
    if layout == "random":
        a, b = rng.integers(0, 64, na).astype(np.uint32), rng.integers(0, 64, nb).astype(np.uint32)
    elif layout == "descending":
        a, b = np.arange(na, 0, -1, dtype=np.uint32), np.arange(nb, 0, -1, dtype=np.uint32) * 2
    elif layout == "runs out of place":   # equal keys everywhere but not together: every probe of a neighbour finds something equal somewhere
        a, b = (np.arange(na, dtype=np.uint32) % 3) * 5, (np.arange(nb, dtype=np.uint32) % 2) * 5
    else:
        na, nb = 3 * T, T
        a = np.full(na, 5, np.uint32)
        a[T] = a[2 * T] = 0
        b = np.concatenate((np.full(1, 5, np.uint32), np.full(T // 2 - 1, 9, np.uint32), np.full(T - T // 2, 5, np.uint32)))
    for kind in KINDS:
        for cap in (R + 1, 5 * R + 7):
            run_join(dev, kind, "uint", a, b, "%s, capacity %d" % (layout, cap), capacity=cap, compare=False)
        run_join(dev, kind, "uint", b[:64], a, "%s, a short A" % layout, capacity=3 * R, compare=False)
        run_join(dev, kind, "uint", a, b, "%s, the count form" % layout, capacity=0, outs=(False, False, False), compare=False)
        for kt in ("uchar", "double"):
            run_join(dev, kind, kt, a.astype(_NP[kt]), b.astype(_NP[kt]), "%s %s" % (layout, kt), capacity=2 * R + 1, compare=False)


@pytest.mark.parametrize("kind", KINDS)
def test_host_data_form(dev, kind):
    clo, ctx, q = dev
    T = tile_of(dev, "int")
    a, b = keys_of_type("int", T + 9, 1)[::4], keys_of_type("int", 2 * T + 1, 2)[::4]
    j = clo.Join(kind, ctx, "int")
    qc = clo.Queue(ctx)
    try:
        ia, ib, keys, K = join(kind, a, b)
        assert j.count(a, b, q_exec=q) == K
        for qe, qcomm in ((q, None), (q, qc), (None, None)):
            got = j.with_host_data(a, b, keys_out=True, q_exec=qe, q_comm=qcomm)      # capacity None: the count form first
            assert got[3] == K and np.array_equal(got[0], ia) and np.array_equal(got[1], ib) and np.array_equal(got[2], keys)
        for cap in (0, 5, K + 9):
            w = join(kind, a, b, capacity=cap)
            got = j.with_host_data(a, b, capacity=cap, q_exec=q)
            assert got[3] == K and got[2] is None and np.array_equal(got[0], w[0]) and np.array_equal(got[1], w[1]), cap
        # empty sides
        got = j.with_host_data(a, b[:0], q_exec=q)
        assert got[3] == (a.size if kind in ("left", "full") else 0) and (got[1] == NONE).all()
        got = j.with_host_data(a[:0], b, q_exec=q)
        assert got[3] == (b.size if kind in ("right", "full") else 0) and (got[0] == NONE).all()
        assert j.with_host_data(a[:0], b[:0], keys_out=True)[3] == 0
    finally:
        qc.close()
        j.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    n, cap = 1000, 5000
    need = lib.clo_hip_join_workspace_bytes(3, n, n)
    assert need > 0 and need % 256 == 0
    rng = np.random.default_rng(1)
    ka, kb = (Region(dev, 8 * n + 16, 0, np.concatenate((np.sort(rng.integers(0, n, n + 4).astype(np.uint32)), np.zeros(n, np.uint32))), i) for i in range(2))
    ia, ib = (Region(dev, 4 * cap + 16, 0, None, i) for i in range(2))
    ko = Region(dev, 8 * cap + 16, 0, None, 2)
    num = Region(dev, 16, 0, None, 0)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(ka_p, na, kb_p, nb, ia_p, ib_p, ko_p, capacity=cap, kind=3, num_p=num.ptr, ks=4, kk=0, w=ws.ptr, wb=need):
        return lib.clo_hip_join(kind, ka_p, na, kb_p, nb, ia_p, ib_p, ko_p, capacity, num_p, ks, kk, w, wb, s)

    try:
        full = (ka.ptr, n, kb.ptr, n, ia.ptr, ib.ptr, ko.ptr)
        for kind in (-1, 4, 100):
            assert call(*full, kind=kind) == EARGS
        for kk in (-1, 3):
            assert call(*full, kk=kk) == EARGS
        for ks, kk in ((3, 0), (16, 0), (0, 0), (1, 2)):
            assert call(*full, ks=ks, kk=kk) == EUNSUPPORTED, (ks, kk)
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(ka.ptr, (1 << 32) - n, kb.ptr, n, ia.ptr, ib.ptr, ko.ptr) == EARGS                    # n = 2^32
        assert call(ka.ptr, 1 << 32, kb.ptr, 0, ia.ptr, ib.ptr, ko.ptr) == EARGS
        assert call(*full, capacity=1 << 32) == EARGS
        assert call(None, n, kb.ptr, n, ia.ptr, ib.ptr, ko.ptr) == EARGS                                  # a missing array
        assert call(ka.ptr, n, None, n, ia.ptr, ib.ptr, ko.ptr) == EARGS
        assert call(ka.ptr, n, kb.ptr, n, None, None, None) == EARGS                                      # a capacity and no output
        for i in (0, 2, 4, 5, 6):                                                                       # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        q.finish()
        for r in (ia, ib, ko, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; the count form; 8-byte keys of kind 2 over the
        # same bytes; n 0 needs no workspace and still writes num_out
        first = lambda: read_num(q, num)
        a_keys, b_keys = ka.contents(np.uint32)[:n], kb.contents(np.uint32)[:n]
        for kind in range(4):
            assert call(*full, kind=kind, wb=lib.clo_hip_join_workspace_bytes(kind, n, n)) == 0
            q.finish()
            assert first() == join(KINDS[kind], a_keys, b_keys, capacity=0)[3]
        assert call(ka.ptr, n, kb.ptr, n, None, None, None, capacity=0, kind=0) == 0
        q.finish()
        assert first() == join("inner", a_keys, b_keys, capacity=0)[3]
        assert call(ka.ptr, n // 4, kb.ptr, n // 4, ia.ptr, None, ko.ptr, ks=8, kk=2) == 0
        q.finish()
        assert first() <= max_rows("full", n // 4, n // 4)
        assert call(None, 0, None, 0, ia.ptr, None, None, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (ka, kb, ia, ib, ko, num):
            r.close()


def test_getters(dev):
    from cl_ops_amd._hip import lib
    for ks in (1, 2, 4, 8):
        assert dev[0].join_tile(ks) % 256 == 0 and dev[0].join_tile(ks) > 0
    assert dev[0].join_tile(3) == 0 and dev[0].join_out_tile() % 256 == 0
    for kind in range(4):
        last = 0
        for n in (0, 1, 100, 5000, 10 ** 6):
            w = lib.clo_hip_join_workspace_bytes(kind, n, n // 2)
            assert (w == 0) == (n == 0) and w >= last and w % 256 == 0
            last = w


@pytest.mark.parametrize("kind", KINDS)
def test_graph_capture_and_replay(dev, kind):
    """clo_hip_join captured from a client stream after one eager warm-up and replayed three times on new contents of
    the same buffers, the outputs and num_out refilled with a canary before each (the protocol of
    test_gpu_graph_capture.py). The rounds' inputs overlap differently, so that K of the three replays (rounds 1 to 3)
    is different on every one of them for every kind, once above the capacity."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T = tile_of(dev, "uint")
    na, nb = 2 * T + 3, T + 1
    cap = 3 * (na + nb)
    need = lib.clo_hip_join_workspace_bytes(KINDS.index(kind), na, nb)
    made = [GC.Mem(gdev, x) for x in (4 * na, 4 * nb, 4 * cap, 4 * cap, 4 * cap, 8, need)]
    ka, kb, ia, ib, ko, num, ws = made
    kinds = ["uniform", "all equal", "A below B", "pairs and triples, some shared", "uniform"]
    sent, ks = {}, {}

    def load(k):
        rng = np.random.default_rng(100 + k)
        if kinds[k] == "uniform":
            a, b = np.sort(rng.integers(0, na, na).astype(np.uint32)), np.sort(rng.integers(0, na, nb).astype(np.uint32))
        elif kinds[k] == "all equal":
            a, b = np.full(na, 9 + k, np.uint32), np.full(nb, 9 + k, np.uint32)
        elif kinds[k] == "A below B":
            a, b = np.arange(na, dtype=np.uint32) + np.uint32(k), np.arange(nb, dtype=np.uint32) + np.uint32(na + 5)
        else:   # every key twice in A and three times in B, some keys of either side in the other
            a, b = np.arange(na, dtype=np.uint32) // np.uint32(2), (np.arange(nb, dtype=np.uint32) // np.uint32(3)) * np.uint32(5)
        sent[k] = (a, b)
        for m in (ia, ib, ko, num):
            m.fill()
        ka.put(a)
        kb.put(b)
        want = join(kind, a, b, capacity=cap)
        ks[k] = want[3]
        return want

    def enqueue():
        return lib.clo_hip_join(KINDS.index(kind), ka.ptr, na, kb.ptr, nb, ia.ptr, ib.ptr, ko.ptr, cap, num.ptr, 4, 0, ws.ptr, need, q.stream)

    def verify(k, want):
        tag = "%s round %d (%s)" % (kind, k, kinds[k])
        assert int(num.get(np.uint64, 1)[0]) == want[3], tag + ": num_out"
        rest = GC.canary(np.uint32, cap - want[0].size)
        for m, w, name in ((ia, want[0], "idx_a_out"), (ib, want[1], "idx_b_out"), (ko, want[2], "keys_out")):
            GC.same(m.get(np.uint32, cap), np.concatenate((w, rest)), tag + ": " + name)
        GC.same(ka.get(np.uint32, na), sent[k][0], tag + ": keys_a")
        GC.same(kb.get(np.uint32, nb), sent[k][1], tag + ": keys_b")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        replayed = [ks[k] for k in (1, 2, 3)]
        assert len(set(replayed)) == 3 and max(replayed) > cap, ks             # K differed on every replay
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()
