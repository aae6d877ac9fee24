"""CloSetOp (include/clo_setop.h) on the GPU against the numpy model of tests/setop_model.py, bit for bit. Every array
is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs and num_out are pre-filled with the pattern, and after every call num_out is the
model's k, the first k rows equal the model's, and the guards, every input and every entry at index >= k are unchanged.
With T = clo_hip_setop_tile: sizes around the tile edges for every op and value mode, runs of one key longer than
tiles (in A, in B, in both, starting mid-tile, two back to back), extreme overlaps and empty results, tile counts around
the widths of the count scan and more tiles than the chip holds, every key type with its special values,
element-aligned views, one object used large -> small -> large, a seeded fuzz, identities with the library's own merge
as a second oracle, unsorted inputs (the bounds contract only), the host-data form, the thin ABI's status codes, and
clo_hip_setop captured into a graph and replayed on inputs that change k."""
import numpy as np
import pytest

from merge_model import sort_keys
from setop_model import OPS, capacity, setop
from test_gpu_histogram import Region
from test_gpu_merge import KEY_TYPES, _NP, _VS, guards_intact, keys_of_type, sorted_uint, values_for

pytestmark = pytest.mark.gpu

SCAN_SWEEP = 256 * 8   # counts per sweep of the one-group scan (clo_hip_setop.hip: SETOP_THREADS * SETOP_SCAN_ITEMS)


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def tile_of(dev, kt, mode="keys"):
    t = dev[0].setop_tile(np.dtype(_NP[kt]).itemsize, _VS[mode])
    assert t > 0 and t % 64 == 0
    return t


def keeps_b(op):
    return op in ("union", "symmetric_difference")


def run_setop(dev, op, kt, a, b, mode, what, offs=(0, 0, 0, 0, 0, 0), obj=None, compare=True, pass_vb=True):
    """One call on views at byte offsets offs = (keys_a, values_a, keys_b, values_b, keys_out, values_out); checks
    everything and returns k. compare False (unsorted inputs): success, guards, inputs and k <= capacity only.
    pass_vb False: values_b is NULL (intersection and difference never look at it)."""
    clo, ctx, q = dev
    dt = np.dtype(_NP[kt])
    a, b = np.ascontiguousarray(a, dtype=dt), np.ascontiguousarray(b, dtype=dt)
    na, nb, vs = a.size, b.size, _VS[mode]
    cap = capacity(op, na, nb)
    what = "%s, %s" % (op, what)
    va, vb = values_for(mode, na, nb)
    s = obj or clo.SetOp(op, ctx, kt, vs)
    assert s.max_numel_out(na, nb) == cap
    ka_r, kb_r = Region(dev, a.nbytes, offs[0], a, 0), Region(dev, b.nbytes, offs[2], b, 1)
    va_r = Region(dev, va.nbytes, offs[1], va, 1) if va is not None else None
    vb_r = Region(dev, vb.nbytes, offs[3], vb, 0) if vb is not None and (pass_vb or keeps_b(op)) else None
    ko_r = Region(dev, cap * dt.itemsize, offs[4], None, 2) if mode != "arg_only" else None
    vo_r = Region(dev, cap * vs, offs[5], None, 2) if vs else None
    num_r = Region(dev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert s.with_device_data(q, ka_r.view if na else None, view(va_r) if na else None, na, kb_r.view if nb else None,
                                  view(vb_r) if nb else None, nb, view(ko_r), view(vo_r), num_r.view), what
        q.finish()
        k = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        num_r.check(np.array([k], np.uint64), what + ": num_out")
        assert k <= cap, "%s: k = %d above the capacity %d" % (what, k, cap)
        if compare:
            want_k, p = setop(op, a, b)
            assert k == p.size, "%s: k = %d, the model keeps %d" % (what, k, p.size)
            if ko_r:
                ko_r.check(want_k, what + ": keys_out")                # ... and nothing at index >= k
            if vo_r:
                vo_r.check(np.concatenate((va, vb))[p] if va is not None else p, what + ": values_out")
        else:
            for r in (ko_r, vo_r):
                if r:
                    guards_intact(r, what)
        ka_r.check(a, what + ": keys_a")
        kb_r.check(b, what + ": keys_b")
        if va_r:
            va_r.check(va, what + ": values_a")
        if vb_r:
            vb_r.check(vb, what + ": values_b")
        return k
    finally:
        for r in (ka_r, kb_r, va_r, vb_r, ko_r, vo_r, num_r):
            if r:
                r.close()
        if obj is None:
            s.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "arg"])
@pytest.mark.parametrize("op", OPS)
def test_sizes_around_the_tile_edges(dev, op, mode):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", mode)
    sizes = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)
    obj = clo.SetOp(op, ctx, "uint", _VS[mode])
    for na in sizes:
        for nb in sizes:
            span = max(4, (na + nb) // 3)                              # runs of about three, in A and in B
            run_setop(dev, op, "uint", sorted_uint(na, na * 31 + nb, span), sorted_uint(nb, nb * 17 + na + 1, span), mode,
                      "%s %d + %d" % (mode, na, nb), obj=obj, pass_vb=(na + nb) % 2 == 0)
    obj.close()


def runs(*parts):
    return np.concatenate([np.full(c, k, np.uint32) for k, c in parts] + [np.zeros(0, np.uint32)])


@pytest.mark.parametrize("op", OPS)
def test_runs_longer_than_tiles(dev, op):
    """One key m times in A and n times in B: the rank of an element and the other run's length come from outside the
    tile. Alone, behind a few smaller keys (the run starts mid-tile, at different places in A and in B), and two such
    runs back to back (a tile's first and last key are both long runs)."""
    T = tile_of(dev, "uint", "arg")
    for m, n in ((3 * T + 5, T // 2), (T // 2, 3 * T + 5), (2 * T, 2 * T), (2 * T + 1, 2 * T), (0, 3 * T), (3 * T, 0)):
        tag = "run of %d in A and %d in B" % (m, n)
        run_setop(dev, op, "uint", runs((7, m)), runs((7, n)), "arg", tag)
        run_setop(dev, op, "uint", runs((1, 3), (2, 1), (4, 37), (7, m)), runs((2, 2), (3, 70), (7, n)), "v4", tag + " behind smaller keys")
        run_setop(dev, op, "uint", runs((5, 11), (7, m), (9, n), (12, 4)), runs((7, n), (9, m), (11, 1)), "arg", tag + " and the reverse behind it")


@pytest.mark.parametrize("op", OPS)
def test_extreme_overlaps(dev, op):
    T = tile_of(dev, "uint", "v4")
    u = lambda x: np.asarray(x, dtype=np.uint32)
    same = sorted_uint(2 * T + 3, 4)
    cases = {
        "A == B": (same, same),
        "A == B, no duplicates": (np.arange(2 * T + 3), np.arange(2 * T + 3)),
        "A below B": (np.arange(2 * T + 3), np.arange(T + 1) + 10 * T),
        "B below A": (np.arange(T + 1) + 10 * T, np.arange(2 * T + 3)),
        "interleaved": (2 * np.arange(T + 40), 2 * np.arange(T + 41) + 1),
        "5 of A inside 3 T of B": ([T // 2, T - 1, T, 2 * T + 1, 5 * T], np.arange(3 * T)),
        "5 of B inside 3 T of A": (np.arange(3 * T), [0, T - 1, T, T, 2 * T]),
        "A a subset of B": (np.arange(T + 7) * 3, np.arange(3 * T + 21)),
    }
    for name, (a, b) in cases.items():
        for mode in ("v4", "arg_only"):
            k = run_setop(dev, op, "uint", u(a), u(b), mode, "%s, %s" % (name, mode))
        # outputs of length 0: k = 0 and (run_setop checked it) nothing written
        if (op == "intersection" and name in ("A below B", "B below A", "interleaved")) or \
                (op in ("difference", "symmetric_difference") and name.startswith("A == B")) or (op == "difference" and name == "A a subset of B"):
            assert k == 0, (op, name, k)


@pytest.mark.parametrize("tiles", [255, 256, 257, SCAN_SWEEP - 1, SCAN_SWEEP, SCAN_SWEEP + 1, 2 * SCAN_SWEEP + 5])
def test_tile_counts_of_the_count_scan(dev, tiles):
    """Around the scan's work-group size and its sweep (the carry from sweep to sweep), and beyond two sweeps: more
    tiles than the chip holds at once (256 compute units of at most 8 work-groups)."""
    T = tile_of(dev, "uint", "arg")
    n = (tiles - 1) * T + 5
    na = n // 2 + 3
    rng = np.random.default_rng(tiles)
    a = np.sort(rng.integers(0, n // 2, na, dtype=np.uint32))          # about half of A's elements have a partner
    b = np.sort(rng.integers(0, n // 2, n - na, dtype=np.uint32))
    assert -(-n // T) == tiles
    ops = OPS if tiles in (257, SCAN_SWEEP + 1) else (OPS[tiles % 4], OPS[(tiles + 2) % 4])
    for op in ops:
        run_setop(dev, op, "uint", a, b, "arg", "%d tiles" % tiles)


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types(dev, kt):
    T = tile_of(dev, kt, "v4")
    a, b = keys_of_type(kt, T + 1, 5), keys_of_type(kt, 2 * T + 3, 6)   # few distinct keys, the type's specials: runs across tiles
    for i, op in enumerate(OPS):
        run_setop(dev, op, kt, a, b, "v8", "%s v8" % kt)               # 8-byte values with distinct high words
        run_setop(dev, op, kt, b, a, ("v4", "arg", "keys", "arg_only")[i], "%s, reversed" % kt, pass_vb=False)


def test_element_aligned_views(dev):
    """Views at odd element offsets inside their allocations: nothing may assume 16-byte alignment."""
    for i, (kt, mode, offs) in enumerate((("uchar", "keys", (1, 0, 3, 0, 5, 0)), ("uchar", "v8", (1, 8, 1, 24, 7, 8)), ("char", "arg", (13, 0, 2, 0, 1, 4)),
                                          ("ushort", "v4", (2, 4, 6, 12, 10, 4)), ("uint", "v4", (4, 4, 4, 4, 4, 4)), ("uint", "keys", (4, 0, 12, 0, 8, 0)),
                                          ("float", "v8", (4, 8, 8, 8, 12, 8)), ("ulong", "v8", (8, 8, 8, 8, 8, 8)), ("double", "arg_only", (8, 0, 8, 0, 0, 12)))):
        T = tile_of(dev, kt, mode)
        a, b = keys_of_type(kt, T + 37, 8), keys_of_type(kt, 2 * T + 3, 9)
        for op in (OPS[i % 4], OPS[(i + 1) % 4]):
            run_setop(dev, op, kt, a, b, mode, "%s %s at %s" % (kt, mode, offs), offs=offs)


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    for op in ("union", "difference"):
        s = clo.SetOp(op, ctx, "uint", 4)
        for k, (na, nb) in enumerate(((40 * T + 3, 25 * T + 1), (5, 9), (0, 3), (60 * T + 7, 11), (3 * T, 3 * T))):
            run_setop(dev, op, "uint", sorted_uint(na, k), sorted_uint(nb, k + 50), "v4" if k % 2 == 0 else "arg", "call %d" % k, obj=s)
        s.close()


def test_seeded_fuzz(dev):
    """About a hundred cases over ops, modes, key types, sizes and run mixtures; a failure names its case."""
    rng = np.random.default_rng(20240607)
    modes = ("keys", "v4", "v8", "arg", "arg_only")
    for case in range(100):
        op, mode, kt = OPS[rng.integers(4)], modes[rng.integers(5)], KEY_TYPES[rng.integers(len(KEY_TYPES))]
        T = tile_of(dev, kt, mode)
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
        run_setop(dev, op, kt, a, b, mode, "fuzz case %d: %s %s %s %d + %d (seed %d)" % (case, kt, mode, mix, na, nb, seed),
                  pass_vb=bool(rng.integers(2)))


def test_identities_with_the_librarys_own_merge(dev):
    """A second oracle that shares nothing with the model: clo_merge of (A - B) and (B - A) is the symmetric
    difference, bit for bit; the arg indices of intersection and difference partition [0, numel_a); the union has
    numel_b + |A - B| elements."""
    clo, ctx, q = dev
    T = tile_of(dev, "float", "keys")
    a, b = keys_of_type("float", 3 * T + 11, 21), keys_of_type("float", 2 * T + 5, 22)
    a, b = np.concatenate((a, a[:T])), np.concatenate((b, b[-T:]))     # different run lengths in A and in B
    a, b = sort_keys(a), sort_keys(b)
    diff, arg = clo.SetOp("difference", ctx, "float", 0), {op: clo.SetOp(op, ctx, "float", 4) for op in ("intersection", "difference")}
    sym, uni, mer = clo.SetOp("symmetric_difference", ctx, "float", 0), clo.SetOp("union", ctx, "float", 0), clo.Merge(ctx, "float", 0)
    try:
        a_b = diff.with_host_data(a, b, q_exec=q)[0]
        b_a = diff.with_host_data(b, a, q_exec=q)[0]
        merged = mer.with_host_data(a_b, b_a, q_exec=q)[0]
        sd = sym.with_host_data(a, b, q_exec=q)[0]
        assert sd.size > 0 and a_b.size > 0 and b_a.size > 0
        assert np.array_equal(merged.view(np.uint32), sd.view(np.uint32))
        pi, pd = arg["intersection"].with_host_data(a, b, q_exec=q)[1], arg["difference"].with_host_data(a, b, q_exec=q)[1]
        assert pi.size > 0 and pd.size == a_b.size
        assert np.array_equal(np.sort(np.concatenate((pi, pd))), np.arange(a.size, dtype=np.uint32))
        assert (np.diff(pi.astype(np.int64)) > 0).all() and (np.diff(pd.astype(np.int64)) > 0).all()      # each in A's order
        assert uni.with_host_data(a, b, q_exec=q)[0].size == b.size + a_b.size
    finally:
        for x in (diff, sym, uni, mer, *arg.values()):
            x.close()


@pytest.mark.parametrize("layout", ["random", "descending", "runs out of place", "counts above the capacity"])
def test_unsorted_inputs_stay_inside_their_arrays(dev, layout):
    """The bounds contract: the precondition is broken, k and the contents are unspecified and not compared; the call
    succeeds, k <= capacity, the guards around the outputs and num_out are intact and the inputs unchanged. The
    intersection's capacity, min(numel_a, numel_b), is the one a wrong count could exceed: B is the short input."""
    T = tile_of(dev, "uint", "v4")
    rng = np.random.default_rng(9)
    na, nb = 2 * T + 3, T + 1
    if layout == "random":
        a, b = rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
    elif layout == "descending":
        a, b = np.arange(na, 0, -1, dtype=np.uint32), np.arange(nb, 0, -1, dtype=np.uint32) * 2
    elif layout == "runs out of place":   # equal keys everywhere but not together: every probe of a neighbour finds something equal somewhere
        a, b = (np.arange(na, dtype=np.uint32) % 3) * 5, (np.arange(nb, dtype=np.uint32) % 2) * 5
    else:
        # Built for the schedule as it is: A is one run of 3 T fives with a zero planted at the start of its second and
        # third tile, B a five, larger keys, then fives. Every tile of A then finds a lower bound of five just behind its
        # zero and T fives in B: the tiles' intersection counts add up to 3 T - 2 where min(numel_a, numel_b) is T.
        na, nb = 3 * T, T
        a = np.full(na, 5, np.uint32)
        a[T] = a[2 * T] = 0
        b = np.concatenate((np.full(1, 5, np.uint32), np.full(T // 2 - 1, 9, np.uint32), np.full(T - T // 2, 5, np.uint32)))
    for op in OPS:
        for mode in ("keys", "v4", "v8", "arg"):
            run_setop(dev, op, "uint", a, b, mode, "%s %s" % (layout, mode), compare=False)
        run_setop(dev, op, "uint", b[:64], a, "v4", "%s, a short A" % layout, compare=False)
        for kt in ("uchar", "double"):
            run_setop(dev, op, kt, a.astype(_NP[kt]), b.astype(_NP[kt]), "v4", "%s %s" % (layout, kt), compare=False)


@pytest.mark.parametrize("mode", ["keys", "v4", "v8", "arg", "arg_only"])
def test_host_data_form(dev, mode):
    clo, ctx, q = dev
    T = tile_of(dev, "int", mode)
    a, b = keys_of_type("int", T + 9, 1), keys_of_type("int", 2 * T + 1, 2)
    va, vb = values_for(mode, a.size, b.size)
    for op in OPS:
        s = clo.SetOp(op, ctx, "int", _VS[mode])
        ko, vo = s.with_host_data(a, b, va, vb if keeps_b(op) else None, keys_out=mode != "arg_only", q_exec=q if mode != "v4" else None)
        want_k, p = setop(op, a, b)
        assert (ko is None) == (mode == "arg_only") and (vo is None) == (mode == "keys")
        if ko is not None:
            assert np.array_equal(ko, want_k), op
        if vo is not None:
            assert np.array_equal(vo, np.concatenate((va, vb))[p] if va is not None else p), op
        # an empty result, and an empty input
        ko, vo = s.with_host_data(a[:0], b, va[:0] if va is not None else None, vb if va is not None and keeps_b(op) else None, keys_out=mode != "arg_only", q_exec=q)
        got = ko if ko is not None else vo
        assert got.size == (b.size if keeps_b(op) else 0), op
        s.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 elements in all; the transfers on a queue of their own, then no queue at all (the call makes and
    destroys one). The count is read first and says how many rows are copied: inputs that share keys, and inputs whose
    result is empty (the intersection of disjoint arrays, the difference and the symmetric difference of equal ones)."""
    clo, ctx, q = dev
    T = tile_of(dev, "int", "v4")
    a, b = keys_of_type("int", T + 1, 3), keys_of_type("int", T, 4)
    low, high = np.arange(T + 1, dtype=np.int32), np.arange(T, dtype=np.int32) + np.int32(5 * T)
    qc = clo.Queue(ctx)
    try:
        for op in OPS:
            s = clo.SetOp(op, ctx, "int", 4)
            for qe, qcomm in ((q, qc), (None, None)):
                for x, y in ((a, b), (low, high) if op == "intersection" else (low, low)):
                    vx, vy = values_for("v4", x.size, y.size)
                    ko, vo = s.with_host_data(x, y, vx, vy if keeps_b(op) else None, q_exec=qe, q_comm=qcomm)
                    want_k, p = setop(op, x, y)
                    what = (op, qe is None, qcomm is None, x is a)
                    assert np.array_equal(ko, want_k) and np.array_equal(vo, np.concatenate((vx, vy))[p]), what
                    if x is not a and op in ("intersection", "difference", "symmetric_difference"):
                        assert ko.size == 0 and vo.size == 0, what
            s.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    n = 1000
    need = lib.clo_hip_setop_workspace_bytes(n, n)
    assert need > 0 and need % 256 == 0
    ka, kb, ko = (Region(dev, 8 * n + 16, 0, np.concatenate((sorted_uint(n + 4, i), np.zeros(n, np.uint32))), i) for i in range(3))
    va, vb, vo = (Region(dev, 16 * n + 16, 0, None, i) for i in range(3))
    num = Region(dev, 16, 0, None, 0)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(ka_p, va_p, na, kb_p, vb_p, nb, ko_p, vo_p, op=0, num_p=num.ptr, ks=4, kind=0, vs=4, w=ws.ptr, wb=need):
        return lib.clo_hip_setop(op, ka_p, va_p, na, kb_p, vb_p, nb, ko_p, vo_p, num_p, ks, kind, vs, w, wb, s)

    try:
        full = (ka.ptr, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, vo.ptr)
        for op in (-1, 4, 100):
            assert call(*full, op=op) == EARGS
        for kind in (-1, 3):
            assert call(*full, kind=kind) == EARGS
        for ks, vs in ((3, 4), (16, 4), (0, 0), (4, 2), (4, 16)):
            assert call(*full, ks=ks, vs=vs) == EUNSUPPORTED, (ks, vs)
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(ka.ptr, va.ptr, (1 << 32) - n, kb.ptr, vb.ptr, n, ko.ptr, vo.ptr) == EARGS            # n = 2^32
        assert call(ka.ptr, va.ptr, 1 << 32, kb.ptr, vb.ptr, 0, ko.ptr, vo.ptr) == EARGS
        assert call(None, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, vo.ptr) == EARGS                          # a missing array
        assert call(ka.ptr, va.ptr, n, None, vb.ptr, n, ko.ptr, vo.ptr) == EARGS
        assert call(ka.ptr, va.ptr, n, kb.ptr, None, n, ko.ptr, vo.ptr) == EARGS                          # a union looks at values_b
        assert call(ka.ptr, va.ptr, n, kb.ptr, None, n, ko.ptr, vo.ptr, op=3) == EARGS
        assert call(ka.ptr, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, None) == EARGS
        assert call(ka.ptr, None, n, kb.ptr, None, n, None, None, vs=0) == EARGS
        assert call(ka.ptr, None, n, kb.ptr, None, n, ko.ptr, vo.ptr, vs=8) == EARGS                      # the arg form is 4-byte
        assert call(ka.ptr, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, None, vs=0) == EARGS                    # values with value_size 0
        for i in range(8):                                                                              # one misaligned pointer at a time
            args = list(full)
            if i in (2, 5):
                continue
            args[i] += 2
            assert call(*args) == EARGS, i
        args = list(full)
        args[1] += 4
        assert call(*args, vs=8) == EARGS                                                               # 4-aligned is not 8-aligned
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        q.finish()
        for r in (ko, vo, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; an intersection without values_b; 8-byte keys
        # of kind 2 over the same bytes; n 0 needs no workspace and still writes num_out
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        a_keys, b_keys = ka.contents(np.uint32)[:n], kb.contents(np.uint32)[:n]
        assert call(*full) == 0
        q.finish()
        assert first() == setop("union", a_keys, b_keys)[1].size
        assert call(ka.ptr, va.ptr, n, kb.ptr, None, n, ko.ptr, vo.ptr, op=1) == 0
        q.finish()
        assert first() == setop("intersection", a_keys, b_keys)[1].size
        assert call(ka.ptr, None, n // 4, kb.ptr, None, n // 4, ko.ptr, None, op=2, ks=8, kind=2, vs=0) == 0
        q.finish()
        assert first() <= n // 4
        assert call(None, None, 0, None, None, 0, ko.ptr, None, vs=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (ka, kb, ko, va, vb, vo, num):
            r.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "arg"])
@pytest.mark.parametrize("op", OPS)
def test_graph_capture_and_replay(dev, op, mode):
    """clo_hip_setop captured from a client stream after one eager warm-up and replayed three times on new contents of
    the same buffers, the outputs and num_out refilled with a canary before each (the protocol of
    test_gpu_graph_capture.py). The rounds' inputs overlap differently, so that k differs from replay to replay."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T = tile_of(dev, "uint", mode)
    na, nb, vs = 2 * T + 3, T + 1, _VS[mode]
    cap = capacity(op, na, nb)
    valued = mode == "v4"
    need = lib.clo_hip_setop_workspace_bytes(na, nb)
    made = [GC.Mem(gdev, x) for x in (4 * na, 4 * nb, 4 * na, 4 * nb, 4 * cap, 4 * cap, 8, need)]
    ka, kb, va, vb, ko, vo, num, ws = made
    kinds = ["uniform", "all equal", "A below B", "B inside A", "uniform"]
    sent, ks = {}, set()

    def load(k):
        rng = np.random.default_rng(100 + k)
        if kinds[k] == "uniform":
            a, b = np.sort(rng.integers(0, na, na).astype(np.uint32)), np.sort(rng.integers(0, na, nb).astype(np.uint32))
        elif kinds[k] == "all equal":
            a, b = np.full(na, 9 + k, np.uint32), np.full(nb, 9 + k, np.uint32)
        elif kinds[k] == "A below B":
            a, b = np.arange(na, dtype=np.uint32) + np.uint32(k), np.arange(nb, dtype=np.uint32) + np.uint32(na + 5)
        else:
            a, b = np.arange(na, dtype=np.uint32), np.arange(nb, dtype=np.uint32) * np.uint32(2) + np.uint32(1)
        x, y = rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
        sent[k] = (a, b, x, y)
        for m in (ko, vo, num):
            m.fill()
        for mem_, arr in ((ka, a), (kb, b), (va, x), (vb, y)):
            mem_.put(arr)
        want_k, p = setop(op, a, b)
        ks.add(p.size)
        return want_k, (np.concatenate((x, y))[p] if valued else p)

    def enqueue():
        return lib.clo_hip_setop(OPS.index(op), ka.ptr, va.ptr if valued else None, na, kb.ptr, vb.ptr if valued else None, nb, ko.ptr,
                                 vo.ptr if vs else None, num.ptr, 4, 0, vs, ws.ptr, need, q.stream)

    def verify(k, want):
        tag = "%s %s round %d (%s)" % (op, mode, k, kinds[k])
        kept = want[0].size
        assert int(num.get(np.uint64, 1)[0]) == kept, tag + ": num_out"
        rest = GC.canary(np.uint32, cap - kept)
        GC.same(ko.get(np.uint32, cap), np.concatenate((want[0], rest)), tag + ": keys_out")
        GC.same(vo.get(np.uint32, cap), np.concatenate((want[1], rest)) if vs else GC.canary(np.uint32, cap), tag + ": values_out")
        for mem_, arr, name in ((ka, sent[k][0], "keys_a"), (kb, sent[k][1], "keys_b"), (va, sent[k][2], "values_a"), (vb, sent[k][3], "values_b")):
            GC.same(mem_.get(np.uint32, arr.size), arr, tag + ": " + name)

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(ks) >= 3, ks                                         # k differed between the replays
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()
