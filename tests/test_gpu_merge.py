"""CloMerge (include/clo_merge.h) on the GPU against the numpy model of tests/merge_model.py, bit for bit. Every array
is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs are pre-filled with the pattern, and after every call they equal the model while
the guards and all inputs are unchanged. With T = clo_hip_merge_tile: sizes around the tile edges in every value mode,
where the merge path runs (one input below the other, alternation, a split on a tile boundary, a short input inside a
long one), ties (the stability cases: values carry the source index), every key type with its special values, the
library's own by-key sort as a second oracle, element-aligned views, more tiles than the chip holds at once, one object
used large -> small -> large, unsorted inputs (the bounds contract only), the host-data form, the thin ABI's status
codes, and clo_hip_merge captured into a graph and replayed."""
import numpy as np
import pytest

from merge_model import merge, sort_keys
from test_gpu_histogram import Region

pytestmark = pytest.mark.gpu

_NP = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
       "long": np.int64, "ulong": np.uint64, "half": np.float16, "float": np.float32, "double": np.float64}
_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
KEY_TYPES = list(_NP)
_KIND = {"i": 1, "u": 0, "f": 2}
# value modes: keys only; 4-byte values; 8-byte values; argmerge with keys_out; argmerge without
_VS = {"keys": 0, "v4": 4, "v8": 8, "arg": 4, "arg_only": 4}


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def tile_of(dev, kt, mode="keys"):
    t = dev[0].merge_tile(np.dtype(_NP[kt]).itemsize, _VS[mode])
    assert t > 0 and t % 64 == 0
    return t


def values_for(mode, na, nb):
    """Values that carry the source index in A || B; the 8-byte ones with a non-zero high word that differs per element."""
    if mode == "v4":
        v = np.arange(na + nb, dtype=np.uint32)
    elif mode == "v8":
        i = np.arange(na + nb, dtype=np.uint64)
        v = ((np.uint64(0xC0DE0000) + (i * np.uint64(2654435761) & np.uint64(0xFFFF))) << np.uint64(32)) | i
    else:
        return None, None
    return v[:na], v[na:]


def guards_intact(r, what):
    """The guard bytes on both sides of the region's view are what they were (the view itself is not looked at)."""
    got = r.base.read(r.q, np.uint8, r.host.size)
    for lo, hi, where in ((0, r.at, "below"), (r.at + r.n, r.host.size, "above")):
        assert np.array_equal(got[lo:hi], r.host[lo:hi]), "%s: the guard %s the view was written" % (what, where)


def run_merge(dev, kt, a, b, mode, what, offs=(0, 0, 0, 0, 0, 0), obj=None, compare=True):
    """One call on views at byte offsets offs = (keys_a, values_a, keys_b, values_b, keys_out, values_out); checks
    everything. compare False (unsorted inputs): success, guards and inputs only."""
    clo, ctx, q = dev
    dt = np.dtype(_NP[kt])
    a, b = np.ascontiguousarray(a, dtype=dt), np.ascontiguousarray(b, dtype=dt)
    na, nb, vs = a.size, b.size, _VS[mode]
    n = na + nb
    va, vb = values_for(mode, na, nb)
    m = obj or clo.Merge(ctx, kt, vs)
    ka_r, kb_r = Region(dev, a.nbytes, offs[0], a, 0), Region(dev, b.nbytes, offs[2], b, 1)
    va_r = Region(dev, va.nbytes, offs[1], va, 1) if va is not None else None
    vb_r = Region(dev, vb.nbytes, offs[3], vb, 0) if vb is not None else None
    ko_r = Region(dev, n * dt.itemsize, offs[4], None, 2) if mode != "arg_only" else None
    vo_r = Region(dev, n * vs, offs[5], None, 2) if vs else None
    view = lambda r: r.view if r is not None else None
    try:
        assert m.with_device_data(q, ka_r.view, view(va_r), na, kb_r.view, view(vb_r), nb, view(ko_r), view(vo_r)), what
        q.finish()
        if compare:
            want_k, p = merge(a, b)
            if ko_r:
                ko_r.check(want_k, what + ": keys_out")
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
            vb_r.check(vb, what + ": values_b")
    finally:
        for r in (ka_r, kb_r, va_r, vb_r, ko_r, vo_r):
            if r:
                r.close()
        if obj is None:
            m.close()


def sorted_uint(n, seed, span=None):
    """n ascending uint keys from a narrow range, so that ties occur inside and across the inputs."""
    rng = np.random.default_rng(seed)
    return np.sort(rng.integers(0, span or max(4, n // 3), n, dtype=np.uint32))


@pytest.mark.parametrize("mode", ["keys", "v4", "arg"])
def test_sizes_around_the_tile_edges(dev, mode):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", mode)
    sizes = (0, 1, 2, 63, 64, 65, T - 1, T, T + 1, 2 * T + 3)
    obj = clo.Merge(ctx, "uint", _VS[mode])
    for na in sizes:
        for nb in sizes:
            if na + nb == 0:   # test_both_empty
                continue
            span = max(4, (na + nb) // 3)
            run_merge(dev, "uint", sorted_uint(na, na * 31 + nb, span), sorted_uint(nb, nb * 17 + na + 1, span), mode,
                      "%s %d + %d" % (mode, na, nb), obj=obj)
    obj.close()


def test_both_empty(dev):
    """Nothing is enqueued that writes: outputs given keep their canary."""
    clo, ctx, q = dev
    for mode in ("keys", "v4", "arg"):
        m = clo.Merge(ctx, "uint", _VS[mode])
        ko, vo = Region(dev, 64, 0, None, 2), Region(dev, 64, 0, None, 2)
        try:
            assert m.with_device_data(q, None, None, 0, None, None, 0, ko.view, vo.view if _VS[mode] else None)
            q.finish()
            ko.check(None, mode + ": keys_out")
            vo.check(None, mode + ": values_out")
        finally:
            ko.close()
            vo.close()
            m.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "arg_only"])
def test_where_the_path_runs(dev, mode):
    T = tile_of(dev, "uint", mode)
    u = lambda x: np.asarray(x, dtype=np.uint32)
    lo, hi = np.arange(2 * T + 3), np.arange(T + 1) + 10 * T
    cases = {
        "A below B": (lo, hi),                          # whole tiles from A, the switch to B inside a tile
        "B below A": (hi, lo),
        "B below A, equal lengths": (np.arange(T) + 10 * T, np.arange(T)),
        "alternation": (2 * np.arange(T + 40), 2 * np.arange(T + 41) + 1),                 # a0 < b0 < a1 < ...
        "alternation, B first": (2 * np.arange(T + 41) + 1, 2 * np.arange(T + 40)),
        "split on a tile boundary": (np.arange(T), np.arange(T) + T),                      # the first T outputs are exactly A
        "split on the second boundary": (np.arange(2 * T) * 2, np.concatenate((np.arange(T) * 2 + 1, np.arange(T) + 8 * T))),
        "5 of A inside 3 T of B": ([T // 2, T - 1, T, 2 * T + 1, 5 * T], np.arange(3 * T)),
        "5 of B inside 3 T of A": (np.arange(3 * T), [0, T - 1, T, T, 2 * T]),
        "5 of A below, 3 T of B": ([0, 0, 0, 0, 0], np.arange(3 * T) + 1),
        "5 of A above 3 T of B": (np.arange(5) + 4 * T, np.arange(3 * T)),
    }
    for name, (a, b) in cases.items():
        run_merge(dev, "uint", u(a), u(b), mode, "%s, %s" % (name, mode))


@pytest.mark.parametrize("mode", ["v4", "arg", "v8"])
def test_ties_keep_a_before_b(dev, mode):
    """The stability cases. The values are the source indices: any reordering among equal keys shows."""
    T = tile_of(dev, "uint", mode)
    u = lambda *parts: np.concatenate([np.full(c, k, np.uint32) for k, c in parts])
    run_merge(dev, "uint", u((7, 2 * T + 3)), u((7, T + 1)), mode, "all equal, " + mode)       # all of A, then all of B
    run_merge(dev, "uint", u((7, T + 1)), u((7, 2 * T + 3)), mode, "all equal, B longer, " + mode)
    # eight distinct keys: runs of 1.5 T equal keys in both inputs at once, straddling tile boundaries in both
    r = T + T // 2
    eight = [(k * 3 + 1, r + k) for k in range(8)]
    run_merge(dev, "uint", u(*eight), u(*[(k, c + 5) for k, c in eight]), mode, "eight keys, " + mode)
    # a run of equal keys (from both inputs) that begins one element before / one after / on a tile boundary of the output
    for start in (T - 1, T + 1, T, 2 * T - 1, 2 * T + 1):
        below_a = start // 2
        a = u((0, below_a), (5, T), (9, 3))
        b = u((0, start - below_a), (5, T + 2), (6, 1))
        run_merge(dev, "uint", a, b, mode, "tie run from output %d, %s" % (start, mode))


def keys_of_type(kt, n, seed):
    """n keys of type kt in the merge's order, from few distinct values (ties) that include the type's edges."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(_NP[kt])
    if dt.kind == "f":
        bits = 8 * dt.itemsize
        mant = {16: 10, 32: 23, 64: 52}[bits]
        sign, exp_all = 1 << (bits - 1), ((1 << (bits - 1)) - 1) ^ ((1 << mant) - 1)
        pos = [0, exp_all, exp_all | 1, exp_all | 3, exp_all | (1 << (mant - 1)), exp_all | (1 << (mant - 1)) | 6]   # +0, +inf, four NaN payloads
        special = np.array(pos + [x | sign for x in pos], dtype=_U[dt.itemsize]).view(dt)
        pool = np.concatenate((special, np.array([-3.5, -1.0, -0.25, 0.25, 1.0, 2.0, 1000.0], dtype=dt)))
    else:
        info = np.iinfo(dt)
        mid = [-3, -2, -1, 0, 1, 2, 3] if dt.kind == "i" else [0, 1, 2, info.max // 2, info.max // 2 + 1]   # signed: across zero
        pool = np.array([info.min, info.max, info.max - 1] + mid, dtype=dt)
    return sort_keys(pool[rng.integers(0, pool.size, n)])


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types(dev, kt):
    for mode in ("v4", "v8"):
        T = tile_of(dev, kt, mode)
        a, b = keys_of_type(kt, T + 1, 5), keys_of_type(kt, 2 * T + 3, 6)
        run_merge(dev, kt, a, b, mode, "%s %s" % (kt, mode))
    run_merge(dev, kt, b, a, "arg", "%s arg" % kt)
    run_merge(dev, kt, a, b[:7], "keys", "%s keys" % kt)


@pytest.mark.parametrize("kt", ["uint", "int", "float"])
def test_against_the_librarys_own_sort(dev, kt):
    """Sort each half by key (values = index), merge the two on the same queue with no host synchronisation in
    between, and compare with the by-key sort of the concatenation: the same bits."""
    clo, ctx, q = dev
    T = tile_of(dev, kt, "v4")
    n = 3 * T + 7
    h1, h2 = n // 2, n - n // 2
    rng = np.random.default_rng(3)
    dt = np.dtype(_NP[kt])
    keys = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    keys[::3] &= np.uint32(0x80000003)                                          # ties, of both signs
    if kt == "float":
        keys[::17] = np.resize(np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc00002], np.uint32), keys[::17].shape)
    keys = keys.view(dt)
    index = np.concatenate((np.arange(h1, dtype=np.uint32), np.arange(h2, dtype=np.uint32)))
    B = lambda nbytes: clo.Buffer(ctx, nbytes)
    kin, vin = B(4 * n), B(4 * n)
    k1, v1, k2, v2 = B(4 * h1), B(4 * h1), B(4 * h2), B(4 * h2)
    mk, mv, sk, sv = B(4 * n), B(4 * n), B(4 * n), B(4 * n)
    in1 = clo.Buffer(ctx, 4 * h1, device_ptr=kin.ptr)
    in2 = clo.Buffer(ctx, 4 * h2, device_ptr=kin.ptr + 4 * h1)
    s, m = clo.Sorter("satradix", ctx, kt), clo.Merge(ctx, kt, 4)
    try:
        kin.write(q, keys)
        vin.write(q, index)
        s.by_key_with_device_data(q, in1, None, k1, v1, h1)
        s.by_key_with_device_data(q, in2, None, k2, v2, h2)
        m.with_device_data(q, k1, v1, h1, k2, v2, h2, mk, mv)
        s.by_key_with_device_data(q, kin, vin, sk, sv, n)
        q.finish()
        got_k, got_v = mk.read(q, np.uint32, n), mv.read(q, np.uint32, n)
        assert np.array_equal(got_k, sk.read(q, np.uint32, n)) and np.array_equal(got_v, sv.read(q, np.uint32, n))
        want_k, p = merge(sort_keys(keys[:h1]), sort_keys(keys[h1:]))           # and the model agrees with both
        assert np.array_equal(got_k, want_k.view(np.uint32))
    finally:
        for x in (in1, in2, kin, vin, k1, v1, k2, v2, mk, mv, sk, sv, s, m):
            x.close()


def test_element_aligned_views(dev):
    """Views at odd element offsets inside their allocations: nothing may assume 16-byte alignment."""
    for kt, mode, offs in (("uchar", "keys", (1, 0, 3, 0, 5, 0)), ("uchar", "v8", (1, 8, 1, 24, 7, 8)), ("char", "arg", (13, 0, 2, 0, 1, 4)),
                           ("ushort", "v4", (2, 4, 6, 12, 10, 4)), ("uint", "v4", (4, 4, 4, 4, 4, 4)), ("uint", "keys", (4, 0, 12, 0, 8, 0)),
                           ("float", "v8", (4, 8, 8, 8, 12, 8)), ("ulong", "v8", (8, 8, 8, 8, 8, 8)), ("double", "arg_only", (8, 0, 8, 0, 0, 12))):
        T = tile_of(dev, kt, mode)
        a, b = keys_of_type(kt, T + 37, 8), keys_of_type(kt, 2 * T + 3, 9)
        run_merge(dev, kt, a, b, mode, "%s %s at %s" % (kt, mode, offs), offs=offs)


def test_more_tiles_than_the_chip_holds(dev):
    na, nb = (1 << 22) + 5, (1 << 21) + 3
    assert (na + nb) // tile_of(dev, "uint", "v4") > 256 * 8
    rng = np.random.default_rng(1)
    a = np.sort(rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32))
    b = np.sort(rng.integers(0, 1 << 20, nb, dtype=np.uint64).astype(np.uint32) << np.uint32(12))   # ties inside B and with A's range
    run_merge(dev, "uint", a, b, "v4", "2^22 + 5 and 2^21 + 3")


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    m = clo.Merge(ctx, "uint", 4)
    for k, (na, nb) in enumerate(((40 * T + 3, 25 * T + 1), (5, 9), (0, 3), (60 * T + 7, 11), (3 * T, 3 * T))):
        run_merge(dev, "uint", sorted_uint(na, k), sorted_uint(nb, k + 50), "v4" if k % 2 == 0 else "arg", "call %d" % k, obj=m)
    m.close()


@pytest.mark.parametrize("layout", ["random", "descending"])
def test_unsorted_inputs_stay_inside_their_arrays(dev, layout):
    """The bounds contract: the precondition is broken, the contents are unspecified and not compared; the call
    succeeds, the guards around both outputs are intact and the inputs unchanged. (The kernel clamps the split points
    it reads to what the sizes allow and takes one existing element per step.)"""
    T = tile_of(dev, "uint", "v4")
    rng = np.random.default_rng(9)
    na, nb = 2 * T + 3, T + 1
    if layout == "random":
        a, b = rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
    else:
        a, b = np.arange(na, 0, -1, dtype=np.uint32), np.arange(nb, 0, -1, dtype=np.uint32) * 2
    for mode in ("keys", "v4", "v8", "arg"):
        run_merge(dev, "uint", a, b, mode, "%s %s" % (layout, mode), compare=False)
    for kt in ("uchar", "double"):
        run_merge(dev, kt, a.astype(_NP[kt]), b.astype(_NP[kt]), "v4", "%s %s" % (layout, kt), compare=False)


@pytest.mark.parametrize("mode", ["keys", "v4", "v8", "arg", "arg_only"])
def test_host_data_form(dev, mode):
    clo, ctx, q = dev
    T = tile_of(dev, "int", mode)
    a, b = keys_of_type("int", T + 9, 1), keys_of_type("int", 2 * T + 1, 2)
    va, vb = values_for(mode, a.size, b.size)
    m = clo.Merge(ctx, "int", _VS[mode])
    ko, vo = m.with_host_data(a, b, va, vb, keys_out=mode != "arg_only", q_exec=q if mode != "v4" else None)
    m.close()
    want_k, p = merge(a, b)
    assert (ko is None) == (mode == "arg_only") and (vo is None) == (mode == "keys")
    if ko is not None:
        assert np.array_equal(ko, want_k)
    if vo is not None:
        assert np.array_equal(vo, np.concatenate((va, vb))[p] if va is not None else p)


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 merged elements; the transfers on a queue of their own, then no queue at all (the call makes and
    destroys one); with values and as argmerge."""
    clo, ctx, q = dev
    qc = clo.Queue(ctx)
    try:
        for mode in ("v4", "arg"):
            T = tile_of(dev, "int", mode)
            a, b = keys_of_type("int", T + 1, 3), keys_of_type("int", T, 4)
            va, vb = values_for(mode, a.size, b.size)
            want_k, p = merge(a, b)
            m = clo.Merge(ctx, "int", _VS[mode])
            for qe, qcomm in ((q, qc), (None, None)):
                ko, vo = m.with_host_data(a, b, va, vb, q_exec=qe, q_comm=qcomm)
                assert np.array_equal(ko, want_k), (mode, qe is None, qcomm is None)
                assert np.array_equal(vo, np.concatenate((va, vb))[p] if va is not None else p), (mode, qe is None, qcomm is None)
            m.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    n = 1000
    need = lib.clo_hip_merge_workspace_bytes(n, n)
    assert need > 0 and need % 256 == 0
    ka, kb, ko = (Region(dev, 4 * n + 16, 0, sorted_uint(n + 4, i), i) for i in range(3))
    va, vb, vo = (Region(dev, 8 * n + 16, 0, None, i) for i in range(3))
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(ka_p, va_p, na, kb_p, vb_p, nb, ko_p, vo_p, ks=4, kind=0, vs=4, w=ws.ptr, wb=need):
        return lib.clo_hip_merge(ka_p, va_p, na, kb_p, vb_p, nb, ko_p, vo_p, ks, kind, vs, w, wb, s)

    try:
        full = (ka.ptr, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, vo.ptr)
        for kind in (-1, 3):
            assert call(*full, kind=kind) == EARGS
        for ks, vs in ((3, 4), (16, 4), (0, 0), (4, 2), (4, 16)):
            assert call(*full, ks=ks, vs=vs) == EUNSUPPORTED, (ks, vs)
        assert call(ka.ptr, va.ptr, (1 << 32) - n, kb.ptr, vb.ptr, n, ko.ptr, vo.ptr) == EARGS            # n = 2^32
        assert call(ka.ptr, va.ptr, 1 << 32, kb.ptr, vb.ptr, 0, ko.ptr, vo.ptr) == EARGS
        assert call(None, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, vo.ptr) == EARGS                          # a missing array
        assert call(ka.ptr, va.ptr, n, None, vb.ptr, n, ko.ptr, vo.ptr) == EARGS
        assert call(ka.ptr, va.ptr, n, kb.ptr, None, n, ko.ptr, vo.ptr) == EARGS
        assert call(ka.ptr, va.ptr, n, kb.ptr, vb.ptr, n, ko.ptr, None) == EARGS
        assert call(ka.ptr, None, n, kb.ptr, None, n, None, None, vs=0) == EARGS
        assert call(ka.ptr, None, n, kb.ptr, None, n, ko.ptr, vo.ptr, vs=8) == EARGS                      # argmerge is 4-byte
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
        for r in (ko, vo):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size, 8-byte keys of kind 2 over the same bytes
        assert call(*full) == 0
        assert call(ka.ptr, None, n // 4, kb.ptr, None, n // 4, ko.ptr, None, ks=8, kind=2, vs=0) == 0   # (n / 2 outputs of 8 bytes)
        assert call(None, None, 0, None, None, 0, ko.ptr, None, vs=0, w=None, wb=0) == 0                # n 0 needs no workspace
        q.finish()
    finally:
        ws.close()
        for r in (ka, kb, ko, va, vb, vo):
            r.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "arg"])
def test_graph_capture_and_replay(dev, mode):
    """clo_hip_merge captured from a client stream after one eager warm-up and replayed three times on new contents of
    the same buffers, the outputs refilled with a canary before each (the protocol of test_gpu_graph_capture.py)."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T = tile_of(dev, "uint", mode)
    na, nb, vs = 2 * T + 3, T + 1, _VS[mode]
    n = na + nb
    valued = mode == "v4"
    need = lib.clo_hip_merge_workspace_bytes(na, nb)
    made = [GC.Mem(gdev, x) for x in (4 * na, 4 * nb, 4 * na, 4 * nb, 4 * n, 4 * n, need)]
    ka, kb, va, vb, ko, vo, ws = made
    kinds = ["uniform", "all equal", "A below B", "B below A", "uniform"]
    sent = {}

    def load(k):
        rng = np.random.default_rng(100 + k)
        if kinds[k] == "uniform":
            a, b = np.sort(rng.integers(0, n, na).astype(np.uint32)), np.sort(rng.integers(0, n, nb).astype(np.uint32))
        elif kinds[k] == "all equal":
            a, b = np.full(na, 9 + k, np.uint32), np.full(nb, 9 + k, np.uint32)
        else:
            a, b = np.arange(na, dtype=np.uint32) + np.uint32(k), np.arange(nb, dtype=np.uint32) + np.uint32(na + 5)
            if kinds[k] == "B below A":
                a, b = (b[0] + np.arange(na, dtype=np.uint32)), np.arange(nb, dtype=np.uint32)
        x, y = rng.integers(0, 1 << 32, na, dtype=np.uint64).astype(np.uint32), rng.integers(0, 1 << 32, nb, dtype=np.uint64).astype(np.uint32)
        sent[k] = (a, b, x, y)
        ko.fill()
        vo.fill()
        for mem_, arr in ((ka, a), (kb, b), (va, x), (vb, y)):
            mem_.put(arr)
        want_k, p = merge(a, b)
        return want_k, (np.concatenate((x, y))[p] if valued else p)

    def enqueue():
        return lib.clo_hip_merge(ka.ptr, va.ptr if valued else None, na, kb.ptr, vb.ptr if valued else None, nb, ko.ptr,
                                 vo.ptr if vs else None, 4, 0, vs, ws.ptr, need, q.stream)

    def verify(k, want):
        tag = "%s round %d (%s)" % (mode, k, kinds[k])
        GC.same(ko.get(np.uint32, n), want[0], tag + ": keys_out")
        GC.same(vo.get(np.uint32, n), want[1] if vs else GC.canary(np.uint32, n), tag + ": values_out")
        for mem_, arr, name in ((ka, sent[k][0], "keys_a"), (kb, sent[k][1], "keys_b"), (va, sent[k][2], "values_a"), (vb, sent[k][3], "values_b")):
            GC.same(mem_.get(np.uint32, arr.size), arr, tag + ": " + name)

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()
