"""CloReduceByKey (include/clo_reduce.h) on the GPU against the numpy model of tests/rbk_model.py, bit for bit.
Every input and output is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side
(the method of test_gpu_views.py); the outputs are pre-filled with the pattern, and after every call the rows [0, m)
equal the model, the rows from m on, the guards and both inputs are unchanged, and the run count is m. Sizes around
the tile edges (the tile comes from clo_hip_reduce_by_key_tile, not from a constant here), run structures that carry
an open run through tiles without a head, every key size, float keys with both zeros and two NaN payloads, every
value -> sum pair, min / max, views at byte offsets es and 16 - es, absent outputs, the sort-by-key -> reduce-by-key
pipeline on one queue, an object reused for a large, a small and a large call, and the thin C-ABI's status codes."""
import ctypes as C

import numpy as np
import pytest

from rbk_model import rbk

pytestmark = pytest.mark.gpu

G = 256
_PAT = [((np.arange(251 * 16) * 167 + 41 * k) % 251).astype(np.uint8) ^ np.uint8(0xA5) for k in range(5)]
_NP = {"uchar": np.uint8, "ushort": np.uint16, "uint": np.uint32, "int": np.int32, "ulong": np.uint64, "long": np.int64,
       "float": np.float32, "double": np.float64}
_BITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
KEY_TYPES = ["uchar", "ushort", "uint", "int", "ulong", "float", "double"]
PAIRS = [("uint", "uint"), ("uint", "ulong"), ("int", "int"), ("int", "long"), ("long", "long"), ("ulong", "ulong"),
         (None, "uint"), (None, "ulong")]


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


class Region:
    """nbytes at byte G + off of an owned allocation of nbytes + 2 G + 16 bytes filled with a canary pattern."""

    def __init__(self, dev, nbytes, off=0, data=None, salt=0):
        clo, ctx, self.q = dev
        self.n, self.at = nbytes, G + off
        self.host = np.resize(_PAT[salt], nbytes + 2 * G + 16)
        if data is not None:
            self.host[self.at:self.at + nbytes] = np.ascontiguousarray(data).view(np.uint8)
        self.base = clo.Buffer(ctx, self.host.size)
        self.base.write(self.q, self.host)
        self.view = clo.Buffer(ctx, max(nbytes, 1), device_ptr=self.base.ptr + self.at)

    @property
    def ptr(self):
        return self.base.ptr + self.at

    def check(self, want=None, what=""):
        """The view starts with the bytes of `want` (None: nothing) and everything else is what it was."""
        got = self.base.read(self.q, np.uint8, self.host.size)
        exp = self.host.copy()
        if want is not None:
            w = np.ascontiguousarray(want).view(np.uint8)
            assert w.size <= self.n
            exp[self.at:self.at + w.size] = w
        if not np.array_equal(got, exp):
            bad = np.flatnonzero(got != exp)
            where = "the guard below" if bad[0] < self.at else "the guard above" if bad[0] >= self.at + self.n else "the view"
            raise AssertionError("%s: %d bytes differ, first at byte %d of %s (view of %d bytes at %d)"
                                 % (what, bad.size, bad[0] - self.at, where, self.n, self.at))

    def close(self):
        self.view.close()
        self.base.close()


def palette(dt, seed=0):
    """Distinct keys of a type, as many as it has (at most 4099), neighbours always different: floats start with
    -0.0, +0.0 and two NaNs that differ in their payload only."""
    dt = np.dtype(dt)
    bits = _BITS[dt.itemsize]
    rng = np.random.default_rng(1000 + seed)
    count = min(4099, 1 << (8 * dt.itemsize))
    p = np.unique(rng.integers(0, 1 << 63, 3 * count, dtype=np.uint64).astype(bits) if dt.itemsize < 8
                  else rng.integers(0, 1 << 63, 3 * count, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, 3 * count, dtype=np.uint64))
    p = rng.permutation(p)[:count]
    if dt.kind == "f":
        sp = {4: [0x80000000, 0x00000000, 0x7fc00001, 0x7fc00002], 8: [1 << 63, 0, (0x7ff8 << 48) | 1, (0x7ff8 << 48) | 2]}[dt.itemsize]
        sp = np.array(sp, dtype=np.uint64).astype(bits)
        p = np.concatenate((sp, p[~np.isin(p, sp)]))
    return p.view(dt)


def geometric(n, mean, seed):
    heads = np.random.default_rng(seed).random(n) < 1.0 / mean
    if n:
        heads[0] = True
    return np.cumsum(heads) - 1


def structure(name, n, tile, seed=0):
    """Run numbers per element (consecutive runs get consecutive numbers), or for 'unsorted' key numbers."""
    i = np.arange(n, dtype=np.int64)
    if name == "equal":
        return np.zeros(n, np.int64)
    if name == "distinct":
        return i
    if name == "tile":
        return i // tile
    if name == "tile+1":
        return (i + tile - 1) // tile
    if name == "tile-1":
        return (i + 1) // tile
    if name == "ends_on_last":
        r = geometric(n, 100, seed)
        r[-min(n, 3 * tile // 2):] = r[-1] if n else 0     # a long last run: it ends on the last element
        return r
    if name == "last_run_1":
        r = geometric(n, 100, seed)
        if n >= 2:
            r[-1] = r[-2] + 1
        return r
    if name == "alternating":
        return i % 2
    if name.startswith("geo"):
        return geometric(n, int(name[3:]), seed)
    if name == "unsorted":
        return np.random.default_rng(seed).integers(0, 4, n)
    raise KeyError(name)


STRUCTURES = ["equal", "distinct", "tile", "tile+1", "tile-1", "ends_on_last", "last_run_1", "alternating", "geo3", "geo100",
              "geo50000", "unsorted"]


def make_keys(kt, runs, seed=0):
    p = palette(_NP[kt], seed)
    return p[runs % p.size]


def make_values(vt, n, seed):
    """Over the full range of the type, so that 32-bit sums wrap."""
    if vt is None:
        return None
    rng = np.random.default_rng(seed + 77)
    a = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return a.astype(_BITS[np.dtype(_NP[vt]).itemsize]).view(_NP[vt])


def run_case(dev, kt, vt, st, op, keys, values, what, offs=(0, 0, 0, 0), want_k=True, want_a=True, obj=None):
    """One call on views at byte offsets offs = (keys_in, values_in, keys_out, aggr_out); checks everything."""
    clo, ctx, q = dev
    n = keys.size
    ks, ss = keys.itemsize, np.dtype(_NP[st]).itemsize
    r = obj or clo.ReduceByKey(ctx, kt, vt, st, op=op)
    kin = Region(dev, n * ks, offs[0], keys, 0)
    vin = Region(dev, n * values.itemsize, offs[1], values, 1) if values is not None else None
    ko = Region(dev, n * ks, offs[2], None, 2)
    ao = Region(dev, n * ss, offs[3], None, 3)
    cnt = Region(dev, 8, 0, None, 4)
    try:
        evt = r.with_device_data(q, kin.view, vin.view if vin else None, ko.view if want_k else None, ao.view if want_a else None,
                                 cnt.view, n)
        assert evt
        q.finish()
        wk, wa, m = rbk(keys, values, op, _NP[st])
        cnt.check(np.array([m], np.uint64), what + ": run count")
        ko.check(wk if want_k else None, what + ": keys_out")
        ao.check(wa if want_a else None, what + ": aggr_out")
        kin.check(keys, what + ": keys_in")
        if vin:
            vin.check(values, what + ": values_in")
    finally:
        for x in (kin, vin, ko, ao, cnt):
            if x:
                x.close()
        if obj is None:
            r.close()


def tile_of(dev, kt, vt):
    clo = dev[0]
    t = clo.reduce_by_key_tile(np.dtype(_NP[kt]).itemsize, np.dtype(_NP[vt]).itemsize if vt else 0)
    assert t > 0
    return t


def edge_sizes(tile):
    return [0, 1, 2, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1, 70001, (1 << 20) + 3]


@pytest.mark.parametrize("struct", STRUCTURES)
def test_run_structures_at_the_tile_edges(dev, struct):
    """uint keys, uint values summed in uint (the sums wrap) and run lengths in uint, every size around the tile edges."""
    clo, ctx, q = dev
    for vt in ("uint", None):
        tile = tile_of(dev, "uint", vt)
        obj = clo.ReduceByKey(ctx, "uint", vt, "uint")
        for n in edge_sizes(tile):
            keys = make_keys("uint", structure(struct, n, tile, seed=n), seed=1)
            run_case(dev, "uint", vt, "uint", "sum", keys, make_values(vt, n, n), "%s n=%d values=%s" % (struct, n, vt), obj=obj)
        obj.close()


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_and_value_sum_pairs(dev, kt):
    for vt, st in PAIRS:
        tile = tile_of(dev, kt, vt)
        for struct, n in (("geo3", 2 * tile + 1), ("geo100", 70001), ("equal", 3 * tile - 1), ("unsorted", tile + 1)):
            keys = make_keys(kt, structure(struct, n, tile, seed=3), seed=2)
            run_case(dev, kt, vt, st, "sum", keys, make_values(vt, n, 5), "%s %s->%s %s n=%d" % (kt, vt, st, struct, n))


def test_float_keys_compare_by_their_bits(dev):
    """-0.0 | +0.0 and NaN | NaN with another payload are run boundaries; equal NaN bits are one run."""
    for kt, bits in (("float", np.uint32), ("double", np.uint64)):
        p = palette(_NP[kt])[:4]
        assert np.isnan(p[2]) and np.isnan(p[3]) and p[0] == p[1] and len(set(p.view(bits).tolist())) == 4
        keys = np.repeat(np.resize(p, 4000), np.random.default_rng(9).integers(1, 9, 4000))
        wk, wa, m = rbk(keys, None, "sum", np.uint32)
        assert m == 4000
        run_case(dev, kt, None, "uint", "sum", keys, None, kt + " zeros and NaNs")
        run_case(dev, kt, "int", "long", "sum", keys, make_values("int", keys.size, 1), kt + " zeros and NaNs, values")


@pytest.mark.parametrize("op", ["min", "max"])
def test_min_max(dev, op):
    for kt in ("uchar", "uint", "double"):
        for vt, st in (("int", "long"), ("uint", "uint"), ("int", "int"), ("uint", "long"), ("int", "ulong"), ("ulong", "ulong"), ("long", "long"),
                       ("uint", "int")):
            tile = tile_of(dev, kt, vt)
            for struct, n in (("geo100", 2 * tile + 1), ("equal", 2 * tile + 5), ("geo3", 70001), ("geo50000", 5 * tile + 3)):
                keys = make_keys(kt, structure(struct, n, tile, seed=4), seed=3)
                run_case(dev, kt, vt, st, op, keys, make_values(vt, n, 6), "%s %s %s->%s %s n=%d" % (op, kt, vt, st, struct, n))


def test_min_max_without_values_is_refused(dev):
    clo, ctx, q = dev
    from cl_ops_amd.api import CLO_ERROR_ARGS
    r = clo.ReduceByKey(ctx, "uint", "uint", "uint", op="max")
    b = [clo.Buffer(ctx, 64) for _ in range(4)]
    with pytest.raises(clo.CloError) as e:
        r.with_device_data(q, b[0], None, b[1], b[2], b[3], 16)
    assert e.value.code == CLO_ERROR_ARGS
    with pytest.raises(clo.CloError) as e:   # in place
        r.with_device_data(q, b[0], b[1], b[0], b[2], b[3], 16)
    assert e.value.code == CLO_ERROR_ARGS and "overlaps" in e.value.message
    for x in b:
        x.close()
    r.close()


@pytest.mark.parametrize("kt,vt,st", [("uchar", "uint", "uint"), ("ushort", "int", "long"), ("uint", "uint", "ulong"), ("float", "int", "int"),
                                      ("ulong", "ulong", "ulong"), ("double", "uint", "uint")])
def test_element_aligned_views_and_absent_outputs(dev, kt, vt, st):
    """Views at byte offsets es and 16 - es of each array in turn and of all at once; keys_out NULL; aggr_out NULL;
    values NULL."""
    ks, vs, ss = (np.dtype(_NP[t]).itemsize for t in (kt, vt, st))
    tile = tile_of(dev, kt, vt)
    n = 2 * tile + 3
    keys = make_keys(kt, structure("geo100", n, tile, seed=8), seed=4)
    values = make_values(vt, n, 9)
    o = lambda es: [es, 16 - es] if es < 8 else [8, 24]
    cases = []
    for which, es in enumerate((ks, vs, ks, ss)):
        for off in o(es):
            c = [0, 0, 0, 0]
            c[which] = off
            cases.append(tuple(c))
    cases.append((o(ks)[0], o(vs)[1], o(ks)[1], o(ss)[0]))
    for offs in cases:
        run_case(dev, kt, vt, st, "sum", keys, values, "%s %s->%s offsets %s" % (kt, vt, st, offs), offs=offs)
    offs = cases[-1]
    run_case(dev, kt, vt, st, "sum", keys, values, "keys_out NULL", offs=offs, want_k=False)
    run_case(dev, kt, vt, st, "sum", keys, values, "aggr_out NULL", offs=offs, want_a=False)
    run_case(dev, kt, vt, st, "max", keys, values, "aggr_out NULL, max", offs=offs, want_a=False)
    run_case(dev, kt, None, st, "sum", keys, None, "values NULL", offs=offs)
    run_case(dev, kt, None, st, "sum", keys, None, "values NULL, keys_out NULL", offs=offs, want_k=False)
    run_case(dev, kt, None, st, "sum", keys, None, "values NULL, aggr_out NULL", offs=offs, want_a=False)


@pytest.mark.parametrize("struct", ["equal", "distinct", "geo100", "geo50000"])
def test_2p24(dev, struct):
    n = 1 << 24
    tile = tile_of(dev, "uint", "uint")
    keys = make_keys("uint", structure(struct, n, tile, seed=11), seed=5)
    run_case(dev, "uint", "uint", "uint", "sum", keys, make_values("uint", n, 12), struct + " 2^24")
    run_case(dev, "uint", None, "ulong", "sum", keys, None, struct + " 2^24 run lengths")


def test_2p26_plus_5(dev):
    n = (1 << 26) + 5
    tile = tile_of(dev, "uint", "uint")
    keys = make_keys("uint", structure("geo50000", n, tile, seed=13), seed=6)
    run_case(dev, "uint", "uint", "ulong", "sum", keys, make_values("uint", n, 14), "geo50000 2^26+5")


def test_host_data_form(dev):
    clo, ctx, q = dev
    tile = tile_of(dev, "uint", "int")
    n = 3 * tile + 17
    keys = make_keys("uint", structure("geo100", n, tile, seed=15), seed=7)
    values = make_values("int", n, 16)
    r = clo.ReduceByKey(ctx, "uint", "int", "long", op="min")
    for qe in (q, None):
        ko, ao = r.with_host_data(keys, values, q_exec=qe)
        wk, wa, m = rbk(keys, values, "min", np.int64)
        assert ko.size == m and np.array_equal(ko, wk) and ao.dtype == np.int64 and np.array_equal(ao, wa)
    ko, ao = r.with_host_data(keys, values, want_aggr=False)
    assert ao is None and np.array_equal(ko, wk)
    ko, ao = r.with_host_data(keys[:0], values[:0])
    assert ko.size == 0 and ao.size == 0
    r.close()
    r = clo.ReduceByKey(ctx, "float")
    k = np.array([0.0, -0.0, -0.0, 1.5], np.float32)
    ko, ao = r.with_host_data(k)
    assert list(ao) == [1, 2, 1] and np.array_equal(ko.view(np.uint32), k.view(np.uint32)[[0, 1, 3]])
    r.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 elements; the transfers on a queue of their own, then no queue at all (the call makes and destroys
    one). The run count is read first and says how many rows are copied: many runs, one run, and no run at all (the
    only input without a run is the empty one)."""
    clo, ctx, q = dev
    tile = tile_of(dev, "uint", "int")
    n = 2 * tile + 1
    keys = make_keys("uint", structure("geo100", n, tile, seed=25), seed=8)
    values = make_values("int", n, 26)
    r = clo.ReduceByKey(ctx, "uint", "int", "long", op="sum")
    qc = clo.Queue(ctx)
    try:
        for qe, qcomm in ((q, qc), (None, None)):
            for k in (keys, np.full(n, 7, np.uint32), keys[:0]):
                ko, ao = r.with_host_data(k, values[:k.size], q_exec=qe, q_comm=qcomm)
                wk, wa, m = rbk(k, values[:k.size], "sum", np.int64)
                assert ko.size == m == ao.size and np.array_equal(ko, wk) and np.array_equal(ao, wa), (qe is None, qcomm is None, k.size)
    finally:
        r.close()
        qc.close()


def test_sort_by_key_then_reduce_by_key_on_one_queue(dev):
    """The pipeline this exists for: no host synchronisation between the two calls."""
    clo, ctx, q = dev
    n = 1 << 22
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 1000, n, dtype=np.uint32)
    values = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    kin, vin, ks, vs = Region(dev, n * 4, 0, keys, 0), Region(dev, n * 4, 0, values, 1), Region(dev, n * 4, 0, None, 2), Region(dev, n * 4, 0, None, 3)
    rk, ra, cnt = Region(dev, n * 4, 0, None, 2), Region(dev, n * 4, 0, None, 3), Region(dev, 8, 0, None, 4)
    s = clo.Sorter("satradix", ctx, "uint")
    r = clo.ReduceByKey(ctx, "uint", "uint", "uint")
    try:
        assert s.by_key_with_device_data(q, kin.view, vin.view, ks.view, vs.view, n)
        assert r.with_device_data(q, ks.view, vs.view, rk.view, ra.view, cnt.view, n)
        q.finish()
        uk = np.unique(keys)
        want = np.zeros(1000, np.uint32)
        with np.errstate(over="ignore"):
            np.add.at(want, keys, values)
        cnt.check(np.array([uk.size], np.uint64), "run count")
        rk.check(uk, "distinct keys")
        ra.check(want[uk], "sums per key")
        kin.check(keys, "keys_in")
        vin.check(values, "values_in")
    finally:
        s.close()
        r.close()
        for x in (kin, vin, ks, vs, rk, ra, cnt):
            x.close()


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    tile = tile_of(dev, "uint", "uint")
    obj = clo.ReduceByKey(ctx, "uint", "uint", "ulong")
    for n, struct in (((1 << 22) + 1, "geo100"), (5, "distinct"), (tile + 1, "equal"), ((1 << 22) + 7, "geo50000"), ((1 << 23) + 3, "geo3")):
        keys = make_keys("uint", structure(struct, n, tile, seed=n), seed=8)
        run_case(dev, "uint", "uint", "ulong", "sum", keys, make_values("uint", n, n), "reuse n=%d %s" % (n, struct), obj=obj)
    obj.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib, CLO_HIP_EARGS, CLO_HIP_EUNSUPPORTED, CLO_HIP_EWORKSPACE
    n = 100000
    need = lib.clo_hip_reduce_by_key_workspace_bytes(n)
    ws, k, o, a, c = (clo.Buffer(ctx, b) for b in (need + 512, n * 8, n * 8, n * 8, 64))
    before = c.read(q, np.uint8, 64)
    call = lambda cnt, w, wb, key_size=4, vt=5, st=5, op=0, ko=o.ptr, ao=a.ptr, vals=k.ptr, numel=n: lib.clo_hip_reduce_by_key(
        k.ptr, vals, ko, ao, cnt, numel, key_size, vt, st, op, w, wb, q.stream)
    assert call(c.ptr + 4, ws.ptr, need) == CLO_HIP_EARGS            # the count word: 8 bytes
    assert call(c.ptr, ws.ptr + 64, need) == CLO_HIP_EARGS           # the workspace: 256 bytes
    assert call(None, ws.ptr, need) == CLO_HIP_EARGS
    assert call(c.ptr, ws.ptr, need, ko=None, ao=None) == CLO_HIP_EARGS
    assert call(c.ptr, ws.ptr, need, op=3) == CLO_HIP_EARGS
    assert call(c.ptr, ws.ptr, need, op=1, vals=None) == CLO_HIP_EARGS
    assert call(c.ptr, ws.ptr, need, numel=1 << 32) == CLO_HIP_EARGS
    assert call(c.ptr, ws.ptr, need - 1) == CLO_HIP_EWORKSPACE
    assert call(c.ptr, ws.ptr, 0) == CLO_HIP_EWORKSPACE
    for kw in (dict(key_size=3), dict(vt=9), dict(st=9), dict(st=10), dict(vt=3), dict(vt=7, st=5), dict(st=8), dict(st=11)):
        assert call(c.ptr, ws.ptr, need, **kw) == CLO_HIP_EUNSUPPORTED, kw
    q.finish()
    assert np.array_equal(c.read(q, np.uint8, 64), before)          # none of them touched the count
    assert call(c.ptr, ws.ptr, need, numel=0) == 0
    q.finish()
    assert c.read(q, np.uint64, 1)[0] == 0
    for x in (ws, k, o, a, c):
        x.close()
