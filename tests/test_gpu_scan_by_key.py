"""CloScanByKey (include/clo_scan_by_key.h) on the GPU against the numpy model of tests/sbk_model.py, bit for bit.
Every input and output is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side
(the Region of test_gpu_reduce_by_key.py); the output is pre-filled with the pattern, and after every call it equals
the model over its whole length while the guards and both inputs are unchanged (in place: the values' view holds the
results, its guards are unchanged). Sizes around the tile edges (the tile comes from clo_hip_scan_by_key_tile, not
from a constant here), the twelve run structures of the reduce-by-key tests, structures that carry an open run
through tiles without a head, every key type, float keys with both zeros and two NaN payloads, every value -> sum
pair, min / max with the identity at every head of the exclusive form, sums that wrap, views at byte offsets es and
16 - es, in place, 2^24 and 2^26 + 5 elements, the host-data form, an object reused for a large, a small and a large
call, the sort-by-key -> scan-by-key -> reduce-by-key pipeline on one queue, and the thin C-ABI's status codes.
Every comparison is exact integer equality."""
import numpy as np
import pytest

from sbk_model import sbk, heads_of, identity
from rbk_model import rbk
from test_gpu_reduce_by_key import Region, palette, structure, make_keys, make_values, STRUCTURES, KEY_TYPES, _NP

pytestmark = pytest.mark.gpu

PAIRS = [("uint", "uint"), ("uint", "ulong"), ("int", "int"), ("int", "long"), ("long", "long"), ("ulong", "ulong"),
         ("uint", "int"), ("int", "ulong"), (None, "uint"), (None, "ulong")]


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def run_case(dev, kt, vt, st, op, inclusive, keys, values, what, offs=(0, 0, 0), in_place=False, obj=None):
    """One call on views at byte offsets offs = (keys_in, values_in, data_out); checks everything."""
    clo, ctx, q = dev
    n = keys.size
    ks, ss = keys.itemsize, np.dtype(_NP[st]).itemsize
    r = obj or clo.ScanByKey(ctx, kt, vt, st, op=op, inclusive=inclusive)
    assert r.inclusive == bool(inclusive) and r.op == op
    kin = Region(dev, n * ks, offs[0], keys, 0)
    vin = Region(dev, n * values.itemsize, offs[1], values, 1) if values is not None else None
    out = None if in_place else Region(dev, n * ss, offs[2], None, 3)
    try:
        evt = r.with_device_data(q, kin.view, vin.view if vin else None, vin.view if in_place else out.view, n)
        assert evt
        q.finish()
        want = sbk(keys, values, op, _NP[st], inclusive)
        assert want.size == n and want.dtype == np.dtype(_NP[st])
        kin.check(keys, what + ": keys_in")
        if in_place:
            vin.check(want, what + ": values_in after the call in place")
        else:
            out.check(want, what + ": data_out")
            if vin:
                vin.check(values, what + ": values_in")
    finally:
        for x in (kin, vin, out):
            if x:
                x.close()
        if obj is None:
            r.close()


def tile_of(dev, kt, vt):
    clo = dev[0]
    t = clo.scan_by_key_tile(np.dtype(_NP[kt]).itemsize, np.dtype(_NP[vt]).itemsize if vt else 0)
    assert t > 0
    return t


def edge_sizes(tile):
    return [0, 1, 3, 4, 5, tile - 1, tile, tile + 1, 2 * tile - 1, 2 * tile + 1, 4 * tile + 5]


@pytest.mark.parametrize("struct", STRUCTURES)
def test_run_structures_at_the_tile_edges(dev, struct):
    """uint keys; uint values summed in uint (the sums wrap) and the ranks in uint; both kinds; every edge size."""
    clo, ctx, q = dev
    for vt in ("uint", None):
        tile = tile_of(dev, "uint", vt)
        for inclusive in (False, True):
            obj = clo.ScanByKey(ctx, "uint", vt, "uint", inclusive=inclusive)
            for n in edge_sizes(tile):
                keys = make_keys("uint", structure(struct, n, tile, seed=n), seed=1)
                run_case(dev, "uint", vt, "uint", "sum", inclusive, keys, make_values(vt, n, n),
                         "%s n=%d values=%s inclusive=%s" % (struct, n, vt, inclusive), obj=obj)
            obj.close()


@pytest.mark.parametrize("struct", ["equal", "geo50000"])
def test_open_runs_carried_through_tiles_without_a_head(dev, struct):
    """The carry path: a run that spans several whole tiles, for every op and both kinds, 32- and 64-bit sums."""
    for vt, st in (("uint", "uint"), ("int", "long"), (None, "uint")):
        tile = tile_of(dev, "uint", vt)
        n = 9 * tile + 3
        runs = structure(struct, n, tile, seed=31)
        assert np.diff(np.flatnonzero(np.diff(np.concatenate(([-1], runs, [-2]))))).max() > 2 * tile   # a run longer than two tiles
        keys = make_keys("uint", runs, seed=9)
        for op in (("sum", "min", "max") if vt else ("sum",)):
            for inclusive in (False, True):
                run_case(dev, "uint", vt, st, op, inclusive, keys, make_values(vt, n, 32), "%s %s %s->%s inclusive=%s" % (struct, op, vt, st, inclusive))


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_and_value_sum_pairs(dev, kt):
    for i, (vt, st) in enumerate(PAIRS):
        tile = tile_of(dev, kt, vt)
        for j, (struct, n) in enumerate((("geo3", 2 * tile + 1), ("geo100", 70001), ("equal", 3 * tile - 1), ("unsorted", tile + 1))):
            keys = make_keys(kt, structure(struct, n, tile, seed=3), seed=2)
            for inclusive in ((False, True) if j == 0 else ((i + j) % 2 == 0,)):
                run_case(dev, kt, vt, st, "sum", inclusive, keys, make_values(vt, n, 5), "%s %s->%s %s n=%d inclusive=%s" % (kt, vt, st, struct, n, inclusive))


def test_float_keys_compare_by_their_bits(dev):
    """-0.0 | +0.0 and NaN | NaN with another payload are run boundaries; equal NaN bits are one run."""
    for kt, bits in (("float", np.uint32), ("double", np.uint64)):
        p = palette(_NP[kt])[:4]
        assert np.isnan(p[2]) and np.isnan(p[3]) and p[0] == p[1] and len(set(p.view(bits).tolist())) == 4
        keys = np.repeat(np.resize(p, 4000), np.random.default_rng(9).integers(1, 9, 4000))
        assert heads_of(keys).sum() == 4000
        run_case(dev, kt, None, "uint", "sum", False, keys, None, kt + " zeros and NaNs, ranks")
        run_case(dev, kt, "int", "long", "sum", True, keys, make_values("int", keys.size, 1), kt + " zeros and NaNs, values")
        run_case(dev, kt, "int", "int", "max", False, keys, make_values("int", keys.size, 1), kt + " zeros and NaNs, max")


@pytest.mark.parametrize("op", ["min", "max"])
def test_min_max(dev, op):
    """Signed and unsigned, 32- and 64-bit sums; the exclusive form holds the identity at every head."""
    for kt in ("uchar", "uint", "double"):
        for vt, st in (("int", "long"), ("uint", "uint"), ("int", "int"), ("uint", "long"), ("int", "ulong"), ("ulong", "ulong"), ("long", "long"),
                       ("uint", "int")):
            tile = tile_of(dev, kt, vt)
            for struct, n in (("geo100", 2 * tile + 1), ("equal", 2 * tile + 5), ("geo3", 70001), ("geo50000", 5 * tile + 3)):
                keys = make_keys(kt, structure(struct, n, tile, seed=4), seed=3)
                values = make_values(vt, n, 6)
                want = sbk(keys, values, op, _NP[st], False)
                assert (want[heads_of(keys)] == identity(op, _NP[st])).all() and (want != identity(op, _NP[st])).any()
                for inclusive in (False, True):
                    run_case(dev, kt, vt, st, op, inclusive, keys, values, "%s %s %s->%s %s n=%d inclusive=%s" % (op, kt, vt, st, struct, n, inclusive))


def test_sums_that_wrap(dev):
    """Full-range values in long runs: the 32-bit sums differ from the low words of nothing but their own wrap."""
    tile = tile_of(dev, "uint", "uint")
    n = 6 * tile + 1
    keys = make_keys("uint", structure("geo50000", n, tile, seed=41), seed=4)
    for vt, st in (("uint", "uint"), ("int", "int"), ("int", "uint"), ("long", "long"), ("ulong", "ulong")):
        values = make_values(vt, n, 42)
        wide = sbk(keys, values.astype(np.int64 if vt == "int" else np.uint64) if np.dtype(_NP[vt]).itemsize == 4 else values, "sum",
                   np.uint64, True)
        if np.dtype(_NP[st]).itemsize == 4:
            assert (wide >> np.uint64(32)).any()     # the sums do not fit 32 bits
            assert np.array_equal(sbk(keys, values, "sum", _NP[st], True).view(np.uint32), wide.astype(np.uint32))
        for inclusive in (False, True):
            run_case(dev, "uint", vt, st, "sum", inclusive, keys, values, "wrapping %s->%s inclusive=%s" % (vt, st, inclusive))


def test_min_max_without_values_and_overlaps_are_refused(dev):
    clo, ctx, q = dev
    from cl_ops_amd.api import CLO_ERROR_ARGS
    r = clo.ScanByKey(ctx, "uint", "uint", "uint", op="max")
    rw = clo.ScanByKey(ctx, "uint", "uint", "ulong")
    b = [clo.Buffer(ctx, 256) for _ in range(3)]
    shifted = clo.Buffer(ctx, 64, device_ptr=b[1].ptr + 4)
    before = [x.read(q, np.uint8, 256) for x in b]
    for call, word in ((lambda: r.with_device_data(q, b[0], None, b[2], 16), "min / max"),
                       (lambda: r.with_device_data(q, b[0], b[1], b[0], 16), "keys_in"),
                       (lambda: r.with_device_data(q, b[0], b[1], shifted, 16), "values_in"),
                       (lambda: rw.with_device_data(q, b[0], b[1], b[1], 16), "values_in"),
                       (lambda: r.with_device_data(q, b[0], b[1], None, 16), "data_out"),
                       (lambda: r.with_device_data(q, b[0], b[1], b[2], 65), "exceeds")):
        with pytest.raises(clo.CloError) as e:
            call()
        assert e.value.code == CLO_ERROR_ARGS and word in e.value.message, e.value
    q.finish()
    for x, was in zip(b, before):
        assert np.array_equal(x.read(q, np.uint8, 256), was)
    shifted.close()
    for x in b:
        x.close()
    r.close()
    rw.close()


@pytest.mark.parametrize("kt,vt,st", [("uchar", "uint", "uint"), ("ushort", "int", "long"), ("uint", "uint", "ulong"), ("float", "int", "int"),
                                      ("ulong", "ulong", "ulong"), ("double", "uint", "uint")])
def test_element_aligned_views(dev, kt, vt, st):
    """Views at byte offsets es and 16 - es of keys, values and out, each in turn and all at once; values NULL too."""
    ks, vs, ss = (np.dtype(_NP[t]).itemsize for t in (kt, vt, st))
    tile = tile_of(dev, kt, vt)
    n = 2 * tile + 3
    keys = make_keys(kt, structure("geo100", n, tile, seed=8), seed=4)
    values = make_values(vt, n, 9)
    o = lambda es: [es, 16 - es] if es < 8 else [8, 24]
    cases = []
    for which, es in enumerate((ks, vs, ss)):
        for off in o(es):
            c = [0, 0, 0]
            c[which] = off
            cases.append(tuple(c))
    cases.append((o(ks)[0], o(vs)[1], o(ss)[0]))
    cases.append((o(ks)[1], o(vs)[0], o(ss)[1]))
    for i, offs in enumerate(cases):
        run_case(dev, kt, vt, st, "sum", i % 2 == 1, keys, values, "%s %s->%s offsets %s" % (kt, vt, st, offs), offs=offs)
    run_case(dev, kt, vt, st, "max", False, keys, values, "max, offsets %s" % (cases[-1],), offs=cases[-1])
    run_case(dev, kt, None, st, "sum", False, keys, None, "values NULL, offsets %s" % (cases[-1],), offs=cases[-1])
    run_case(dev, kt, None, st, "sum", True, keys, None, "values NULL, offsets %s" % (cases[-2],), offs=cases[-2])


@pytest.mark.parametrize("vt", ["uint", "long"])
def test_in_place(dev, vt):
    """out == values_in for a sum type as wide as the values: aligned and element-aligned views, every op, both kinds."""
    es = np.dtype(_NP[vt]).itemsize
    for kt in ("uint", "uchar"):
        tile = tile_of(dev, kt, vt)
        for struct, n in (("geo100", 4 * tile + 5), ("geo50000", 7 * tile + 1), ("equal", 3 * tile), ("distinct", tile + 1), ("geo3", 5)):
            keys = make_keys(kt, structure(struct, n, tile, seed=17), seed=6)
            values = make_values(vt, n, 18)
            for op in ("sum", "min", "max"):
                for inclusive in (False, True):
                    for voff in (0, es if es < 8 else 8):
                        run_case(dev, kt, vt, vt, op, inclusive, keys, values, "in place %s %s %s %s n=%d inclusive=%s off=%d"
                                 % (kt, vt, op, struct, n, inclusive, voff), offs=(0, voff, 0), in_place=True)


@pytest.mark.parametrize("struct", ["equal", "distinct", "geo100", "geo50000"])
def test_2p24(dev, struct):
    n = 1 << 24
    tile = tile_of(dev, "uint", "uint")
    keys = make_keys("uint", structure(struct, n, tile, seed=11), seed=5)
    run_case(dev, "uint", "uint", "uint", "sum", False, keys, make_values("uint", n, 12), struct + " 2^24")
    run_case(dev, "uint", None, "ulong", "sum", True, keys, None, struct + " 2^24 ranks from 1")
    run_case(dev, "uint", "uint", "uint", "max", True, keys, make_values("uint", n, 12), struct + " 2^24 max")


def test_2p26_plus_5(dev):
    n = (1 << 26) + 5
    tile = tile_of(dev, "uint", "uint")
    keys = make_keys("uint", structure("geo50000", n, tile, seed=13), seed=6)
    run_case(dev, "uint", "uint", "ulong", "sum", False, keys, make_values("uint", n, 14), "geo50000 2^26+5")


def test_host_data_form(dev):
    clo, ctx, q = dev
    tile = tile_of(dev, "uint", "int")
    n = 3 * tile + 17
    keys = make_keys("uint", structure("geo100", n, tile, seed=15), seed=7)
    values = make_values("int", n, 16)
    r = clo.ScanByKey(ctx, "uint", "int", "long", op="min", inclusive=True)
    for qe in (q, None):
        got = r.with_host_data(keys, values, q_exec=qe)
        assert got.dtype == np.int64 and np.array_equal(got, sbk(keys, values, "min", np.int64, True))
    assert r.with_host_data(keys[:0], values[:0]).size == 0
    r.close()
    r = clo.ScanByKey(ctx, "uint", "int", "int")
    got = r.with_host_data(keys, values)
    assert np.array_equal(got, sbk(keys, values, "sum", np.int32))
    mine = values.copy()
    assert r.with_host_data(keys, mine, out=mine) is mine and np.array_equal(mine, got)     # in place
    r.close()
    r = clo.ScanByKey(ctx, "float")
    k = np.array([0.0, -0.0, -0.0, 1.5], np.float32)
    assert list(r.with_host_data(k)) == [0, 0, 1, 0]
    r.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 elements; the transfers on a queue of their own, then no queue at all (the call makes and destroys
    one); into a new array and in place, where the values' device buffer is the output too."""
    clo, ctx, q = dev
    tile = tile_of(dev, "uint", "int")
    n = 2 * tile + 1
    keys = make_keys("uint", structure("geo100", n, tile, seed=25), seed=8)
    values = make_values("int", n, 26)
    want = sbk(keys, values, "sum", np.int32)
    r = clo.ScanByKey(ctx, "uint", "int", "int")
    qc = clo.Queue(ctx)
    try:
        for qe, qcomm in ((q, qc), (None, None)):
            assert np.array_equal(r.with_host_data(keys, values, q_exec=qe, q_comm=qcomm), want), (qe is None, qcomm is None)
            mine = values.copy()
            assert r.with_host_data(keys, mine, q_exec=qe, q_comm=qcomm, out=mine) is mine and np.array_equal(mine, want), (qe is None, qcomm is None)
    finally:
        r.close()
        qc.close()


def _view(region, dtype, count):
    raw = region.base.read(region.q, np.uint8, region.host.size)
    return raw[region.at:region.at + count * np.dtype(dtype).itemsize].copy().view(dtype)


def test_sort_scan_reduce_by_key_on_one_queue(dev):
    """The pipeline this exists for, without a host wait between the calls: sort by key, the rank of every element
    in its group, running sum / min / max per group, and the groups' aggregates and sizes from reduce by key. The
    inclusive result at every run's last element is that run's aggregate."""
    clo, ctx, q = dev
    n = 1 << 22
    rng = np.random.default_rng(21)
    keys = rng.integers(0, 1000, n, dtype=np.uint32)
    values = rng.integers(0, 1 << 32, n, dtype=np.uint32)
    R = lambda data, salt: Region(dev, n * 4, 0, data, salt)
    kin, vin, ks, vs = R(keys, 0), R(values, 1), R(None, 2), R(None, 3)
    ranks, counts_k, counts, cnt0 = R(None, 2), R(None, 2), R(None, 3), Region(dev, 8, 0, None, 4)
    ops = ("sum", "min", "max")
    scans = {op: R(None, 3) for op in ops}
    aggr = {op: (R(None, 2), R(None, 3), Region(dev, 8, 0, None, 4)) for op in ops}
    s = clo.Sorter("satradix", ctx, "uint")
    ranker = clo.ScanByKey(ctx, "uint", None, "uint")
    counter = clo.ReduceByKey(ctx, "uint", None, "uint")
    scanners = {op: clo.ScanByKey(ctx, "uint", "uint", "uint", op=op, inclusive=True) for op in ops}
    reducers = {op: clo.ReduceByKey(ctx, "uint", "uint", "uint", op=op) for op in ops}
    try:
        assert s.by_key_with_device_data(q, kin.view, vin.view, ks.view, vs.view, n)
        assert ranker.with_device_data(q, ks.view, None, ranks.view, n)
        assert counter.with_device_data(q, ks.view, None, counts_k.view, counts.view, cnt0.view, n)
        for op in ops:
            assert scanners[op].with_device_data(q, ks.view, vs.view, scans[op].view, n)
            assert reducers[op].with_device_data(q, ks.view, vs.view, aggr[op][0].view, aggr[op][1].view, aggr[op][2].view, n)
        q.finish()
        order = np.argsort(keys, kind="stable")
        sk, sv = keys[order], values[order]
        ks.check(sk, "sorted keys")
        vs.check(sv, "sorted values")
        ranks.check(sbk(sk, None, "sum", np.uint32), "ranks")
        uk, m = np.unique(keys), np.unique(keys).size
        ends = np.append(np.flatnonzero(heads_of(sk))[1:], n) - 1
        got_ranks, got_counts = _view(ranks, np.uint32, n), _view(counts, np.uint32, m)
        cnt0.check(np.array([m], np.uint64), "run count")
        assert np.array_equal(got_ranks[ends] + np.uint32(1), got_counts)                # the last rank + 1 is the group's size
        assert np.array_equal(got_counts, np.bincount(keys, minlength=1000)[uk].astype(np.uint32))
        for op in ops:
            scans[op].check(sbk(sk, sv, op, np.uint32, True), "running " + op)
            wk, wa, wm = rbk(sk, sv, op, np.uint32)
            aggr[op][2].check(np.array([wm], np.uint64), op + ": run count")
            aggr[op][1].check(wa, op + ": aggregates")
            assert np.array_equal(_view(scans[op], np.uint32, n)[ends], _view(aggr[op][1], np.uint32, m)), op
        kin.check(keys, "keys_in")
        vin.check(values, "values_in")
    finally:
        for x in [s, ranker, counter] + list(scanners.values()) + list(reducers.values()):
            x.close()
        for x in [kin, vin, ks, vs, ranks, counts_k, counts, cnt0] + list(scans.values()) + [y for t in aggr.values() for y in t]:
            x.close()


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    tile = tile_of(dev, "uint", "uint")
    obj = clo.ScanByKey(ctx, "uint", "uint", "ulong", inclusive=True)
    for n, struct in (((1 << 22) + 1, "geo100"), (5, "distinct"), (tile + 1, "equal"), ((1 << 22) + 7, "geo50000"), ((1 << 23) + 3, "geo3")):
        keys = make_keys("uint", structure(struct, n, tile, seed=n), seed=8)
        run_case(dev, "uint", "uint", "ulong", "sum", True, keys, make_values("uint", n, n), "reuse n=%d %s" % (n, struct), obj=obj)
    obj.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib, CLO_HIP_EARGS, CLO_HIP_EUNSUPPORTED, CLO_HIP_EWORKSPACE
    n = 100000
    need = lib.clo_hip_scan_by_key_workspace_bytes(n)
    ws, k, v, o = (clo.Buffer(ctx, b) for b in (need + 512, n * 8, n * 8, n * 8))
    o.write(q, np.resize(np.arange(251, dtype=np.uint8), n * 8))
    before = o.read(q, np.uint8, n * 8)
    call = lambda w, wb, key_size=4, vt=5, st=5, op=0, inclusive=0, keys=k.ptr, vals=v.ptr, out=o.ptr, numel=n: lib.clo_hip_scan_by_key(
        keys, vals, out, numel, key_size, vt, st, op, inclusive, w, wb, q.stream)
    assert call(ws.ptr + 64, need) == CLO_HIP_EARGS           # the workspace: 256 bytes
    assert call(None, need) == CLO_HIP_EARGS
    assert call(ws.ptr, need, op=3) == CLO_HIP_EARGS
    assert call(ws.ptr, need, op=-1) == CLO_HIP_EARGS
    assert call(ws.ptr, need, inclusive=2) == CLO_HIP_EARGS
    assert call(ws.ptr, need, op=1, vals=None) == CLO_HIP_EARGS
    assert call(ws.ptr, need, op=2, vals=None) == CLO_HIP_EARGS
    assert call(ws.ptr, need, numel=1 << 32) == CLO_HIP_EARGS
    assert call(ws.ptr, need, keys=None) == CLO_HIP_EARGS
    assert call(ws.ptr, need, out=None) == CLO_HIP_EARGS
    assert call(ws.ptr, need, out=o.ptr + 2) == CLO_HIP_EARGS   # data arrays: aligned to their element
    assert call(ws.ptr, need - 1) == CLO_HIP_EWORKSPACE
    assert call(ws.ptr, 0) == CLO_HIP_EWORKSPACE
    for kw in (dict(key_size=3), dict(vt=9), dict(st=9), dict(st=10), dict(vt=3), dict(vt=7, st=5), dict(st=8), dict(st=11)):
        assert call(ws.ptr, need, **kw) == CLO_HIP_EUNSUPPORTED, kw
    assert call(ws.ptr, need, numel=0) == 0
    assert call(None, 0, numel=0, keys=None, vals=None, out=None) == 0
    q.finish()
    assert np.array_equal(o.read(q, np.uint8, n * 8), before)          # none of them wrote anything
    keys = make_keys("uint", structure("geo100", n, 8192, seed=1), seed=1)
    values = make_values("uint", n, 2)
    k.write(q, keys)
    v.write(q, values)
    assert call(ws.ptr, need, inclusive=1) == 0                        # and the call that is right, on the same buffers
    q.finish()
    assert np.array_equal(o.read(q, np.uint32, n), sbk(keys, values, "sum", np.uint32, True))
    for x in (ws, k, v, o):
        x.close()
