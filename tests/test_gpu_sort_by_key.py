"""Sorting by key on the MI355X (clo_sort_by_key_with_device_data / _with_host_data; satradix): every key type
against a numpy stable argsort in the sort's own key order (unsigned by bits, signed numerically, float / half in IEEE
total order with -0 < +0 and NaNs at the ends by sign), a key field inside the element, values given and NULL
(argsort), keys_out given and NULL, in place; sizes that cross every path of the sort (one launch, single-sweep
passes, chain-free passes on small and on big tiles) with CLO_RADIX_SWEEP 0 and 1 and radix 2, 4, 16, 256; stability;
2^28 pairs; the AoS pair sort and torch.sort as independent results; host data; a profiling queue; the refusal of a
run-time compiled get_key."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_NP = {"uchar": np.uint8, "char": np.int8, "ushort": np.uint16, "short": np.int16, "uint": np.uint32, "int": np.int32,
       "half": np.float16, "float": np.float32}
_INT = {1: np.int8, 2: np.int16, 4: np.int32}


def order_key(a, etype, get_key=None):
    """The key of every element as a signed integer array whose numpy order is the sort's order."""
    if get_key == "((x) & 0xffff)":
        return (a & 0xffff).astype(np.int64)
    if etype in ("half", "float"):
        x = a.view(_INT[a.itemsize]).astype(np.int64)
        mx = (1 << (8 * a.itemsize - 1)) - 1
        return np.where(x < 0, -((x & mx) + 1), x)      # sign-magnitude -> total order: -NaN < -inf < ... < -0 < +0 < ... < +NaN
    return a.astype(np.int64)


def make_keys(etype, n, seed, kind="random"):
    rng = np.random.default_rng(seed)
    dt = np.dtype(_NP[etype])
    if kind == "dups":
        bits = rng.integers(0, 3, n, dtype=np.uint32)
    elif kind == "equal":
        bits = np.full(n, 7, dtype=np.uint32)
    else:
        bits = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    a = bits.astype({1: np.uint8, 2: np.uint16, 4: np.uint32}[dt.itemsize]).view(dt)
    if etype in ("half", "float") and n:
        sp = (np.array([0, 0x8000, 0x7c00, 0xfc00, 0x7e01, 0xfe02], np.uint16).view(np.float16) if etype == "half" else
              np.array([0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc00002], np.uint32).view(np.float32))
        a[::11] = np.resize(sp, a[::11].shape)
    if kind == "sorted":
        a = a[np.argsort(order_key(a, etype), kind="stable")]
    elif kind == "reversed":
        a = a[np.argsort(order_key(a, etype), kind="stable")][::-1].copy()
    return a


def by_key(clo, ctx, q, s, keys, values, mode):
    """mode: 'full' (values in, keys out), 'argsort' (no values, keys out), 'argsort_only' (no values, no keys out),
    'inplace' (outputs are the inputs). Returns (keys out or None, values out)."""
    n = keys.size
    kin, kout = clo.Buffer(ctx, max(keys.nbytes, 16)), clo.Buffer(ctx, max(keys.nbytes, 16))
    vin, vout = clo.Buffer(ctx, max(4 * n, 16)), clo.Buffer(ctx, max(4 * n, 16))
    if n:
        kin.write(q, keys)
        vin.write(q, values)
    if mode == "inplace":
        s.by_key_with_device_data(q, kin, vin, kin, vin, n)
        kr, vr = kin, vin
    else:
        s.by_key_with_device_data(q, kin, vin if mode == "full" else None, kout if mode != "argsort_only" else None, vout, n)
        kr, vr = (kout if mode != "argsort_only" else None), vout
    q.finish()
    got_v = vr.read(q, np.uint32, n) if n else np.zeros(0, np.uint32)
    got_k = kr.read(q, keys.dtype, n) if (kr is not None and n) else (np.zeros(0, keys.dtype) if kr is not None else None)
    for b in (kin, kout, vin, vout):
        b.close()
    return got_k, got_v


def check(keys, values, etype, mode, got_k, got_v, get_key=None):
    order = np.argsort(order_key(keys, etype, get_key), kind="stable")
    want_v = values[order] if mode in ("full", "inplace") else order.astype(np.uint32)
    assert np.array_equal(got_v, want_v), mode
    if mode != "argsort_only":
        assert np.array_equal(got_k.view(np.uint8), keys[order].view(np.uint8)), mode   # bits, NaNs included


@pytest.fixture(scope="module")
def dev():
    import cl_ops_amd as clo
    ctx = clo.Context(0)
    q = clo.Queue(ctx)
    yield clo, ctx, q
    q.close()
    ctx.close()


@pytest.mark.parametrize("etype,get_key", [(t, None) for t in _NP] + [("uint", "((x) & 0xffff)")])
@pytest.mark.parametrize("n", [0, 1, 31, 8193, 70001, (1 << 20) + 3, (1 << 22) + 1])
def test_key_types(dev, etype, get_key, n):
    clo, ctx, q = dev
    keys = make_keys(etype, n, n)
    values = np.random.default_rng(n + 1).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s = clo.Sorter("satradix", ctx, etype, get_key=get_key)
    for mode in ("full", "argsort", "argsort_only", "inplace"):
        got_k, got_v = by_key(clo, ctx, q, s, keys, values, mode)
        check(keys, values, etype, mode, got_k, got_v, get_key)
    s.close()


_REF = {}


@pytest.mark.parametrize("n", [0, 1, 31, 8192, 8193, 70001, (1 << 20) + 3, (1 << 22) + 1, 1 << 25])
@pytest.mark.parametrize("radix", [2, 4, 16, 256])
@pytest.mark.parametrize("sweep", ["0", "1"])
def test_paths(dev, monkeypatch, n, radix, sweep):
    """uint keys with values and argsort over every path: CLO_RADIX_SWEEP is read when the sorter is made."""
    clo, ctx, q = dev
    monkeypatch.setenv("CLO_RADIX_SWEEP", sweep)
    if n not in _REF:
        keys = make_keys("uint", n, 7 + n)
        values = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        _REF[n] = (keys, values, np.argsort(keys, kind="stable"))
    keys, values, order = _REF[n]
    s = clo.Sorter("satradix", ctx, "uint", options="radix=%d" % radix)
    got_k, got_v = by_key(clo, ctx, q, s, keys, values, "full")
    assert np.array_equal(got_k, keys[order]) and np.array_equal(got_v, values[order])
    got_k, got_v = by_key(clo, ctx, q, s, keys, values, "argsort_only")
    assert got_k is None and np.array_equal(got_v, order.astype(np.uint32))
    s.close()


@pytest.mark.parametrize("kind", ["dups", "equal", "sorted", "reversed"])
@pytest.mark.parametrize("n", [8000, (1 << 20) + 3, (1 << 22) + 1])
@pytest.mark.parametrize("etype", ["uint", "short", "float"])
def test_stability(dev, kind, n, etype):
    clo, ctx, q = dev
    keys = make_keys(etype, n, 3, kind)
    values = np.arange(n, dtype=np.uint32)
    s = clo.Sorter("satradix", ctx, etype)
    got_k, got_v = by_key(clo, ctx, q, s, keys, values, "full")
    check(keys, values, etype, "full", got_k, got_v)
    s.close()


def test_full_size(dev):
    """2^28 uint32 keys with values, and 2^28 argsort, against torch.sort(stable=True) on the GPU."""
    import torch
    clo, ctx, q = dev
    n = 1 << 28
    g = torch.Generator(device="cuda").manual_seed(5)
    k64 = torch.randint(0, 1 << 32, (n,), device="cuda", dtype=torch.int64, generator=g)
    keys = k64.to(torch.int32)                       # the same bits as uint32
    values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
    ref = torch.sort(k64, stable=True).indices
    s = clo.Sorter("satradix", ctx, "uint")
    ko, vo, vo2 = (torch.empty_like(keys) for _ in range(3))
    torch.cuda.synchronize()
    B = lambda t: clo.Buffer(ctx, t.numel() * 4, device_ptr=t.data_ptr())
    bk, bv, bko, bvo, bvo2 = B(keys), B(values), B(ko), B(vo), B(vo2)
    s.by_key_with_device_data(q, bk, bv, bko, bvo, n)
    s.by_key_with_device_data(q, bk, None, None, bvo2, n)
    q.finish()
    assert torch.equal(ko, keys[ref]) and torch.equal(vo, values[ref])
    assert torch.equal(vo2.to(torch.int64) & 0xffffffff, ref)
    for b in (bk, bv, bko, bvo, bvo2):
        b.close()
    s.close()


def test_equals_the_aos_pair_sort(dev):
    """At 2^24: the separate-array result is the unpacked result of the existing AoS pair sort (BASELINE config 4)."""
    clo, ctx, q = dev
    n = 1 << 24
    rng = np.random.default_rng(11)
    keys = rng.integers(0, 1 << 20, n, dtype=np.uint32)     # many duplicates: stability shows
    values = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    pairs = (keys.astype(np.uint64) << np.uint64(32)) | values
    sp = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    src = clo.Buffer(ctx, pairs.nbytes)
    src.write(q, pairs)
    sp.with_device_data(q, src, None, n)
    aos = src.read(q, np.uint64, n)
    s = clo.Sorter("satradix", ctx, "uint")
    got_k, got_v = by_key(clo, ctx, q, s, keys, values, "full")
    assert np.array_equal(got_k, (aos >> np.uint64(32)).astype(np.uint32))
    assert np.array_equal(got_v, (aos & np.uint64(0xffffffff)).astype(np.uint32))
    src.close()
    sp.close()
    s.close()


@pytest.mark.parametrize("n", [5000, (1 << 20) + 3, (1 << 24) + 7])
def test_int_argsort_equals_torch(dev, n):
    import torch
    clo, ctx, q = dev
    t = torch.randint(-1000, 1000, (n,), device="cuda", dtype=torch.int32)
    idx = torch.empty_like(t)
    torch.cuda.synchronize()
    s = clo.Sorter("satradix", ctx, "int")
    bk, bi = clo.Buffer(ctx, 4 * n, device_ptr=t.data_ptr()), clo.Buffer(ctx, 4 * n, device_ptr=idx.data_ptr())
    s.by_key_with_device_data(q, bk, None, None, bi, n)
    q.finish()
    assert torch.equal(idx.to(torch.int64), torch.sort(t, stable=True).indices)
    bk.close()
    bi.close()
    s.close()


@pytest.mark.parametrize("etype,n", [("uint", 70001), ("float", (1 << 22) + 1), ("uchar", 4000)])
def test_host_data_equals_device_data(dev, etype, n):
    clo, ctx, q = dev
    keys = make_keys(etype, n, 9)
    values = np.random.default_rng(2).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    s = clo.Sorter("satradix", ctx, etype)
    dk, dv = by_key(clo, ctx, q, s, keys, values, "full")
    hk, hv = s.by_key_with_host_data(keys, values, q)
    assert np.array_equal(hk.view(np.uint8), dk.view(np.uint8)) and np.array_equal(hv, dv)
    hk, hi = s.by_key_with_host_data(keys)
    assert np.array_equal(hi, np.argsort(order_key(keys, etype), kind="stable").astype(np.uint32))
    s.close()


def test_profiling_queue_reports_the_kernels(dev):
    clo, ctx, _ = dev
    qp = clo.Queue(ctx, profiling=True)
    s = clo.Sorter("satradix", ctx, "uint")
    for n, names in (((1 << 22) + 1, {"satradix_histogram", "clo_scan_blelloch_wgscan", "satradix_scatter"}),
                     (5000, {"satradix_kv_pack", "satradix_localsort", "satradix_kv_unpack"})):
        keys = make_keys("uint", n, 1)
        kin, vout = clo.Buffer(ctx, 4 * n), clo.Buffer(ctx, 4 * n)
        kin.write(qp, keys)
        clo.Profiler(qp).duration_ns()          # (drop the copy's event)
        s.by_key_with_device_data(qp, kin, None, None, vout, n)
        prof = clo.Profiler(qp)
        assert prof.duration_ns() > 0
        agg = prof.aggregates()
        assert set(agg) == names, (n, agg)
        prof.close()
        assert np.array_equal(vout.read(qp, np.uint32, n), np.argsort(keys, kind="stable").astype(np.uint32))
        kin.close()
        vout.close()
    s.close()
    qp.close()


def test_refuses_a_run_time_compiled_get_key(dev):
    clo, ctx, q = dev
    from cl_ops_amd.api import CLO_ERROR_ARGS
    s = clo.Sorter("satradix", ctx, "uint", get_key="((x) / 65536)")    # not parseable as a shift: compiled with hiprtc
    with pytest.raises(clo.CloError) as e:
        s.by_key_with_host_data(np.arange(16, dtype=np.uint32))
    assert e.value.code == CLO_ERROR_ARGS and "get_key" in e.value.message
    s.close()
