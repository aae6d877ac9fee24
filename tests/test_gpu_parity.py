"""GPU parity tests: the HIP path, called through the C-ABI (clo_sort_* /
clo_scan_* of libcl_ops_hip.so), against the CPU oracle on the same seeded
inputs. Bit-exact equality everywhere (integer/byte work)."""
import os

import numpy as np
import pytest

import oracle_lib as O

CLO_ERROR_ARGS = 2

pytestmark = pytest.mark.gpu


def rand_u32(rng, n):
    return rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)


def rand_u64(rng, n):
    return rng.integers(0, 2**63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)


# ----------------------------------------------------------------------------
# scan
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 512, 1000, 4096, 16384, 16385, 100000, 1 << 20, (1 << 22) + 77])
@pytest.mark.parametrize("types", [("uint", "uint"), ("uint", "ulong"), ("uchar", "uint"), ("int", "long"),
                                   ("ushort", "ushort"), ("ulong", "ulong")])
def test_scan_matches_serial_scan(gpu, n, types):
    import cl_ops_amd as clo
    ctx, q = gpu
    et, st = types
    rng = np.random.default_rng(n * 7 + len(et))
    edt, sdt = clo.api.CLO_TYPE_NP[et], clo.api.CLO_TYPE_NP[st]
    info = np.iinfo(edt)
    a = rng.integers(max(info.min, -1000), min(info.max, 128) + 1, n).astype(edt)
    sc = clo.Scanner("blelloch", ctx, et, st)
    got = sc.with_host_data(a, q)
    sc.close()
    exp = O.serial_scan(a.astype(sdt) if np.issubdtype(edt, np.signedinteger) else a, sdt) \
        if np.issubdtype(edt, np.signedinteger) else O.serial_scan(a, sdt)
    assert got.dtype == sdt
    assert np.array_equal(got, exp)


@pytest.mark.parametrize("types", [("uint", "uint"), ("uint", "ulong"), ("int", "long"), ("uchar", "ushort")])
def test_scan_in_chunks_with_device_carry_and_reduce(gpu, types):
    """clo_hip_scan_exclusive_carry over uneven chunks == one scan of the whole
    array; clo_hip_reduce_sum == the carry out of the last chunk."""
    import cl_ops_amd as clo
    from cl_ops_amd import _hip
    from cl_ops_amd._hip import lib
    ctx, q = gpu
    et, st = types
    edt, sdt = clo.api.CLO_TYPE_NP[et], clo.api.CLO_TYPE_NP[st]
    rng = np.random.default_rng(42)
    n = 300000
    info = np.iinfo(edt)
    a = rng.integers(max(info.min, -100000), min(info.max, 100000), n, endpoint=True).astype(edt)
    signed = int(np.issubdtype(edt, np.signedinteger))
    src, dst = clo.Buffer(ctx, a.nbytes), clo.Buffer(ctx, n * sdt.itemsize)
    carry, total = clo.Buffer(ctx, 16), clo.Buffer(ctx, 8)
    src.write(q, a)
    carry.write(q, np.zeros(2, np.uint64))
    cuts = [0, 1, 5000, 5000, 70001, 262144, n]     # includes an empty chunk
    wsb = lib.clo_hip_scan_workspace_bytes(n, edt.itemsize, sdt.itemsize)
    ws = clo.Buffer(ctx, wsb)
    _hip.check(lib.clo_hip_scan_workspace_init(ws.ptr, wsb, q.stream), "clo_hip_scan_workspace_init")   # once per allocation
    for k in range(len(cuts) - 1):
        lo, hi = cuts[k], cuts[k + 1]
        _hip.check(lib.clo_hip_scan_exclusive_carry(src.ptr + lo * edt.itemsize, dst.ptr + lo * sdt.itemsize, hi - lo,
                                                    edt.itemsize, signed, sdt.itemsize, carry.ptr + 8 * (k & 1),
                                                    carry.ptr + 8 * ((k + 1) & 1), ws.ptr, wsb, q.stream),
                   "clo_hip_scan_exclusive_carry")
    _hip.check(lib.clo_hip_reduce_sum(src.ptr, n, edt.itemsize, signed, total.ptr, q.stream), "clo_hip_reduce_sum")
    got = dst.read(q, sdt, n)
    wide = a.astype(np.int64) if signed else a.astype(np.uint64)
    exp = np.concatenate((np.zeros(1, wide.dtype), np.cumsum(wide[:-1], dtype=wide.dtype))).astype(sdt)
    assert np.array_equal(got, exp)
    mask = np.uint64((1 << (8 * sdt.itemsize)) - 1)
    full = np.uint64(int(wide.sum(dtype=wide.dtype)) & 0xFFFFFFFFFFFFFFFF)
    assert total.read(q, np.uint64, 1)[0] == full
    assert carry.read(q, np.uint64, 2)[(len(cuts) - 1) & 1] & mask == full & mask
    for b in (src, dst, carry, total, ws):
        b.close()


@pytest.mark.parametrize("types", [("uint", "uint"), ("uint", "ulong")])
@pytest.mark.parametrize("n", [1 << 25, (1 << 25) + (1 << 23) + 12345])     # (the pipeline starts at 2^25: chunks of 2^24, a short last one)
def test_scan_host_data_pipelined_chunks(gpu, n, types):
    """numel >= 2 chunks: clo_scan_with_host_data goes through the chunked
    copy-in / scan / copy-out pipeline (helper thread for the copies out)."""
    import cl_ops_amd as clo
    ctx, q = gpu
    et, st = types
    sdt = clo.api.CLO_TYPE_NP[st]
    a = np.random.default_rng(n).integers(0, 128, n, dtype=np.uint32)
    sc = clo.Scanner("blelloch", ctx, et, st)
    for queues in ((q, None), (q, clo.Queue(ctx))):
        got = sc.with_host_data(a, queues[0], queues[1])
        exp = np.concatenate((np.zeros(1, np.uint64), np.cumsum(a[:-1], dtype=np.uint64))).astype(sdt)
        assert np.array_equal(got, exp)
        if queues[1] is not None:
            queues[1].close()
    sc.close()


def test_scan_wraps_in_sum_type(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = np.full(70000, 0xF0000000, dtype=np.uint32)
    sc = clo.Scanner("blelloch", ctx, "uint", "uint")
    got = sc.with_host_data(a, q)
    sc.close()
    assert np.array_equal(got, O.serial_scan(a, np.uint32))


def test_scan_matches_reference_decomposition(gpu):
    """3-kernel Blelloch restatement (oracle) == HIP single pass, where the
    reference scans everything (numel multiple of 2*lws)."""
    import cl_ops_amd as clo
    ctx, q = gpu
    a = O.scan_bench_rand(0, np.uint32, 1 << 18)
    sc = clo.Scanner("blelloch", ctx, "uint", "ulong")
    got = sc.with_host_data(a, q)
    sc.close()
    assert np.array_equal(got, O.blelloch(a, np.uint64, dev_max_lws=256))


# ----------------------------------------------------------------------------
# satradix
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 16, 100, 1024, 4096, 8192, 8193, 50000, 1 << 17, (1 << 20) + 3])
def test_satradix_u32_keys(gpu, n):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = rand_u32(np.random.default_rng(n), n)
    s = clo.Sorter("satradix", ctx, "uint")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a))


@pytest.mark.parametrize("n", [16, 1024, 4096, 1 << 16])
@pytest.mark.parametrize("radix", [2, 4, 16, 256])
def test_satradix_matches_reference_decomposition(gpu, n, radix):
    import cl_ops_amd as clo
    ctx, q = gpu
    if n < radix:
        pytest.skip("upstream's launch shape needs numel >= radix (clo_sort_satradix.c:190-197)")
    a = O.bench_rand(0, "uint", n)
    s = clo.Sorter("satradix", ctx, "uint", options="radix=%d" % radix)
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, O.satradix(a, radix=radix, dev_max_lws=256))


@pytest.mark.parametrize("radix", [8, 32, 64, 128])
def test_satradix_odd_digit_widths_sort_fully(gpu, radix):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = rand_u32(np.random.default_rng(radix), 30000)
    s = clo.Sorter("satradix", ctx, "uint", options="radix=%d" % radix)
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a))


@pytest.mark.parametrize("n", [1024, 4096, 70001, 1 << 19])
def test_satradix_pairs_stable(gpu, n):
    """BASELINE config 4 shape: ulong elements, uint key in the high word,
    value = original index; heavy duplication exercises stability."""
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 1000, n, dtype=np.uint64)
    e = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    got = s.with_host_data(e, q)
    s.close()
    assert np.array_equal(got, O.stable_sort(e, key_size=4, key_shift=32))
    if n <= 4096:
        assert np.array_equal(got, O.satradix(e, key_size=4, key_shift=32, dev_max_lws=256))


@pytest.mark.parametrize("n", [4096, 100000])
def test_satradix_u64_keys(gpu, n):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = rand_u64(np.random.default_rng(n), n)
    s = clo.Sorter("satradix", ctx, "ulong")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a))


@pytest.mark.parametrize("radix", [16, 256])
@pytest.mark.parametrize("et", ["uchar", "ushort", "char", "short", "int", "long"])
def test_satradix_other_integer_types(gpu, et, radix):
    """Unsigned: raw bit order. Signed: numeric order — upstream's kernels
    ignore the type and leave negative keys after the positive ones, which its
    own check rejects (SURVEY §8a-6 iii, §8f-1); non-negative inputs must give
    what upstream's decomposition gives."""
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    rng = np.random.default_rng(5)
    info = np.iinfo(dt)
    a = rng.integers(info.min, info.max, 20000, dtype=np.int64, endpoint=True).astype(dt)
    s = clo.Sorter("satradix", ctx, et, options="radix=%d" % radix)
    got = s.with_host_data(a, q)
    assert got.dtype == dt and np.array_equal(got, np.sort(a))
    ut = np.dtype("u%d" % dt.itemsize)
    nonneg = (a.view(ut) >> ut.type(1)).view(dt)[:4096].copy()    # top bit clear
    got = s.with_host_data(nonneg, q)
    s.close()
    u = nonneg.view(ut)
    assert np.array_equal(got.view(u.dtype), O.satradix(u, radix=radix, dev_max_lws=256))


@pytest.mark.parametrize("radix", [2, 16, 64, 256])
@pytest.mark.parametrize("et", ["half", "float", "double"])
def test_satradix_floating_point_keys(gpu, et, radix):
    """IEEE keys through the order-preserving transform: negatives, both
    zeros, infinities; the result must be the same multiset of bit patterns."""
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    rng = np.random.default_rng(7)
    n = 30011
    a = (rng.standard_normal(n) * 1000).astype(dt)
    a[:8] = np.array([0.0, -0.0, np.inf, -np.inf, 1.0, -1.0, np.finfo(dt).tiny, -np.finfo(dt).tiny], dtype=dt)
    s = clo.Sorter("satradix", ctx, et, options="radix=%d" % radix)
    got = s.with_host_data(a, q)
    s.close()
    u = np.dtype("u%d" % dt.itemsize)
    assert np.array_equal(np.sort(got.view(u)), np.sort(a.view(u)))          # permutation of the bit patterns
    assert np.all(got[:-1] <= got[1:])                                      # numeric order
    z = np.flatnonzero(got == 0)
    assert np.all(np.signbit(got[z])[:-1] >= np.signbit(got[z])[1:])        # -0 before +0
    # positive keys: identical to upstream's raw-bit decomposition
    pos = np.abs(a[:4096])
    s = clo.Sorter("satradix", ctx, et, options="radix=%d" % radix)
    got = s.with_host_data(pos, q)
    s.close()
    assert np.array_equal(got.view(u), np.sort(pos.view(u)))
    if (8 * dt.itemsize) % (radix.bit_length() - 1) == 0:   # (upstream drops the last partial digit otherwise)
        assert np.array_equal(got.view(u), O.satradix(pos.view(u), radix=radix, dev_max_lws=256))


def test_satradix_float_key_inside_a_wider_element(gpu):
    """float key in the high word of a ulong element (get_key), value = index: stable."""
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 50000
    rng = np.random.default_rng(9)
    k = rng.integers(-50, 50, n).astype(np.float32)
    e = (k.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter("satradix", ctx, "ulong", key_type="float", get_key="as_float((uint) ((x) >> 32))")
    try:
        got = s.with_host_data(e, q)
    except clo.CloError:
        s.close()
        pytest.skip("get_key form not recognised by the key parser")
    s.close()
    order = np.argsort(k, kind="stable")
    assert np.array_equal(got, e[order])


@pytest.mark.parametrize("radix", [32, 64, 128, 256])
@pytest.mark.parametrize("n", [1, 100, 4096, 8192, 8193, 70001, (1 << 20) + 3])
def test_satradix_wide_digits_pairs_stable(gpu, n, radix):
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(n + radix)
    keys = rng.integers(0, 5000, n, dtype=np.uint64) * np.uint64(858993)   # spread over all 32 key bits
    keys &= np.uint64(0xFFFFFFFF)
    e = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)", options="radix=%d" % radix)
    got = s.with_host_data(e, q)
    s.close()
    assert np.array_equal(got, O.stable_sort(e, key_size=4, key_shift=32))


@pytest.mark.parametrize("radix", [32, 256])
@pytest.mark.parametrize("et", ["uchar", "ushort", "uint", "ulong"])
def test_satradix_wide_digits_all_element_sizes_in_place(gpu, et, radix):
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    n = 123457
    a = np.random.default_rng(3).integers(0, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
    s = clo.Sorter("satradix", ctx, et, options="radix=%d" % radix)
    b = clo.Buffer(ctx, a.nbytes)
    b.write(q, a)
    s.with_device_data(q, b, None, n)            # in place (odd pass counts copy back)
    assert np.array_equal(b.read(q, dt, n), np.sort(a))
    bo = clo.Buffer(ctx, a.nbytes)
    b.write(q, a)
    s.with_device_data(q, b, bo, n)              # out of place: input untouched
    assert np.array_equal(bo.read(q, dt, n), np.sort(a))
    assert np.array_equal(b.read(q, dt, n), a)
    for x in (b, bo):
        x.close()
    s.close()


def test_satradix_degenerate_inputs(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    s = clo.Sorter("satradix", ctx, "uint")
    n = 20000
    for a in (np.zeros(n, np.uint32), np.full(n, 0xFFFFFFFF, np.uint32), np.arange(n, dtype=np.uint32),
              np.arange(n, dtype=np.uint32)[::-1].copy(), np.full(n, 0x30, np.uint32),
              (np.arange(n, dtype=np.uint32) % 3) << 4):
        assert np.array_equal(s.with_host_data(a, q), np.sort(a))
    s.close()


def test_satradix_device_data_in_place_and_out_of_place(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 300000
    a = rand_u32(np.random.default_rng(11), n)
    s = clo.Sorter("satradix", ctx, "uint")
    bin_, bout = clo.Buffer(ctx, a.nbytes), clo.Buffer(ctx, a.nbytes)
    bin_.write(q, a)
    s.with_device_data(q, bin_, bout, n)
    assert np.array_equal(bout.read(q, np.uint32, n), np.sort(a))
    assert np.array_equal(bin_.read(q, np.uint32, n), a)  # input untouched
    s.with_device_data(q, bin_, None, n)
    assert np.array_equal(bin_.read(q, np.uint32, n), np.sort(a))
    for b in (bin_, bout):
        b.close()
    s.close()


# ----------------------------------------------------------------------------
# bitonic
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
@pytest.mark.parametrize("n", [2, 4, 16, 32, 64, 256, 1024, 4096, 8192, 16384, 1 << 16, 1 << 18])
def test_bitonic_u32(gpu, alg, n):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = O.bench_rand(0, "uint", n)
    s = clo.Sorter(alg, ctx, "uint")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a))
    if n <= 1 << 16:
        assert np.array_equal(got, O.sbitonic(a))


@pytest.mark.parametrize("logn", [15, 19])
@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
def test_bitonic_pairs_tie_order_matches_reference_network(gpu, alg, logn):
    """Non-identity keys: tie order depends on the exact network; must equal the
    restated reference network bit for bit (2^19: 64 tiles, every strided width)."""
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 1 << logn
    rng = np.random.default_rng(3)
    keys = rng.integers(0, 50, n, dtype=np.uint64)
    e = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter(alg, ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    got = s.with_host_data(e, q)
    s.close()
    assert np.array_equal(got, O.sbitonic(e, key_size=4, key_shift=32))
    if logn <= 15:
        exp_ab, _ = O.abitonic(e, key_size=4, key_shift=32, dev_max_lws=256)
        assert np.array_equal(got, exp_ab)


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
@pytest.mark.parametrize("et", ["int", "long", "half", "float", "double", "ushort", "uchar"])
def test_bitonic_typed_compare(gpu, alg, et):
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    rng = np.random.default_rng(9)
    n = 1 << 14
    if np.issubdtype(dt, np.floating):
        a = ((rng.random(n) - 0.5) * (1e4 if et == "half" else 1e6)).astype(dt)
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, n, dtype=np.int64).astype(dt)
    s = clo.Sorter(alg, ctx, et)
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a))


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
def test_bitonic_float_key_inside_a_wider_element(gpu, alg):
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 1 << 13
    k = ((np.random.default_rng(4).random(n) - 0.5) * 1e3).astype(np.float32)
    e = (k.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter(alg, ctx, "ulong", key_type="float", get_key="as_float((uint) ((x) >> 32))")
    got = s.with_host_data(e, q)
    s.close()
    gk = (got >> np.uint64(32)).astype(np.uint32).view(np.float32)
    assert np.all(gk[:-1] <= gk[1:]) and np.array_equal(np.sort(got), np.sort(e))


@pytest.mark.parametrize("n", [5000, 1 << 16, (1 << 20) + 7])
def test_satradix_repeated_calls_changing_buffers_and_sizes(gpu, n):
    """Repeated calls on the same and on changing buffers, in place / out of
    place, with a different size in between (the cached aux buffers and
    workspace are reused across all of them)."""
    import cl_ops_amd as clo
    ctx, q = gpu
    s = clo.Sorter("satradix", ctx, "uint")
    b1, b2, b3 = (clo.Buffer(ctx, 4 * n) for _ in range(3))
    rng = np.random.default_rng(n)
    plan = [(b1, b2, n)] * 4 + [(b1, None, n)] * 3 + [(b3, b2, n)] * 3 + [(b1, b2, n // 2)] * 3 + [(b1, b2, n)] * 3
    for src, dst, m in plan:
        a = rand_u32(rng, m)
        src.write(q, a)
        s.with_device_data(q, src, dst, m)
        assert np.array_equal((dst or src).read(q, np.uint32, m), np.sort(a))
        if dst is not None:
            assert np.array_equal(src.read(q, np.uint32, m), a)
    for b in (b1, b2, b3):
        b.close()
    s.close()


def test_sbitonic_graph_replay_sees_new_data_and_new_buffers(gpu, monkeypatch):
    """The one-launch-per-step schedule (CLO_SBITONIC_STEPS=1; sbitonic's default is the tiled
    schedule): from the third call with the same (buffer, numel, queue) on it
    replays its 136 launches from a captured graph: new contents, another
    buffer, another size and a profiling run in between must all come out sorted."""
    import cl_ops_amd as clo
    from cl_ops_amd._hip import lib
    ctx, q = gpu
    monkeypatch.setenv("CLO_SBITONIC_STEPS", "1")
    n = 1 << 16
    s = clo.Sorter("sbitonic", ctx, "uint")
    b1, b2 = clo.Buffer(ctx, 4 * n), clo.Buffer(ctx, 4 * n)
    rng = np.random.default_rng(77)
    for rep in range(5):                       # calls 3.. replay the graph
        a = rand_u32(rng, n)
        b1.write(q, a)
        s.with_device_data(q, b1, None, n)
        assert np.array_equal(b1.read(q, np.uint32, n), np.sort(a)), rep
    for buf, m in ((b2, n), (b2, n), (b2, n), (b1, n >> 1), (b1, n >> 1), (b1, n >> 1), (b1, n)):
        a = rand_u32(rng, m)
        buf.write(q, a)
        s.with_device_data(q, buf, None, m)
        assert np.array_equal(buf.read(q, np.uint32, m), np.sort(a))
    lib.clo_hip_timing_enable(1)               # per-kernel timing needs real launches
    lib.clo_hip_timing_reset()
    for _ in range(2):
        a = rand_u32(rng, n)
        b1.write(q, a)
        s.with_device_data(q, b1, None, n)
        assert np.array_equal(b1.read(q, np.uint32, n), np.sort(a))
    from cl_ops_amd import _hip
    assert _hip.timing_read("bitonic_step")[0] == 2 * 136
    lib.clo_hip_timing_enable(0)
    lib.clo_hip_timing_reset()
    for b in (b1, b2):
        b.close()
    s.close()


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
def test_bitonic_descending_compare(gpu, alg):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = rand_u32(np.random.default_rng(2), 1 << 13)
    s = clo.Sorter(alg, ctx, "uint", compare="((a) < (b))")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a)[::-1])
    assert np.array_equal(got, O.sbitonic(a, descending=True))


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("et", ["uint", "int", "float", "ushort", "uchar", "long", "ulong", "double"])
def test_abitonic_many_tiles_typed_and_descending(gpu, et, descending):
    """2^17 elements = 8 (16 for 8-byte types) full tiles: the compile-time-schedule
    presort (complement state for integer keys), the strided passes and the tile
    merges, for every compare mode and both directions."""
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    rng = np.random.default_rng(17)
    n = 1 << 17
    if np.issubdtype(dt, np.floating):
        a = ((rng.random(n) - 0.5) * 1e6).astype(dt)
    else:
        info = np.iinfo(dt)
        if dt == np.uint64:
            a = rng.integers(0, info.max, n, dtype=np.uint64, endpoint=True)
        else:
            a = rng.integers(info.min, info.max, n, dtype=np.int64, endpoint=True).astype(dt)
    s = clo.Sorter("abitonic", ctx, et, compare="((a) < (b))" if descending else None)
    got = s.with_host_data(a, q)
    s.close()
    exp = np.sort(a)
    assert np.array_equal(got, exp[::-1] if descending else exp)


def test_abitonic_general_keys_tie_order_at_2p21(gpu):
    """General keys over 128+ tiles: every strided width and the two-level strided
    passes, tie order bit for bit the restated reference network's."""
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 1 << 21
    a = rand_u32(np.random.default_rng(21), n)
    s = clo.Sorter("abitonic", ctx, "uint", get_key="((x) >> 20)")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, O.sbitonic(a, key_shift=20))
    keys = np.random.default_rng(1).integers(0, 1000, n, dtype=np.uint64)
    e = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter("abitonic", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    got = s.with_host_data(e, q)
    s.close()
    assert np.array_equal(got, O.sbitonic(e, key_size=4, key_shift=32))


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic", "satradix"])
@pytest.mark.parametrize("et", ["float", "double", "half"])
def test_float_keys_follow_the_ieee_total_order(gpu, alg, et):
    """Floating-point keys are ordered by the total order of their bit patterns
    (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN) in every sorter: the same
    image the radix passes sort by. Upstream's `>` ties -0 with +0 and is
    undefined with NaNs; without NaNs the two orders agree as values."""
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    ut = np.dtype("u%d" % dt.itemsize)
    rng = np.random.default_rng(5)
    n = 1 << 15
    a = ((rng.random(n) - 0.5) * 1e4).astype(dt)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0], dtype=dt)
    a[rng.integers(0, n, 4000)] = special[rng.integers(0, special.size, 4000)]
    u = a.view(ut)
    sign = ut.type(1) << ut.type(8 * dt.itemsize - 1)
    image = np.where(u & sign, ~u, u | sign)
    s = clo.Sorter(alg, ctx, et)
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got.view(ut), u[np.argsort(image, kind="stable")])


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
@pytest.mark.parametrize("n", [3, 100, 5000, 70000])
def test_bitonic_non_power_of_two(gpu, alg, n):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = rand_u32(np.random.default_rng(n), n)
    a[: n // 3] = 0xFFFFFFFF  # real elements equal to the pad value
    s = clo.Sorter(alg, ctx, "uint")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, np.sort(a))


# ----------------------------------------------------------------------------
# API surface on a live device
# ----------------------------------------------------------------------------

def test_profiler_reports_exec_queue_time(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = rand_u32(np.random.default_rng(0), 1 << 20)
    s = clo.Sorter("satradix", ctx, "uint")
    q.gc()
    s.with_host_data(a, q)
    prof = clo.Profiler(q)
    ns = prof.duration_ns()
    prof.close()
    s.close()
    assert 1000 < ns < 5e9


def test_host_data_copies_carry_their_names_on_a_profiling_transfer_queue(gpu):
    """The blocking host-data calls name their copies for a CCLProf consumer: upstream's names for a sort and a scan,
    the buffer calls' own for a sort by key (tests/hoststub/host_paths_test.c checks the same over the host stub)."""
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 4099
    rng = np.random.default_rng(5)
    keys = rand_u32(rng, n)
    qc = clo.Queue(ctx, profiling=True)
    prof = clo.Profiler(qc)

    def names():
        assert prof.duration_ns() > 0
        return set(prof.aggregates())

    s = clo.Sorter("satradix", ctx, "uint")
    assert np.array_equal(s.with_host_data(keys, q, qc), np.sort(keys))
    assert names() == {"clo_sort_write", "clo_sort_read"}
    order = np.argsort(keys, kind="stable").astype(np.uint32)
    ko, vo = s.by_key_with_host_data(keys, np.arange(n, dtype=np.uint32), q, qc)
    assert np.array_equal(ko, keys[order]) and np.array_equal(vo, order)
    assert names() == {"write_buffer", "read_buffer"}
    s.close()
    small = (keys & np.uint32(127))
    sc = clo.Scanner("blelloch", ctx, "uint", "ulong")
    assert np.array_equal(sc.with_host_data(small, q, qc), O.serial_scan(small, np.uint64))
    assert names() == {"clo_scan_write", "clo_scan_read"}
    sc.close()
    prof.close()
    qc.close()


# ----------------------------------------------------------------------------
# MSD bucket split used by the multi-GPU exchange (C-ABI: clo_hip_msd_*)
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [1, 2, 3])
@pytest.mark.parametrize("dt", [np.uint32, np.uint64])
def test_msd_histogram_and_partition(gpu, bits, dt):
    import ctypes as C
    import cl_ops_amd as clo
    from cl_ops_amd import _hip
    from cl_ops_amd._hip import lib
    ctx, q = gpu
    n = 200003
    a = rand_u32(np.random.default_rng(bits), n) if dt == np.uint32 else rand_u64(np.random.default_rng(bits), n)
    es, kb = a.dtype.itemsize, 8 * a.dtype.itemsize
    src, dst = clo.Buffer(ctx, a.nbytes), clo.Buffer(ctx, a.nbytes)
    cnt = clo.Buffer(ctx, 8 << bits)
    ws_bytes = lib.clo_hip_msd_workspace_bytes(n, es, bits)
    ws = clo.Buffer(ctx, ws_bytes)
    src.write(q, a)
    cnt2 = clo.Buffer(ctx, 8 << bits)
    _hip.check(lib.clo_hip_msd_histogram(src.ptr, n, es, 0, kb, bits, cnt.ptr, q.stream))
    _hip.check(lib.clo_hip_msd_partition(src.ptr, dst.ptr, n, es, 0, kb, bits, cnt2.ptr, ws.ptr, ws_bytes, q.stream))
    bucket = (a >> a.dtype.type(kb - bits)).astype(np.int64)
    assert np.array_equal(cnt.read(q, np.uint64, 1 << bits), np.bincount(bucket, minlength=1 << bits).astype(np.uint64))
    assert np.array_equal(cnt2.read(q, np.uint64, 1 << bits), np.bincount(bucket, minlength=1 << bits).astype(np.uint64))
    cnt2.close()
    assert np.array_equal(dst.read(q, a.dtype, n), a[np.argsort(bucket, kind="stable")])
    assert lib.clo_hip_check_status(ws.ptr, q.stream) == 0
    for b in (src, dst, cnt, ws):
        b.close()


def test_sharded_sorter_world_size_one_uses_the_hip_ops(gpu):
    import torch
    from cl_ops_amd.multigpu import HipLocalOps, ShardedSorter
    a = rand_u32(np.random.default_rng(1), 1 << 18)
    t = torch.from_numpy(a.view(np.int32).copy()).cuda()
    ops = HipLocalOps("uint", 0)
    out, m = ShardedSorter(ops).sort(t)
    torch.cuda.synchronize()
    assert m == a.size and np.array_equal(out.cpu().numpy().view(np.uint32), np.sort(a))
    ops.close()


# ----------------------------------------------------------------------------
# BASELINE.json's full sizes, through size-independent properties
# ----------------------------------------------------------------------------

def _xor_sum(a):
    return int(np.bitwise_xor.reduce(a)), int(a.sum(dtype=np.uint64))


@pytest.mark.parametrize("path", ["library's choice", "chain-free pair passes", "single-sweep passes"])
def test_full_size_satradix_u32_2p28(gpu, monkeypatch, path):
    import cl_ops_amd as clo
    ctx, q = gpu
    if path != "library's choice":   # (read by the library at every call)
        monkeypatch.setenv("CLO_RADIX_SWEEP", "1" if path == "single-sweep passes" else "0")
    n = 1 << 28
    a = np.random.default_rng(28).integers(0, 1 << 32, n, dtype=np.uint32)
    s = clo.Sorter("satradix", ctx, "uint")
    src, dst = clo.Buffer(ctx, a.nbytes), clo.Buffer(ctx, a.nbytes)
    src.write(q, a)
    s.with_device_data(q, src, dst, n)
    got = dst.read(q, np.uint32, n)
    assert bool(np.all(got[:-1] <= got[1:]))                 # the reference's own check
    assert _xor_sum(got) == _xor_sum(a)                      # same multiset (checksum of checksums)
    # exact equality with the CPU sort on a contiguous sample of the rank space
    assert np.array_equal(got[: 1 << 20], np.sort(a[a <= got[(1 << 20) - 1]])[: 1 << 20])
    s.with_device_data(q, dst, None, n)                      # idempotence, in place
    assert np.array_equal(dst.read(q, np.uint32, n), got)
    for b in (src, dst):
        b.close()
    s.close()


@pytest.mark.parametrize("path", ["library's choice", "chain-free pair passes", "single-sweep passes"])
def test_full_size_satradix_pairs_2p28(gpu, monkeypatch, path):
    """Config 4: 2^28 (uint key, uint value) pairs; stable == values increase inside equal-key runs."""
    import cl_ops_amd as clo
    ctx, q = gpu
    if path != "library's choice":
        monkeypatch.setenv("CLO_RADIX_SWEEP", "1" if path == "single-sweep passes" else "0")
    n = 1 << 28
    keys = np.random.default_rng(4).integers(0, 1 << 26, n, dtype=np.uint64)   # ~4 duplicates per key
    a = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    del keys
    s = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    src = clo.Buffer(ctx, a.nbytes)
    src.write(q, a)
    chk = _xor_sum(a)
    del a
    s.with_device_data(q, src, None, n)
    got = src.read(q, np.uint64, n)
    k, v = got >> np.uint64(32), got & np.uint64(0xFFFFFFFF)
    assert bool(np.all(k[:-1] <= k[1:]))
    assert bool(np.all((k[:-1] != k[1:]) | (v[:-1] < v[1:])))   # stability
    assert _xor_sum(got) == chk
    src.close()
    s.close()


def test_full_size_scan_2p26(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 1 << 26
    a = O.scan_bench_rand(0, np.uint32, 1 << 20)
    a = np.tile(a, n >> 20)
    for st, sdt in (("uint", np.uint32), ("ulong", np.uint64)):
        sc = clo.Scanner("blelloch", ctx, "uint", st)
        got = sc.with_host_data(a, q)
        sc.close()
        assert got[0] == 0
        assert np.array_equal(np.diff(got.astype(np.uint64)).astype(np.uint32), a[:-1])   # out[i+1]-out[i] == in[i]
        assert int(got[-1]) + int(a[-1]) == int(a.sum(dtype=np.uint64)) % (1 << (8 * np.dtype(sdt).itemsize))


def test_full_size_abitonic_2p26(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 1 << 26
    a = np.random.default_rng(26).integers(0, 1 << 32, n, dtype=np.uint32)
    s = clo.Sorter("abitonic", ctx, "uint")
    got = s.with_host_data(a, q)
    s.close()
    assert bool(np.all(got[:-1] <= got[1:])) and _xor_sum(got) == _xor_sum(a)


@pytest.mark.parametrize("radix", [2, 16, 64, 256])
def test_satradix_large_degenerate_keys_keep_input_order(gpu, radix):
    """2^22 (key, index) pairs whose keys are all equal / take two values: every
    digit histogram has one or two huge bins; a stable sort returns the input
    order inside each key."""
    import cl_ops_amd as clo
    ctx, q = gpu
    n = (1 << 22) + 321
    idx = np.arange(n, dtype=np.uint64)
    s = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)", options="radix=%d" % radix)
    same = (np.uint64(0xA5A5A5A5) << np.uint64(32)) | idx
    assert np.array_equal(s.with_host_data(same, q), same)
    two = (np.where(idx % 3 == 0, np.uint64(0xFFFFFFFF), np.uint64(0)) << np.uint64(32)) | idx
    assert np.array_equal(s.with_host_data(two, q), O.stable_sort(two, key_size=4, key_shift=32))
    s.close()


@pytest.mark.parametrize("et,radix", [("float", 16), ("int", 256), ("double", 64)])
def test_full_size_typed_radix_keys_2p26(gpu, et, radix):
    """2^26 signed / IEEE keys (negatives included) through the transform in the
    first and last pass: numeric order, same multiset of bit patterns, idempotent."""
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    n = 1 << 26
    rng = np.random.default_rng(26)
    if np.issubdtype(dt, np.floating):
        a = (rng.standard_normal(n) * 1e3).astype(dt)
    else:
        a = rng.integers(-2**31, 2**31 - 1, n, dtype=np.int64).astype(dt)
    s = clo.Sorter("satradix", ctx, et, options="radix=%d" % radix)
    buf = clo.Buffer(ctx, a.nbytes)
    buf.write(q, a)
    s.with_device_data(q, buf, None, n)
    got = buf.read(q, dt, n)
    u = np.dtype("u%d" % dt.itemsize)
    assert bool(np.all(got[:-1] <= got[1:]))
    assert _xor_sum(got.view(u)) == _xor_sum(a.view(u))
    s.with_device_data(q, buf, None, n)
    assert np.array_equal(buf.read(q, dt, n).view(u), got.view(u))
    buf.close()
    s.close()


def test_indices_above_2p31_satradix_and_scan(gpu):
    """3*2^30 + 5 elements: global indices use bit 31 (positions are 32-bit, as
    upstream's uint gid; numel < 2^32). Inputs are generated and the results
    checked on the device (torch) so that the host never holds the 12 GiB."""
    import torch
    import cl_ops_amd as clo
    ctx, q = gpu
    if torch.cuda.get_device_properties(0).total_memory < (96 << 30):
        pytest.skip("needs ~60 GiB of device memory")
    n = 3 * (1 << 30) + 5
    g = torch.Generator(device="cuda").manual_seed(31)
    a = torch.randint(-(1 << 31), 1 << 31, (n,), dtype=torch.int32, device="cuda", generator=g)
    sum_in = int(a.sum(dtype=torch.int64))
    sq_in = int((a.to(torch.int64) * 0x9E3779B1).bitwise_and(0xFFFFFFFF).sum())
    torch.cuda.synchronize()
    buf = clo.Buffer(ctx, n * 4, device_ptr=a.data_ptr())
    s = clo.Sorter("satradix", ctx, "uint")
    s.with_device_data(q, buf, None, n)
    q.finish()
    b = a ^ (-(1 << 31))                         # unsigned order as signed order
    assert bool((b[1:] >= b[:-1]).all())
    del b
    assert int(a.sum(dtype=torch.int64)) == sum_in
    assert int((a.to(torch.int64) * 0x9E3779B1).bitwise_and(0xFFFFFFFF).sum()) == sq_in
    s.close()
    # scan of ones-and-twos into uint sums: out[i] = (sum of a[:i]) mod 2^32
    a.copy_((a & 1) + 1)
    out = torch.empty_like(a)
    torch.cuda.synchronize()
    bout = clo.Buffer(ctx, n * 4, device_ptr=out.data_ptr())
    sc = clo.Scanner("blelloch", ctx, "uint", "uint")
    sc.with_device_data(q, buf, bout, n)
    q.finish()
    assert int(out[0]) == 0
    d = out[1:] - out[:-1]                       # wraps like the sum type
    assert bool((d == a[:-1]).all())
    assert (int(out[-1]) + int(a[-1])) % (1 << 32) == int(a.sum(dtype=torch.int64)) % (1 << 32)
    sc.close()
    for x in (buf, bout):
        x.close()


# ----------------------------------------------------------------------------
# two ranks sharing the one GPU of this box: HipLocalOps end to end. RCCL
# refuses two ranks on one device, so this test (and only this test) stages the
# exchange through host memory over gloo; everything else is the product path.
# ----------------------------------------------------------------------------

def _two_rank_worker(rank, world, port, n, out_dir):
    import torch
    import torch.distributed as dist
    from cl_ops_amd.multigpu import HipLocalOps, ShardedSorter

    class HostStaged(ShardedSorter):
        def exchange(self, send, recv, sc, so, rc, ro):
            hs, hr = send.cpu(), torch.empty(recv.numel(), dtype=recv.dtype)
            r = self.rank
            hr[ro[r]:ro[r] + rc[r]] = hs[so[r]:so[r] + sc[r]]
            ops = []
            for k in range(1, self.world):
                dst, src = (r + k) % self.world, (r - k) % self.world
                if sc[dst] > 0:
                    ops.append(dist.P2POp(dist.isend, hs[so[dst]:so[dst] + sc[dst]].contiguous(), dst))
                if rc[src] > 0:
                    ops.append(dist.P2POp(dist.irecv, hr[ro[src]:ro[src] + rc[src]], src))
            for w in dist.batch_isend_irecv(ops):
                w.wait()
            recv.copy_(hr)

    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        a = np.random.default_rng(50 + rank).integers(0, 1 << 32, n, dtype=np.uint32)
        local = torch.from_numpy(a.view(np.int32).copy()).cuda()
        ops = HipLocalOps("uint", 0)
        out, m = HostStaged(ops).sort(local, n)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, "in_%d.npy" % rank), a)
        np.save(os.path.join(out_dir, "out_%d.npy" % rank), out[:m].cpu().numpy().view(np.uint32))
        assert np.array_equal(local.cpu().numpy().view(np.uint32), a)   # the shard is only read
        ops.close()
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_two_ranks_on_one_gpu_hip_ops_end_to_end(gpu, tmp_path):
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_two_rank_worker, args=(2, port, 300000, str(tmp_path)), nprocs=2, join=True)
    ins = [np.load(tmp_path / ("in_%d.npy" % r)) for r in range(2)]
    outs = [np.load(tmp_path / ("out_%d.npy" % r)) for r in range(2)]
    assert np.array_equal(np.concatenate(outs), np.sort(np.concatenate(ins)))
    assert np.all(outs[0] >> 31 == 0) and np.all(outs[1] >> 31 == 1)


def _two_rank_scan_worker(rank, world, port, n, out_dir):
    import torch
    import torch.distributed as dist
    from cl_ops_amd.multigpu import HipScanOps, ShardedScanner
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % port, rank=rank, world_size=world)
    try:
        a = np.random.default_rng(60 + rank).integers(0, 1 << 32, n + 17 * rank, dtype=np.uint32)
        local = torch.from_numpy(a.view(np.int32).copy()).cuda()
        out = torch.empty(a.size, dtype=torch.int64, device="cuda")
        ShardedScanner(HipScanOps("uint", "ulong", 0)).scan(local, out, a.size)
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, "in_%d.npy" % rank), a)
        np.save(os.path.join(out_dir, "out_%d.npy" % rank), out.cpu().numpy().view(np.uint64))
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_sharded_scan_two_ranks_on_one_gpu(gpu, tmp_path):
    """uint -> ulong scan over two pieces; the only exchange is the 8-byte all-gather of the sums."""
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_two_rank_scan_worker, args=(2, port, 1 << 20, str(tmp_path)), nprocs=2, join=True)
    a = np.concatenate([np.load(tmp_path / ("in_%d.npy" % r)) for r in range(2)])
    got = np.concatenate([np.load(tmp_path / ("out_%d.npy" % r)) for r in range(2)])
    assert np.array_equal(got, O.serial_scan(a, np.uint64))


def test_sharded_scanner_world_size_one(gpu):
    import torch
    from cl_ops_amd.multigpu import HipScanOps, ShardedScanner
    a = np.random.default_rng(1).integers(0, 128, 100001, dtype=np.uint32)
    local = torch.from_numpy(a.view(np.int32).copy()).cuda()
    out = torch.empty(a.size, dtype=torch.int32, device="cuda")
    ShardedScanner(HipScanOps("uint", "uint", 0)).scan(local, out)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), O.serial_scan(a, np.uint32))


# ----------------------------------------------------------------------------
# the committed golden vectors (tests/golden/make_golden.py) through the HIP path
# ----------------------------------------------------------------------------

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sortscan_golden.npz"))


def test_golden_vectors_through_the_hip_path(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    sorters = {}

    def sorter(alg, et, **kw):
        key = (alg, et, tuple(sorted(kw.items())))
        if key not in sorters:
            sorters[key] = clo.Sorter(alg, ctx, et, **kw)
        return sorters[key]

    checked = 0
    for name in GOLD.files:
        if name.startswith("sort_") and name.endswith("_in"):
            a, exp = GOLD[name], GOLD[name[:-3] + "_out"]
            et = "uint" if a.dtype == np.uint32 else "ulong"
            for alg in ("satradix", "sbitonic", "abitonic", "gselect"):
                if alg == "gselect" and a.size > 1024:
                    continue
                assert np.array_equal(sorter(alg, et).with_host_data(a, q), exp), (name, alg)
                checked += 1
        elif name.startswith("pairs_") and name.endswith("_in"):
            a = GOLD[name]
            kw = dict(key_type="uint", get_key="(uint) ((x) >> 32)")
            assert np.array_equal(sorter("satradix", "ulong", **kw).with_host_data(a, q), GOLD[name[:-3] + "_out"]), name
            for alg in ("sbitonic", "abitonic"):      # tie order = the reference network's
                assert np.array_equal(sorter(alg, "ulong", **kw).with_host_data(a, q), GOLD[name[:-3] + "_bitonic_out"]), (name, alg)
            checked += 3
        elif name.startswith("gselect_pairs_") and name.endswith("_in"):
            kw = dict(key_type="uint", get_key="(uint) ((x) >> 32)")
            for alg in ("gselect", "satradix"):
                assert np.array_equal(sorter(alg, "ulong", **kw).with_host_data(GOLD[name], q), GOLD[name[:-3] + "_out"]), (name, alg)
            checked += 2
        elif name.startswith("typed_") and name.endswith("_in"):
            a, exp = GOLD[name], GOLD[name[:-3] + "_out"]
            et = {"int32": "int", "float32": "float", "float64": "double"}[a.dtype.name]
            for alg in ("satradix", "sbitonic", "abitonic", "gselect"):
                got = sorter(alg, et).with_host_data(a, q)
                assert np.array_equal(got, exp), (name, alg)      # numeric equality
                checked += 1
        elif name.startswith("scan_") and name.endswith("_in"):
            a = GOLD[name]
            tag = name[:-3]
            if tag.startswith("scan_wrap"):
                sc = clo.Scanner("blelloch", ctx, "uint", "uint")
                assert np.array_equal(sc.with_host_data(a, q), GOLD[tag + "_out"]), name
                sc.close()
                checked += 1
            else:
                n = tag.split("_")[1]
                for st, t in (("uint", "u32"), ("ulong", "u64")):
                    sc = clo.Scanner("blelloch", ctx, "uint", st)
                    assert np.array_equal(sc.with_host_data(a, q), GOLD["scan_%s_%s_out" % (t, n)]), (name, st)
                    sc.close()
                    checked += 1
    assert np.array_equal(sorter("satradix", "uint").with_host_data(GOLD["structural_in"], q), GOLD["structural_out"])
    for s_ in sorters.values():
        s_.close()
    assert checked >= 140


# ----------------------------------------------------------------------------
# gselect: upstream's O(n^2) rank sort
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 2, 255, 256, 2048, 2049, 5000])
def test_gselect_matches_reference_kernel(gpu, n):
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(n)
    keys = rng.integers(0, 50, n, dtype=np.uint64)
    e = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    s = clo.Sorter("gselect", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    got = s.with_host_data(e, q)
    s.close()
    assert np.array_equal(got, O.gselect(e, key_size=4, key_shift=32))      # restated kernel
    assert np.array_equal(got, O.stable_sort(e, key_size=4, key_shift=32))  # = a stable sort


@pytest.mark.parametrize("et", ["uint", "int", "float", "short", "ulong"])
@pytest.mark.parametrize("compare", [None, "((a) < (b))"])
def test_gselect_types_and_descending(gpu, et, compare):
    import cl_ops_amd as clo
    ctx, q = gpu
    dt = clo.api.CLO_TYPE_NP[et]
    rng = np.random.default_rng(3)
    n = 3000
    if np.issubdtype(dt, np.floating):
        a = ((rng.random(n) - 0.5) * 100).astype(dt)
        a[:4] = [0.0, -0.0, 1.0, -1.0]
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    s = clo.Sorter("gselect", ctx, et, compare=compare)
    got = s.with_host_data(a, q)
    kind = O.KEY_FLOAT if np.issubdtype(dt, np.floating) else (O.KEY_SIGNED if np.issubdtype(dt, np.signedinteger) else O.KEY_UNSIGNED)
    exp = O.gselect(a, key_kind=kind, descending=compare is not None)
    u = np.dtype("u%d" % dt.itemsize)
    assert np.array_equal(got.view(u), exp.view(u))
    s.close()


def test_gselect_device_data_with_and_without_output_buffer(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    n = 10000
    a = rand_u32(np.random.default_rng(8), n)
    s = clo.Sorter("gselect", ctx, "uint")
    bin_, bout = clo.Buffer(ctx, a.nbytes), clo.Buffer(ctx, a.nbytes)
    bin_.write(q, a)
    s.with_device_data(q, bin_, bout, n)
    assert np.array_equal(bout.read(q, np.uint32, n), np.sort(a))
    assert np.array_equal(bin_.read(q, np.uint32, n), a)
    s.with_device_data(q, bin_, None, n)          # upstream: temporary + copy back (clo_sort_gselect.c:83-127)
    assert np.array_equal(bin_.read(q, np.uint32, n), np.sort(a))
    q2 = clo.Queue(ctx)
    bin_.write(q, a)
    q.finish()
    s.with_device_data(q, bin_, None, n, q_comm=q2)
    q2.finish()
    assert np.array_equal(bin_.read(q, np.uint32, n), np.sort(a))
    with pytest.raises(clo.CloError):
        s.with_device_data(q, bin_, bin_, n)
    for b in (bin_, bout):
        b.close()
    q2.close()
    s.close()


# ----------------------------------------------------------------------------
# compare / get_key outside the ahead-of-time family: compiled at run time
# (hiprtc), as upstream compiles every sorter by OpenCL JIT
# ----------------------------------------------------------------------------

@pytest.mark.parametrize("case", [
    ("uint", "uint", "(x) % 1000u", lambda a: a % 1000),
    ("uint", "uint", "((x) >> 3) * 7u", lambda a: ((a >> 3) * 7) & 0xFFFFFFFF),
    ("uint", "int", "(int) (x) / 2 - 1000", lambda a: (a.view(np.int32) / 2).astype(np.int32) - 1000),   # C division truncates
    ("ulong", "ushort", "(ushort) (((x) >> 7) ^ (x))", lambda a: ((a >> 7) ^ a).astype(np.uint16)),
    ("uint", "float", "(float) (x) * -0.5f", lambda a: a.astype(np.float32) * np.float32(-0.5)),
    ("float", "float", "fabsf(x)", lambda a: np.abs(a)),
    # 8-byte keys: two rounds (low half, then high half of the key in the first round's order)
    ("ulong", "ulong", "(x) * 0x9E3779B97F4A7C15ul", lambda a: a * np.uint64(0x9E3779B97F4A7C15)),
    ("ulong", "long", "(long) ((x) << 40) - 12345", lambda a: (a << np.uint64(40)).view(np.int64) - np.int64(12345)),
    ("uint", "double", "(double) (x) * -1.5 + 1e12", lambda a: a.astype(np.float64) * -1.5 + 1e12),
])
@pytest.mark.parametrize("n", [1000, 100003])
def test_satradix_jit_get_key(gpu, case, n):
    """get_key expressions outside the parsed family: compiled at run time, the
    key materialised, result = stable sort by the computed key (upstream: OpenCL
    JIT of the same macro body, clo_sort_abstract.c:144-179)."""
    import cl_ops_amd as clo
    ctx, q = gpu
    et, kt, expr, fn = case
    dt = clo.api.CLO_TYPE_NP[et]
    rng = np.random.default_rng(n)
    if np.issubdtype(dt, np.floating):
        a = ((rng.random(n) - 0.5) * 1e4).astype(dt)
    else:
        a = rng.integers(0, min(np.iinfo(dt).max, 2**31 - 1), n, dtype=np.int64).astype(dt)
    keys = fn(a)
    s = clo.Sorter("satradix", ctx, et, key_type=kt, get_key=expr)
    got = s.with_host_data(a, q)
    order = np.argsort(keys, kind="stable")
    assert np.array_equal(got.view(np.dtype("u%d" % dt.itemsize)), a[order].view(np.dtype("u%d" % dt.itemsize)))
    # in place on device data, and a compare string is accepted and ignored (as upstream)
    b = clo.Buffer(ctx, a.nbytes)
    b.write(q, a)
    s.with_device_data(q, b, None, n)
    assert np.array_equal(b.read(q, dt, n).view(np.dtype("u%d" % dt.itemsize)), a[order].view(np.dtype("u%d" % dt.itemsize)))
    b.close()
    s.close()


def test_satradix_jit_refuses_bad_expressions(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    with pytest.raises(clo.CloError) as e:
        clo.Sorter("satradix", ctx, "uint", get_key="((x) >> 4")         # does not compile
    assert e.value.code == CLO_ERROR_ARGS and "get_key" in e.value.message
    s = clo.Sorter("satradix", ctx, "uint", compare="((a) >= (b)) /* ignored */")
    a = rand_u32(np.random.default_rng(1), 5000)
    assert np.array_equal(s.with_host_data(a, q), np.sort(a))
    s.close()


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
def test_jit_get_key_division_equals_shift(gpu, alg):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = O.bench_rand(3, "uint", 1 << 15)
    s = clo.Sorter(alg, ctx, "uint", get_key="((x) / 65536)")       # == x >> 16, but not parseable as a shift
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, O.sbitonic(a, key_shift=16))           # bit-exact incl. tie order


@pytest.mark.parametrize("alg", ["sbitonic", "abitonic"])
def test_jit_compare_low_byte_order(gpu, alg):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = O.bench_rand(4, "uint", 1 << 16)
    s = clo.Sorter(alg, ctx, "uint", compare="(((a) & 0xFF) > ((b) & 0xFF))")
    got = s.with_host_data(a, q)
    s.close()
    assert np.array_equal(got, O.sbitonic(a, key_size=1))             # key = low byte, same network, same ties
    assert np.all(np.diff((got & 0xFF).astype(np.int64)) >= 0)


def test_jit_negated_compare_and_float_keys(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    a = O.bench_rand(5, "uint", 1 << 14)
    s = clo.Sorter("abitonic", ctx, "uint", compare="(!((a) <= (b)))")
    assert np.array_equal(s.with_host_data(a, q), np.sort(a))
    s.close()
    f = np.random.default_rng(6).permutation(1 << 14).astype(np.float32) - 5000.0   # distinct values
    s = clo.Sorter("abitonic", ctx, "float", get_key="(-(x))")
    assert np.array_equal(s.with_host_data(f, q), np.sort(f)[::-1])
    s.close()
    pairs = (np.random.default_rng(7).integers(0, 1 << 20, 1 << 14, dtype=np.uint64) << np.uint64(32)) \
        | np.arange(1 << 14, dtype=np.uint64)
    s = clo.Sorter("sbitonic", ctx, "ulong", key_type="uint", get_key="(uint) ((x) / 4294967296ul)")
    assert np.array_equal(s.with_host_data(pairs, q), O.sbitonic(pairs, key_size=4, key_shift=32))
    s.close()


def test_jit_reports_compile_errors_and_sorts_any_numel(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    with pytest.raises(clo.CloError) as e:
        clo.Sorter("abitonic", ctx, "uint", get_key="((x) +* 3)")
    assert e.value.code == 2 and "Could not build kernels" in e.value.message
    s = clo.Sorter("abitonic", ctx, "uint", get_key="((x) % 1000)")
    # not a power of two (round 3; refused before): the flip form of the network, comparators past numel skipped
    for m in (1000, 3, 1025, 70001):
        b = np.random.default_rng(m).permutation(m).astype(np.uint32)
        got = s.with_host_data(b, q)
        assert np.all(np.diff((got % 1000).astype(np.int64)) >= 0) and np.array_equal(np.sort(got), np.arange(m))
    got = s.with_host_data(np.arange(1024, dtype=np.uint32)[::-1].copy(), q)
    assert np.all(np.diff((got % 1000).astype(np.int64)) >= 0) and np.array_equal(np.sort(got), np.arange(1024))
    s.close()
