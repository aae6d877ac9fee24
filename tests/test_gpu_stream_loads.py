"""The read-once loads of a radix sort's step — the histograms over the keys and over the digit bytes, the pass
kernel's tile, the key-value first pass, the single-sweep passes — at the smallest sizes that reach each of their
shapes, bit for bit against numpy: np.sort for keys, a stable argsort for pairs. (The histograms of 4-byte elements on
the 1024-thread tiles mark their loads non-temporal, plain and segmented; every other shape loads with the default
policy: clo_hip_radixw.hip, rw_shape.)

uint32: 2^26 keys are the smallest array on the 1024-thread tiles, 2^26 - 5 the same keys with a partial last tile
(below 256 MiB: 512-thread tiles), 2^26 + 5 a partial last 1024-thread tile, 2^22 + 1 the 512-thread shape, 2^20 the
single-sweep passes. 8-byte elements (uint64 keys, and key << 32 | value pairs sorted by the key): 2^22 elements are
the smallest array on the big tiles, 2^22 - 3 ends in a partial tile. Views that start one element past a 16-byte
boundary take the element-aligned vector loads. One segmented sort of three uneven segments, and one by-key sort with
keys and values in arrays of their own (the fused first pass reads both).

The references are computed once per module. A prefix of an array whose tail holds the largest key sorts to the same
prefix of the sorted array, so one np.sort serves every length of a family."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_TAIL = 16           # elements at the end of every array that hold the largest key


@pytest.fixture(scope="module")
def dev():
    import cl_ops_amd as clo
    ctx = clo.Context(0)
    q = clo.Queue(ctx)
    yield clo, ctx, q
    q.close()
    ctx.close()


def _keys(dt, n, seed):
    a = np.random.default_rng(seed).integers(0, 1 << (8 * np.dtype(dt).itemsize), n, dtype=dt)
    a[-_TAIL:] = np.iinfo(dt).max
    return a


@pytest.fixture(scope="module")
def u32():
    """2^26 + 5 uint32 keys; the last 16 are the largest key."""
    a = _keys(np.uint32, (1 << 26) + 5, 26)
    return a, np.sort(a)


@pytest.fixture(scope="module")
def u64():
    a = _keys(np.uint64, 1 << 22, 22)
    return a, np.sort(a)


@pytest.fixture(scope="module")
def pairs():
    """key << 32 | index with few distinct keys (stability shows); the last 16 keys are the largest."""
    n = 1 << 22
    k = np.random.default_rng(7).integers(0, 1 << 20, n, dtype=np.uint64)
    k[-_TAIL:] = (1 << 32) - 1
    a = (k << np.uint64(32)) | np.arange(n, dtype=np.uint64)
    return a, a[np.argsort(k, kind="stable")]


def _sort_view(dev, s, a, n, off_elems=0):
    """Sorts the first n elements of `a`, placed off_elems elements into an allocation, into a second buffer."""
    clo, ctx, q = dev
    es = a.itemsize
    base = clo.Buffer(ctx, (n + off_elems) * es)
    src = clo.Buffer(ctx, n * es, device_ptr=base.ptr + off_elems * es)
    dst = clo.Buffer(ctx, n * es)
    src.write(q, a[:n])
    s.with_device_data(q, src, dst, n)
    q.finish()
    got = dst.read(q, a.dtype, n)
    src.close()
    dst.close()
    base.close()
    return got


@pytest.mark.parametrize("n,off", [(1 << 26, 0), ((1 << 26) - 5, 0), ((1 << 26) + 5, 0), (1 << 26, 1)])
def test_uint32_big_shape(dev, u32, n, off):
    clo, ctx, q = dev
    a, want = u32
    s = clo.Sorter("satradix", ctx, "uint")
    got = _sort_view(dev, s, a, n, off)
    s.close()
    assert np.array_equal(got, want[:n])


@pytest.mark.parametrize("n", [(1 << 22) + 1, 1 << 20])
def test_uint32_small_tiles_and_sweeps(dev, u32, n):
    clo, ctx, q = dev
    a = u32[0][:n]
    s = clo.Sorter("satradix", ctx, "uint")
    got = _sort_view(dev, s, a, n)
    s.close()
    assert np.array_equal(got, np.sort(a))


@pytest.mark.parametrize("n,off", [(1 << 22, 0), ((1 << 22) - 3, 0), (1 << 22, 1)])
def test_uint64(dev, u64, n, off):
    clo, ctx, q = dev
    a, want = u64
    s = clo.Sorter("satradix", ctx, "ulong")
    got = _sort_view(dev, s, a, n, off)
    s.close()
    assert np.array_equal(got, want[:n])


@pytest.mark.parametrize("n,off", [(1 << 22, 0), ((1 << 22) - 3, 0), (1 << 22, 1)])
def test_pairs(dev, pairs, n, off):
    clo, ctx, q = dev
    a, want = pairs
    s = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    got = _sort_view(dev, s, a, n, off)
    s.close()
    assert np.array_equal(got, want[:n])


def test_segmented_three_uneven_segments(dev, u32):
    import torch
    from cl_ops_amd import _hip
    from cl_ops_amd._hip import lib
    seg = [(1 << 25) + 17, 5, (1 << 25) - 17]          # (2^26 + 5 keys: the segmented launches on the 1024-thread tiles)
    n = sum(seg)
    a = u32[0]
    assert a.size == n
    want = np.concatenate([np.sort(x) for x in np.split(a, np.cumsum(seg)[:-1])])
    ta = torch.from_numpy(a.view(np.int32).copy()).cuda()
    tb = torch.full_like(ta, -1)
    need = lib.clo_hip_radix_seg_workspace_bytes(n, len(seg), 4, 4)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    in_b = C.c_int(-1)
    st = lib.clo_hip_radix_sort_segmented(ta.data_ptr(), ta.data_ptr(), tb.data_ptr(), n, (C.c_size_t * 3)(*seg), 3, None, None, None, 0,
                                          4, 0, 32, 4, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream, C.byref(in_b))
    _hip.check(st, "clo_hip_radix_sort_segmented")
    torch.cuda.synchronize()
    assert in_b.value == 0
    assert np.array_equal(ta.cpu().numpy().view(np.uint32), want)


def test_by_key_separate_arrays(dev, u32):
    """clo_sort_by_key_with_device_data at 2^22 + 1 pairs: the fused first pass loads keys and values from two arrays."""
    clo, ctx, q = dev
    n = (1 << 22) + 1
    keys = u32[0][:n] >> np.uint32(12)                       # (2^20 distinct keys: equal keys keep their order)
    values = np.arange(n, dtype=np.uint32) * np.uint32(2654435761)
    order = np.argsort(keys, kind="stable")
    s = clo.Sorter("satradix", ctx, "uint")
    kin, vin, kout, vout = (clo.Buffer(ctx, 4 * n) for _ in range(4))
    kin.write(q, keys)
    vin.write(q, values)
    s.by_key_with_device_data(q, kin, vin, kout, vout, n)
    q.finish()
    got_k, got_v = kout.read(q, np.uint32, n), vout.read(q, np.uint32, n)
    for b in (kin, vin, kout, vout):
        b.close()
    s.close()
    assert np.array_equal(got_k, keys[order])
    assert np.array_equal(got_v, values[order])
