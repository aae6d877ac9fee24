"""Element indices above 2^31 in reduce by key, scan by key, histogram, merge, the by-key sort, search and the set
operations: n = 2^31 + 2^20 + 5 uchar keys, the smallest shape at which an element index (a position in the haystack, an
index into A || B) needs bit 31 and, with 4-byte outputs, a byte offset passes 2^32, while everything stays at a few
GiB. The inputs are made and the results checked on the device with torch, in chunks, so that the host never holds them
(the method of test_indices_above_2p31_satradix_and_scan); every expectation is closed-form or a torch.bincount, and
exact. (Select has its case in test_gpu_select.py.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = (1 << 31) + (1 << 20) + 5
CHUNK = 1 << 28
CANARY = 0xA5


@pytest.fixture
def dev(gpu):
    import torch
    import cl_ops_amd as clo
    ctx, q = gpu
    if torch.cuda.get_device_properties(0).total_memory < (96 << 30):
        pytest.skip("needs ~60 GiB of device memory")
    yield clo, ctx, q, torch
    torch.cuda.empty_cache()           # (the next test's arrays are as large again)


def chunks(n, step=CHUNK):
    return [(lo, min(lo + step, n)) for lo in range(0, n, step)]


def as_buffer(clo, ctx, t):
    return clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())


class Runs:
    """The run structure of the reduce / scan by key cases: run r(i) = i // 5, except for one run of 3 tiles + 1
    elements laid across index 2^31; the key of run r is r & 0xff (neighbouring runs always differ)."""

    def __init__(self, tile):
        self.long = 3 * tile + 1
        self.s0 = (((1 << 31) - self.long // 2) // 5) * 5          # where the long run starts: a multiple of 5
        self.r0 = self.s0 // 5                                      # its number
        self.after = self.s0 + self.long                            # the first element behind it
        assert self.s0 < (1 << 31) < self.after < N
        self.rows = self.r0 + 1 + -(-(N - self.after) // 5)
        self.last = (N - self.after) - 5 * (self.rows - self.r0 - 2)   # the length of the last run, 1 .. 5

    def run_and_start(self, torch, lo, hi):
        """(r(i), b(i)) for i in [lo, hi): the run's number and its first index."""
        i = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        t = (i - self.after).div(5, rounding_mode="floor")
        r = torch.where(i < self.s0, i.div(5, rounding_mode="floor"), torch.where(i < self.after, self.r0, self.r0 + 1 + t))
        b = torch.where(i < self.s0, i - i % 5, torch.where(i < self.after, self.s0, self.after + 5 * t))
        return i, r, b

    def keys(self, torch):
        k = torch.empty(N, dtype=torch.uint8, device="cuda")
        for lo, hi in chunks(N):
            k[lo:hi] = (self.run_and_start(torch, lo, hi)[1] & 0xff).to(torch.uint8)
        return k


def test_reduce_by_key_run_lengths(dev):
    """Run lengths in uint, keys out. The row count, keys_out[r] = r & 0xff and the lengths (5, the long run's, the last
    run's) are closed-form; the rows from the count on keep their canary."""
    clo, ctx, q, torch = dev
    runs = Runs(clo.reduce_by_key_tile(1, 0))
    keys = runs.keys(torch)
    ko = torch.full((N,), CANARY, dtype=torch.uint8, device="cuda")
    ao = torch.full((N,), CANARY * 0x01010101 - (1 << 32), dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (keys, ko, ao, cnt)]
    r = clo.ReduceByKey(ctx, "uchar", None, "uint")
    assert r.with_device_data(q, bufs[0], None, bufs[1], bufs[2], bufs[3], N)
    q.finish()
    m = runs.rows
    assert int(cnt[0]) == m
    for lo, hi in chunks(m):
        want = (torch.arange(lo, hi, dtype=torch.int64, device="cuda") & 0xff).to(torch.uint8)
        assert bool((ko[lo:hi] == want).all()), "keys_out, rows %d .. %d" % (lo, hi)
        want = torch.full((hi - lo,), 5, dtype=torch.int32, device="cuda")
        if lo <= runs.r0 < hi:
            want[runs.r0 - lo] = runs.long
        if hi == m:
            want[-1] = runs.last
        assert bool((ao[lo:hi] == want).all()), "aggr_out, rows %d .. %d" % (lo, hi)
    assert bool((ko[m:] == CANARY).all()) and bool((ao[m:] == CANARY * 0x01010101 - (1 << 32)).all()), "rows beyond the run count were written"
    assert bool((keys == runs.keys(torch)).all()), "keys_in changed"
    for x in bufs + [r]:
        x.close()


def test_scan_by_key_exclusive_rank(dev):
    """The exclusive rank in uint: data_out[i] = i - b(i), b(i) the first index of i's run."""
    clo, ctx, q, torch = dev
    runs = Runs(clo.scan_by_key_tile(1, 0))
    keys = runs.keys(torch)
    out = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (keys, out)]
    s = clo.ScanByKey(ctx, "uchar", None, "uint")
    assert s.with_device_data(q, bufs[0], None, bufs[1], N)
    q.finish()
    for lo, hi in chunks(N):
        i, _, b = runs.run_and_start(torch, lo, hi)
        assert bool((out[lo:hi] == (i - b).to(torch.int32)).all()), "ranks %d .. %d" % (lo, hi)   # (every rank is below 2^31)
    for x in bufs + [s]:
        x.close()


@pytest.mark.parametrize("st", ["ulong", "uint"])
def test_histogram_counts(dev, st):
    """lower 16, shift 2, 40 bins (the keys 16 .. 175 are counted), counts in ulong and in uint, against torch.bincount
    summed over chunks; the bin behind the last keeps its canary."""
    clo, ctx, q, torch = dev
    g = torch.Generator(device="cuda").manual_seed(41)
    keys = torch.randint(0, 256, (N,), dtype=torch.uint8, device="cuda", generator=g)
    want = torch.zeros(40, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(N):
        d = (keys[lo:hi].to(torch.int64) - 16) >> 2
        want += torch.bincount(d[(d >= 0) & (d < 40)], minlength=40)
    assert 0 < int(want.sum()) < N and int(want.min()) > 0
    out = torch.full((41,), -2, dtype=torch.int64 if st == "ulong" else torch.int32, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, keys), clo.Buffer(ctx, 40 * out.element_size(), device_ptr=out.data_ptr())]
    h = clo.Histogram(ctx, "uchar", None, st)
    assert h.with_device_data(q, bufs[0], None, bufs[1], N, lower=16, shift=2, num_bins=40)
    q.finish()
    assert bool((out[:40].to(torch.int64) == want).all()), (out.tolist(), want.tolist())    # (every count is below 2^31)
    assert int(out[40]) == -2
    for x in bufs + [h]:
        x.close()


def test_argmerge_with_keys_out(dev):
    """na = 2^31 + 5 and nb = 2^20 uchar keys, a[i] = i * 256 // na and b[i] = i * 256 // nb: keys_out is non-decreasing
    with count_a + count_b elements per value, and inside value k's stretch the permutation holds the count_a[k]
    indices of A in order, then na + the indices of B in order (the two 256-entry tables are closed-form)."""
    clo, ctx, q, torch = dev
    na, nb = (1 << 31) + 5, 1 << 20
    assert na + nb == N
    a = torch.empty(na, dtype=torch.uint8, device="cuda")
    for lo, hi in chunks(na):
        a[lo:hi] = (torch.arange(lo, hi, dtype=torch.int64, device="cuda") * 256).div(na, rounding_mode="floor").to(torch.uint8)
    b = (torch.arange(nb, dtype=torch.int64, device="cuda") * 256).div(nb, rounding_mode="floor").to(torch.uint8)
    start_a = [-(-k * na // 256) for k in range(257)]          # the first i with i * 256 // na >= k
    start_b = [-(-k * nb // 256) for k in range(257)]
    T = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda")
    sa, sb = T(start_a[:256]), T(start_b[:256])
    ca, cb = T(np.diff(start_a).tolist()), T(np.diff(start_b).tolist())
    off = sa + sb                                              # where value k's stretch starts in the output
    ko = torch.full((N,), CANARY, dtype=torch.uint8, device="cuda")
    vo = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (a, b, ko, vo)]
    m = clo.Merge(ctx, "uchar", 4)
    assert m.with_device_data(q, bufs[0], None, na, bufs[1], None, nb, bufs[2], bufs[3])
    q.finish()
    counts = torch.zeros(256, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(N):
        k = ko[lo:hi].to(torch.int64)
        counts += torch.bincount(k, minlength=256)
        assert bool((k[1:] >= k[:-1]).all()) and (lo == 0 or int(ko[lo - 1]) <= int(k[0])), "keys_out decreases in %d .. %d" % (lo, hi)
        t = torch.arange(lo, hi, dtype=torch.int64, device="cuda") - off[k]
        want = torch.where(t < ca[k], sa[k] + t, na + sb[k] + t - ca[k])
        assert bool(((vo[lo:hi].to(torch.int64) & 0xFFFFFFFF) == want).all()), "the permutation, outputs %d .. %d" % (lo, hi)
    assert bool((counts == ca + cb).all())
    for x in bufs + [m]:
        x.close()


def test_argsort_by_key_with_keys_out(dev):
    """uchar keys from torch.randint: keys_out is non-decreasing with the input's bincount, keys_in[values_out[j]] ==
    keys_out[j], and values_out increases wherever two neighbouring keys are equal (stability)."""
    clo, ctx, q, torch = dev
    g = torch.Generator(device="cuda").manual_seed(42)
    keys = torch.randint(0, 256, (N,), dtype=torch.uint8, device="cuda", generator=g)
    before = torch.zeros(256, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(N):
        before += torch.bincount(keys[lo:hi].to(torch.int64), minlength=256)
    ko = torch.full((N,), CANARY, dtype=torch.uint8, device="cuda")
    vo = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (keys, ko, vo)]
    s = clo.Sorter("satradix", ctx, "uchar")
    assert s.by_key_with_device_data(q, bufs[0], None, bufs[1], bufs[2], N)
    q.finish()
    after = torch.zeros(256, dtype=torch.int64, device="cuda")
    for lo, hi in chunks(N):
        end = min(hi + 1, N)                                   # one element more: the pair across the chunk's end
        k = ko[lo:end]
        v = vo[lo:end].to(torch.int64) & 0xFFFFFFFF
        after += torch.bincount(k[:hi - lo].to(torch.int64), minlength=256)
        assert bool((k[1:] >= k[:-1]).all()), "keys_out decreases in %d .. %d" % (lo, hi)
        assert bool((keys[v[:hi - lo]] == k[:hi - lo]).all()), "values_out does not lead to the key, outputs %d .. %d" % (lo, hi)
        assert bool(((v[1:] > v[:-1]) | (k[1:] != k[:-1])).all()), "equal keys out of their input order in %d .. %d" % (lo, hi)
    assert bool((after == before).all())
    for x in bufs + [s]:
        x.close()


def same(x, y):
    """x == y everywhere. A helper, so that a failing assert does not print the operands: pytest's report of a failing
    `==` walks both sides element by element, which on two device tensors of 2^28 elements never ends."""
    return bool((x == y).all())


def ascending(x):
    return bool((x[1:] >= x[:-1]).all())


def ramp(torch, n, z=0):
    """x[i] = i * 256 // n as uchar, and the 257 starts of its values: start[k] is the first i with x[i] >= k. z > 0:
    z zeros first and the values 1 .. 255 over the rest, x[i] = 1 + (i - z) * 255 // (n - z)."""
    x = torch.empty(n, dtype=torch.uint8, device="cuda")
    for lo, hi in chunks(n):
        i = torch.arange(lo, hi, dtype=torch.int64, device="cuda")
        x[lo:hi] = ((i * 256).div(n, rounding_mode="floor") if not z else torch.where(i < z, 0, 1 + ((i - z) * 255).div(n - z, rounding_mode="floor"))).to(torch.uint8)
    if not z:
        return x, [-(-k * n // 256) for k in range(257)]
    return x, [0] + [z + -(-(k - 1) * (n - z) // 255) for k in range(1, 257)]


@pytest.mark.parametrize("hay", ["ramp", "zeros up to 2^31 - 3, then the ramp"])
@pytest.mark.parametrize("path", ["general", "sorted"])
def test_search_positions(dev, path, hay):
    """A haystack of N keys h[i] = i * 256 // N; the needles are every byte value, repeated to 3 tiles + 1 entries,
    ascending under NEEDLES_SORTED and in a fixed permutation without. The lower bound of value k is start[k], the upper
    bound start[k + 1]. Every search probes indices above 2^31 on its way, but with this haystack N itself (the upper
    bound of 255) is the one position above 2^31, so the second haystack holds 2^31 - 3 zeros and spreads the values
    1 .. 255 over the 2^20 + 8 keys behind them: all but the lower bounds of 0 and 1 need bit 31 or lie just below it.
    pos_out has a canary behind it."""
    clo, ctx, q, torch = dev
    nn = 3 * clo.search_tile(1) + 1
    z = 0 if hay == "ramp" else (1 << 31) - 3
    hay, start = ramp(torch, N, z)
    start = np.array(start, dtype=np.int64)
    assert start[0] == 0 and start[256] == N and (np.diff(start) > 0).all()
    ndl = np.sort(np.resize(np.arange(256, dtype=np.uint8), nn))
    if path == "general":
        ndl = ndl[np.random.default_rng(31).permutation(nn)]
    needles = torch.from_numpy(ndl).cuda()
    pos = torch.full((nn + 64,), CANARY * 0x01010101 - (1 << 32), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, hay), as_buffer(clo, ctx, needles), clo.Buffer(ctx, 4 * nn, device_ptr=pos.data_ptr())]
    s = clo.Search(ctx, "uchar")
    try:
        for upper in (False, True):
            pos.fill_(CANARY * 0x01010101 - (1 << 32))
            torch.cuda.synchronize()
            assert s.with_device_data(q, bufs[0], N, bufs[1], nn, bufs[2], upper=upper, needles_sorted=path == "sorted")
            q.finish()
            got = pos.cpu().numpy().view(np.uint32)
            want = start[ndl.astype(np.int64) + (1 if upper else 0)]
            assert (want >= 1 << 31).sum() >= (nn // 2 if z else int(upper))
            assert np.array_equal(got[:nn].astype(np.int64), want), "%s, %s" % (path, "upper" if upper else "lower")
            assert (got[nn:] == CANARY * 0x01010101).all(), "pos_out was written behind its end"
        assert np.array_equal(needles.cpu().numpy(), ndl), "the needles changed"
        assert same(hay, ramp(torch, N, z)[0]), "the haystack changed"
    finally:
        for x in bufs + [s]:
            x.close()
        del hay, pos


def _setop_case(dev, op, na, nb, rows_of, count_of):
    """The arg form with keys_out of a[i] = i * 256 // na and b[i] = i * 256 // nb. count_of(ca, cb): the elements kept
    of every value; rows_of(t, k, sa, sb, ca, cb): the index in A || B that row t of value k's stretch holds."""
    clo, ctx, q, torch = dev
    a, start_a = ramp(torch, na)
    b, start_b = ramp(torch, nb)
    T = lambda x: torch.tensor(x, dtype=torch.int64, device="cuda")
    sa, sb = T(start_a[:256]), T(start_b[:256])
    ca, cb = T(np.diff(start_a).tolist()), T(np.diff(start_b).tolist())
    kept = count_of(ca, cb)
    assert int(kept.min()) > 0
    off = torch.cumsum(kept, 0) - kept                         # where value k's stretch starts in the output
    total = int(kept.sum())
    s = clo.SetOp(op, ctx, "uchar", 4)
    cap = s.max_numel_out(na, nb)
    assert (1 << 30) < total <= cap and 4 * total > 1 << 32     # values_out passes byte offset 2^32
    ko = torch.full((cap,), CANARY, dtype=torch.uint8, device="cuda")
    vo = torch.full((cap,), CANARY * 0x01010101 - (1 << 32), dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (a, b, ko, vo, cnt)]
    try:
        assert s.with_device_data(q, bufs[0], None, na, bufs[1], None, nb, bufs[2], bufs[3], bufs[4])
        q.finish()
        assert int(cnt[0]) == total
        counts = torch.zeros(256, dtype=torch.int64, device="cuda")
        above = 0
        for lo, hi in chunks(total):
            k = ko[lo:hi].to(torch.int64)
            counts += torch.bincount(k, minlength=256)
            assert ascending(k) and (lo == 0 or int(ko[lo - 1]) <= int(k[0])), "keys_out decreases in %d .. %d" % (lo, hi)
            t = torch.arange(lo, hi, dtype=torch.int64, device="cuda") - off[k]
            want = rows_of(t, k, sa, sb, ca, cb)
            above += int((want > 1 << 31).sum())
            assert same(vo[lo:hi].to(torch.int64) & 0xFFFFFFFF, want), "the indices, rows %d .. %d" % (lo, hi)
        assert same(counts, kept) and above > 0
        assert same(ko[total:], CANARY) and same(vo[total:], CANARY * 0x01010101 - (1 << 32)), "rows at index >= k were written"
        assert same(a, ramp(torch, na)[0]) and same(b, ramp(torch, nb)[0]), "an input changed"
    finally:
        for x in bufs + [s]:
            x.close()
        del a, b, ko, vo


def test_setop_difference_indices(dev):
    """A - B with na = 2^31 + 5 and nb = 2^20: every value keeps its run of A without the first count_b[k] elements,
    so k = na - nb, and the last rows hold indices above 2^31."""
    _setop_case(dev, "difference", (1 << 31) + 5, 1 << 20, lambda t, k, sa, sb, ca, cb: sa[k] + cb[k] + t, lambda ca, cb: ca - cb)


def test_setop_union_indices(dev):
    """The roles swapped, na = 2^20 and nb = 2^31 + 5: every element of A is kept, then B's elements of rank >=
    count_a[k] within their run, as na + j. The indices from B exceed 2^31 by more than na: the base of B's indices
    (numel_a + the tile's first index of B - ..., mod 2^32) is what this is about."""
    na = 1 << 20
    _setop_case(dev, "union", na, (1 << 31) + 5, lambda t, k, sa, sb, ca, cb: (sa[k] + t).where(t < ca[k], na + sb[k] + t), lambda ca, cb: cb)
