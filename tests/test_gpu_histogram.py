"""CloHistogram (include/clo_histogram.h) on the GPU against the numpy model of tests/hist_model.py, bit for bit.
Every array is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the method of
test_gpu_views.py), so hist_out has a canary directly after bin num_bins - 1; hist_out is pre-filled with the pattern,
and after every call it equals the model while the guards and both inputs are unchanged. Sizes around the tile edges
(the tile comes from clo_hip_histogram_tile), the grid-stride loop walked by 1, 2 and 3 work-groups through the thin
ABI, bin counts on both sides of every switch of the kernels (32 LDS copies / fewer copies / counters in hist_out; the
limit comes from clo_hip_histogram_lds_bins), key layouts, same-address contention, keys outside the range, every key
type with negative and extreme lower bounds and the wrap trap, shifts, every value -> sum pair, "accumulate",
element-aligned views, the histogram -> scan pipeline on one queue, an object reused, the thin ABI's status codes."""
import numpy as np
import pytest

from hist_model import histogram

pytestmark = pytest.mark.gpu

G = 256
_PAT = [((np.arange(251 * 16) * 167 + 41 * k) % 251).astype(np.uint8) ^ np.uint8(0xA5) for k in range(3)]
_NP = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
       "long": np.int64, "ulong": np.uint64}
_UBITS = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
KEY_TYPES = ["char", "uchar", "short", "ushort", "int", "uint", "long", "ulong"]
PAIRS = [("int", "int"), ("int", "uint"), ("uint", "int"), ("uint", "uint"), ("int", "long"), ("int", "ulong"),
         ("uint", "long"), ("uint", "ulong"), ("long", "long"), ("long", "ulong"), ("ulong", "long"), ("ulong", "ulong"),
         (None, "int"), (None, "uint"), (None, "long"), (None, "ulong")]


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

    def contents(self, dtype):
        """What the view held when it was made."""
        return self.host[self.at:self.at + self.n].copy().view(dtype)

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


def key_at(kt, lower, d):
    """lower + d in the key type, for an integer array d (int64, or uint64 holding d modulo 2^64; the true value must
    lie in the type's range)."""
    dt = np.dtype(_NP[kt])
    d = np.asarray(d)
    if d.dtype != np.uint64:
        d = d.astype(np.int64).view(np.uint64)
    u = d + np.uint64(int(lower) & (2 ** 64 - 1))   # modulo 2^64
    return u.astype(_UBITS[dt.itemsize]).view(dt)


def span_of(kt, lower, shift, nb):
    """How many differences d >= 0 are counted AND representable: min(num_bins << shift, max - lower + 1)."""
    return min(nb << shift, int(np.iinfo(_NP[kt]).max) - int(lower) + 1)


def make_keys(kt, layout, n, lower, shift, nb, seed=0):
    rng = np.random.default_rng(seed)
    span = span_of(kt, lower, shift, nb)                 # up to 2^64: differences are kept modulo 2^64 in uint64
    u = lambda x: np.uint64(int(x) % (1 << 64))
    if layout == "uniform":
        d = rng.integers(0, span, n, dtype=np.uint64)
    elif layout == "sorted":
        d = np.sort(rng.integers(0, span, n, dtype=np.uint64))
    elif layout == "alternating":      # two bins, the first and the last that exists
        d = np.where(np.arange(n) % 2 == 0, u(0), u(span - 1))
    elif layout == "equal":
        d = np.full(n, u(span // 2))
    elif layout == "edges":            # exactly at lower, at lower + (num_bins << shift) - 1, and one beyond it; one below
        room = int(np.iinfo(_NP[kt]).max) - int(lower) - span + 1        # how many keys lie beyond the range
        below = -1 if int(lower) > int(np.iinfo(_NP[kt]).min) else 0
        d = np.resize(np.array([u(0), u(span - 1), u(span if room >= 1 else span - 1), u(below)], np.uint64), n)
    elif layout == "skewed":           # 90 % in one bin
        d = np.where(rng.random(n) < 0.9, u(span // 3), rng.integers(0, span, n, dtype=np.uint64))
    else:
        raise KeyError(layout)
    return key_at(kt, lower, d)


def make_values(vt, n, seed):
    """Over the full range of the type, so that 32-bit sums wrap."""
    if vt is None:
        return None
    rng = np.random.default_rng(seed + 77)
    a = rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)
    return a.astype(_UBITS[np.dtype(_NP[vt]).itemsize]).view(_NP[vt])


def run_case(dev, kt, vt, st, keys, values, lower, shift, nb, what, offs=(0, 0, 0), obj=None, accumulate=False, prefill=None,
             want=None):
    """One call on views at byte offsets offs = (keys_in, values_in, hist_out); checks everything. Returns the model's
    histogram."""
    clo, ctx, q = dev
    n = keys.size
    sdt = np.dtype(_NP[st])
    h = obj or clo.Histogram(ctx, kt, vt, st, options="accumulate" if accumulate else None)
    kin = Region(dev, n * keys.itemsize, offs[0], keys, 0)
    vin = Region(dev, n * values.itemsize, offs[1], values, 1) if values is not None else None
    out = Region(dev, nb * sdt.itemsize, offs[2], prefill, 2)
    try:
        assert h.with_device_data(q, kin.view, vin.view if vin else None, out.view, n, lower=lower, shift=shift, num_bins=nb)
        q.finish()
        if want is None:
            want = histogram(keys, values, sdt, lower, shift, nb, onto=out.contents(sdt) if h.accumulate else None)
        out.check(want, what + ": hist_out")
        kin.check(keys, what + ": keys_in")
        if vin:
            vin.check(values, what + ": values_in")
        return want
    finally:
        for x in (kin, vin, out):
            if x:
                x.close()
        if obj is None:
            h.close()


def tile_of(dev, kt, vt):
    t = dev[0].histogram_tile(np.dtype(_NP[kt]).itemsize, np.dtype(_NP[vt]).itemsize if vt else 0)
    assert t > 0
    return t


def lds_bins(dev, st):
    L = dev[0].histogram_lds_bins(np.dtype(_NP[st]).itemsize)
    assert L > 256
    return L


@pytest.mark.parametrize("vt", [None, "uint"])
def test_sizes_around_the_tile_edges(dev, vt):
    """uint keys, counts and uint values summed in uint (the sums wrap); a tenth of the keys lies beyond the last bin."""
    clo, ctx, q = dev
    T = tile_of(dev, "uint", vt)
    obj = clo.Histogram(ctx, "uint", vt, "uint")
    for n in (0, 1, 3, 4, 5, 63, 64, 65, T - 1, T, T + 1, 3 * T + 1, (1 << 20) + 3, (1 << 24) + 5):
        keys = make_keys("uint", "uniform", n, 1000, 2, 285, seed=n)     # 256 bins hold 1024 of the 1140 key values
        run_case(dev, "uint", vt, "uint", keys, make_values(vt, n, n), 1000, 2, 256, "n=%d values=%s" % (n, vt), obj=obj)
    obj.close()


def _thin(dev, keys, values, vt_num, st, lower, shift, nb, max_groups, accumulate=0, key_signed=0):
    """clo_hip_histogram on canaried regions; returns the status and the three regions."""
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    sdt = np.dtype(_NP[st])
    kin = Region(dev, keys.size * keys.itemsize, 0, keys, 0)
    vin = Region(dev, values.size * values.itemsize, 0, values, 1) if values is not None else None
    out = Region(dev, nb * sdt.itemsize, 0, None, 2)
    st_num = clo.CLO_TYPES[st]
    rc = lib.clo_hip_histogram(kin.ptr, vin.ptr if vin else None, out.ptr, keys.size, keys.itemsize, key_signed, vt_num, st_num,
                               lower, shift, nb, accumulate, max_groups, None, 0, q.stream)
    q.finish()
    return rc, kin, vin, out


@pytest.mark.parametrize("max_groups", [1, 2, 3])
def test_grid_stride_loop_with_few_groups(dev, max_groups):
    """7 T + 5 elements on 1, 2 or 3 work-groups: several rounds of the grid-stride loop, groups with different numbers
    of tiles, the last tile partial, the flush of more than one group onto the same bins. All three kernels forms."""
    clo, ctx, q = dev
    for vt, st in ((None, "uint"), ("uint", "ulong")):
        T = tile_of(dev, "uint", vt)
        L = lds_bins(dev, st)
        n = 7 * T + 5
        for nb, layout in ((256, "uniform"), (4096, "uniform"), (L, "skewed"), (L + 1, "skewed"), (3, "equal")):
            keys = make_keys("uint", layout, n, 77, 0, nb, seed=nb)
            values = make_values(vt, n, nb)
            rc, kin, vin, out = _thin(dev, keys, values, clo.CLO_TYPES["uint"], st, 77, 0, nb, max_groups)
            try:
                assert rc == 0
                what = "max_groups=%d %s->%s bins=%d" % (max_groups, vt, st, nb)
                out.check(histogram(keys, values, _NP[st], 77, 0, nb), what)
                kin.check(keys, what + ": keys_in")
            finally:
                for x in (kin, vin, out):
                    if x:
                        x.close()


@pytest.mark.parametrize("st", ["uint", "ulong"])
def test_bin_counts_on_both_sides_of_every_switch(dev, st):
    clo, ctx, q = dev
    L = lds_bins(dev, st)
    T = tile_of(dev, "uint", None)
    n = 3 * T + 1
    obj = clo.Histogram(ctx, "uint", None, st)
    objv = clo.Histogram(ctx, "uint", "uint", st)
    values = make_values("uint", n, 3)
    for nb in (1, 2, 3, 255, 256, 257, 4096, L - 1, L, L + 1, 1 << 20):
        keys = make_keys("uint", "uniform", n, 5, 0, nb + nb // 8 + 1, seed=nb)   # a ninth of the keys beyond the last bin
        run_case(dev, "uint", None, st, keys, None, 5, 0, nb, "counts bins=%d" % nb, obj=obj)
        run_case(dev, "uint", "uint", st, keys, values, 5, 0, nb, "sums bins=%d" % nb, obj=objv)
    obj.close()
    objv.close()


@pytest.mark.parametrize("layout", ["uniform", "sorted", "alternating", "edges", "skewed"])
def test_key_layouts(dev, layout):
    T = tile_of(dev, "uint", None)
    L = lds_bins(dev, "uint")
    n = 5 * T + 7
    for nb, shift in ((256, 0), (256, 4), (1000, 1), (L, 0), (L + 1, 3)):
        keys = make_keys("uint", layout, n, 123456, shift, nb, seed=nb)
        run_case(dev, "uint", None, "uint", keys, None, 123456, shift, nb, "%s bins=%d shift=%d" % (layout, nb, shift))
        run_case(dev, "uint", "int", "long", keys, make_values("int", n, 1), 123456, shift, nb, "%s bins=%d shift=%d, values" % (layout, nb, shift))


def test_all_keys_equal(dev):
    """2^17 + 1 elements in one bin: the bin passes 2^16; same-address contention may cost time, never counts."""
    L = lds_bins(dev, "uint")
    n = (1 << 17) + 1
    for nb in (1, 256, 4096, L, L + 1):
        keys = make_keys("uint", "equal", n, 9, 0, nb)
        want = run_case(dev, "uint", None, "uint", keys, None, 9, 0, nb, "equal keys, counts, bins=%d" % nb)
        assert want[nb // 2] == n and want.sum() == n
        run_case(dev, "uint", "uint", "uint", keys, make_values("uint", n, 2), 9, 0, nb, "equal keys, wrapping sums, bins=%d" % nb)
        run_case(dev, "uint", "uint", "ulong", keys, make_values("uint", n, 2), 9, 0, nb, "equal keys, 64-bit sums, bins=%d" % nb)


def test_nothing_or_half_counted(dev):
    T = tile_of(dev, "int", None)
    L = lds_bins(dev, "uint")
    n = 3 * T + 9
    rng = np.random.default_rng(4)
    for nb in (16, 4096, L + 1):
        outside = np.concatenate((rng.integers(-1000, 100, n // 2), rng.integers(100 + nb, 100 + nb + 5000, n - n // 2))).astype(np.int32)
        want = run_case(dev, "int", None, "uint", outside, None, 100, 0, nb, "every key outside, bins=%d" % nb)
        assert not want.any()
        run_case(dev, "int", "int", "long", outside, make_values("int", n, 1), 100, 0, nb, "every key outside, values, bins=%d" % nb)
        half = np.where(np.arange(n) % 2 == 0, rng.integers(-5000, 100, n), rng.integers(100, 100 + nb, n)).astype(np.int32)
        want = run_case(dev, "int", None, "uint", half, None, 100, 0, nb, "half below lower, bins=%d" % nb)
        assert want.sum() == n // 2
        run_case(dev, "int", "int", "int", half, make_values("int", n, 2), 100, 0, nb, "half below lower, values, bins=%d" % nb)


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_lower_bounds_and_shifts(dev, kt):
    """Every key type: lower 0 / negative for signed types / at the type's minimum / NULL-like 0, shifts 0, 1, 7, B - 1,
    keys over the type's whole range so that most are ignored on both sides."""
    clo, ctx, q = dev
    info = np.iinfo(_NP[kt])
    T = tile_of(dev, kt, None)
    n = 2 * T + 3
    rng = np.random.default_rng(info.bits)
    anywhere = (rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, n, dtype=np.uint64)) \
        .astype(_UBITS[info.bits // 8]).view(_NP[kt])
    lowers = [0, 3, int(info.min)] + ([-50, -1] if info.min < 0 else [])
    obj = clo.Histogram(ctx, kt, "int", "long")
    for lower in lowers:
        for shift in (0, 1, 7, info.bits - 1):
            for nb in (1, 2, 40, 300):
                near = make_keys(kt, "uniform", n, lower, shift, nb, seed=nb + shift)
                below = key_at(kt, lower, -rng.integers(1, min(100, int(lower) - int(info.min) + 1), n)) if int(lower) > int(info.min) else near
                pick = rng.integers(0, 3, n)
                keys = np.where(pick == 0, anywhere, np.where(pick == 1, near, below))
                what = "%s lower=%d shift=%d bins=%d" % (kt, lower, shift, nb)
                run_case(dev, kt, None, "long", keys, None, lower, shift, nb, what, obj=obj)
                if nb == 40:
                    run_case(dev, kt, "int", "long", keys, make_values("int", n, 1), lower, shift, nb, what + ", values", obj=obj)
    obj.close()


@pytest.mark.parametrize("kt,lower", [("uchar", 250), ("int", (1 << 31) - 100), ("ulong", (1 << 64) - 100), ("long", (1 << 63) - 100),
                                      ("ushort", 65500)])
def test_the_wrap_trap(dev, kt, lower):
    """lower near the type's maximum, num_bins << shift running past it: a key below lower, whose difference modulo 2^B
    would fall inside the range, is not counted."""
    info = np.iinfo(_NP[kt])
    T = tile_of(dev, kt, None)
    n = T + 9
    rng = np.random.default_rng(3)
    L = lds_bins(dev, "uint")
    for nb, shift in ((256, 0), (4096, 1), (L + 1, 0)):
        inside = key_at(kt, lower, rng.integers(0, int(info.max) - lower + 1, n))
        trap = key_at(kt, int(info.min), rng.integers(0, min(100, (nb << shift) - (int(info.max) - lower + 1)), n))   # wrapped differences inside the range
        keys = np.where(rng.integers(0, 2, n) == 0, inside, trap)
        wrapped = (keys.astype(object) - lower) % (1 << info.bits)
        assert all((int(x) >> shift) < nb for x in wrapped)                  # unsigned arithmetic alone would count every key
        want = run_case(dev, kt, None, "uint", keys, None, lower, shift, nb, "%s wrap trap bins=%d shift=%d" % (kt, nb, shift))
        assert 0 < want.sum() < n
        run_case(dev, kt, "uint", "ulong", keys, make_values("uint", n, 5), lower, shift, nb, "%s wrap trap, values" % kt)


@pytest.mark.parametrize("vt,st", PAIRS)
def test_value_sum_pairs(dev, vt, st):
    for kt in ("uchar", "uint", "ulong"):
        T = tile_of(dev, kt, vt)
        n = 2 * T + 1
        for nb, lower in ((7, 1), (200, 0)):
            keys = make_keys(kt, "uniform", n, lower, 0, nb + 20, seed=nb)
            run_case(dev, kt, vt, st, keys, make_values(vt, n, nb), lower, 0, nb, "%s %s->%s bins=%d" % (kt, vt, st, nb))
    L = lds_bins(dev, st)
    keys = make_keys("uint", "skewed", 3 * T + 5, 0, 2, L + 1, seed=1)
    run_case(dev, "uint", vt, st, keys, make_values(vt, keys.size, 2), 0, 2, L + 1, "%s->%s, counters in hist_out" % (vt, st))
    run_case(dev, "uint", vt, st, keys, make_values(vt, keys.size, 2), 0, 2, L, "%s->%s, one counter copy" % (vt, st))


def test_sums_that_wrap_extend_and_pass_2p32(dev):
    T = tile_of(dev, "uint", "uint")
    n = 2 * T + 11
    rng = np.random.default_rng(8)
    keys = np.where(rng.random(n) < 0.7, 5, rng.integers(0, 16, n)).astype(np.uint32)
    near = rng.integers((1 << 32) - 1000, 1 << 32, n, dtype=np.uint32)           # values near 2^32 - 1, most in bin 5
    for nb in (16, 4096):
        want = run_case(dev, "uint", "uint", "uint", keys, near, 0, 0, nb, "uint sums that wrap")
        assert int(want[5]) != int(near[keys == 5].astype(np.uint64).sum())      # it did wrap
        want = run_case(dev, "uint", "uint", "ulong", keys, near, 0, 0, nb, "uint -> ulong above 2^32")
        assert want[5] > np.uint64(1 << 32)
        want = run_case(dev, "uint", "int", "long", keys, near.view(np.int32), 0, 0, nb, "int -> long, negative values")
        assert want[5] < 0
        want = run_case(dev, "uint", "uint", "long", keys, near, 0, 0, nb, "uint -> long zero-extends")
        assert want[5] > (1 << 32)


def test_accumulate(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "uint")
    n = 4 * T + 6
    L = lds_bins(dev, "uint")
    for nb in (100, 4096, L + 1):
        keys = make_keys("uint", "uniform", n, 10, 0, nb + 10, seed=nb)
        values = make_values("uint", n, 1)
        pre = np.random.default_rng(nb).integers(1, 1 << 32, nb, dtype=np.uint32)
        whole = histogram(keys, values, np.uint32, 10, 0, nb)
        # without the option a pre-filled buffer is overwritten
        run_case(dev, "uint", "uint", "uint", keys, values, 10, 0, nb, "overwrite, bins=%d" % nb, prefill=pre, want=whole)
        # with it, added onto
        with np.errstate(over="ignore"):
            run_case(dev, "uint", "uint", "uint", keys, values, 10, 0, nb, "accumulate, bins=%d" % nb, accumulate=True, prefill=pre,
                     want=pre + whole)
        # two calls over the two halves equal one call over the whole
        acc = clo.Histogram(ctx, "uint", "uint", "uint", options="accumulate")
        kin, vin = Region(dev, n * 4, 0, keys, 0), Region(dev, n * 4, 0, values, 1)
        out = Region(dev, nb * 4, 0, np.zeros(nb, np.uint32), 2)
        half = (n // 2) | 1                                                       # an odd split: the second half is only element-aligned
        k2 = clo.Buffer(ctx, (n - half) * 4, device_ptr=kin.ptr + half * 4)
        v2 = clo.Buffer(ctx, (n - half) * 4, device_ptr=vin.ptr + half * 4)
        try:
            assert acc.with_device_data(q, kin.view, vin.view, out.view, half, lower=10, shift=0, num_bins=nb)
            assert acc.with_device_data(q, k2, v2, out.view, n - half, lower=10, shift=0, num_bins=nb)
            q.finish()
            out.check(whole, "two halves, bins=%d" % nb)
        finally:
            for x in (k2, v2, kin, vin, out):
                x.close()
            acc.close()


@pytest.mark.parametrize("kt,vt,st", [("uchar", "uint", "uint"), ("ushort", "int", "long"), ("uint", "uint", "ulong"), ("int", "int", "int"),
                                      ("ulong", "ulong", "ulong"), ("long", None, "uint")])
def test_element_aligned_views(dev, kt, vt, st):
    """Views one element off a 256-byte boundary (and 16 bytes less one element) of each array in turn and of all."""
    ks, ss = np.dtype(_NP[kt]).itemsize, np.dtype(_NP[st]).itemsize
    vs = np.dtype(_NP[vt]).itemsize if vt else 4
    T = tile_of(dev, kt, vt)
    n = 2 * T + 3
    o = lambda es: [es, 16 - es] if es < 8 else [8, 24]
    cases = []
    for which, es in enumerate((ks, vs, ss)):
        for off in o(es):
            c = [0, 0, 0]
            c[which] = off
            cases.append(tuple(c))
    cases.append((o(ks)[0], o(vs)[1], o(ss)[0]))
    L = lds_bins(dev, st)
    for nb in (100, L + 1):
        keys = make_keys(kt, "uniform", n, 2, 0, min(nb + 9, 250 if ks == 1 else nb + 9), seed=7)
        values = make_values(vt, n, 9)
        want = None
        for offs in cases:
            want = run_case(dev, kt, vt, st, keys, values, 2, 0, nb, "%s %s->%s offsets %s bins=%d" % (kt, vt, st, offs, nb), offs=offs, want=want)


def test_histogram_then_scan_on_one_queue(dev):
    """The first half of a counting sort: bucket offsets = exclusive scan of the counts, no host wait in between."""
    clo, ctx, q = dev
    n, nb = (1 << 20) + 3, 4096
    keys = make_keys("uint", "skewed", n, 0, 3, nb, seed=2)
    kin, cnt, offs = Region(dev, n * 4, 0, keys, 0), Region(dev, nb * 4, 0, None, 2), Region(dev, nb * 4, 0, None, 1)
    h = clo.Histogram(ctx, "uint", None, "uint")
    s = clo.Scanner("blelloch", ctx, "uint", "uint")
    try:
        assert h.with_device_data(q, kin.view, None, cnt.view, n, lower=0, shift=3, num_bins=nb)
        assert s.with_device_data(q, cnt.view, offs.view, nb)
        q.finish()
        want = histogram(keys, None, np.uint32, 0, 3, nb)
        cnt.check(want, "counts")
        offs.check((np.cumsum(want, dtype=np.uint64) - want).astype(np.uint32), "bucket offsets")
        kin.check(keys, "keys_in")
    finally:
        h.close()
        s.close()
        for x in (kin, cnt, offs):
            x.close()


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    L = lds_bins(dev, "ulong")
    obj = clo.Histogram(ctx, "uint", "uint", "ulong")
    for n, nb, shift, layout in (((1 << 22) + 1, L + 5, 0, "uniform"), (5, 3, 0, "edges"), ((1 << 16) + 1, 256, 9, "skewed"),
                                 ((1 << 22) + 7, 1 << 20, 2, "sorted"), (100, L, 0, "equal"), ((1 << 21) + 3, 17, 20, "uniform")):
        keys = make_keys("uint", layout, n, 42, shift, nb, seed=n)
        run_case(dev, "uint", "uint", "ulong", keys, make_values("uint", n, n), 42, shift, nb, "reuse n=%d bins=%d %s" % (n, nb, layout), obj=obj)
    obj.close()


def test_host_data_form(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "short", "int")
    n = 3 * T + 17
    keys = make_keys("short", "uniform", n, -300, 1, 400, seed=3)
    values = make_values("int", n, 4)
    h = clo.Histogram(ctx, "short", "int", "long")
    want = histogram(keys, values, np.int64, -300, 1, 333)
    for qe in (q, None):
        got = h.with_host_data(keys, values, lower=-300, shift=1, num_bins=333, q_exec=qe)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    h.close()
    h = clo.Histogram(ctx, "short", "int", "long", options="accumulate")
    out = np.arange(333, dtype=np.int64)
    h.with_host_data(keys, values, lower=-300, shift=1, num_bins=333, out=out)
    assert np.array_equal(out, want + np.arange(333))
    h.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 elements; the transfers on a queue of their own, then no queue at all (the call makes and destroys
    one); plain and accumulating, which uploads the output first."""
    clo, ctx, q = dev
    n = 2 * tile_of(dev, "short", "int") + 1
    keys = make_keys("short", "uniform", n, -300, 1, 400, seed=5)
    values = make_values("int", n, 6)
    want = histogram(keys, values, np.int64, -300, 1, 333)
    qc = clo.Queue(ctx)
    try:
        for options in (None, "accumulate"):
            h = clo.Histogram(ctx, "short", "int", "long", options=options)
            for qe, qcomm in ((q, qc), (None, None)):
                out = np.arange(333, dtype=np.int64)
                h.with_host_data(keys, values, lower=-300, shift=1, num_bins=333, out=out, q_exec=qe, q_comm=qcomm)
                assert np.array_equal(out, want + np.arange(333) if options else want), (options, qe is None, qcomm is None)
            h.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib, CLO_HIP_EARGS, CLO_HIP_EUNSUPPORTED
    n, nb = 100000, 64
    k, v, o = (clo.Buffer(ctx, b) for b in (n * 8, n * 8, nb * 8 + 64))
    o.write(q, np.full(nb * 8 + 64, 0x5A, np.uint8))
    call = lambda keys=k.ptr, vals=v.ptr, out=o.ptr, numel=n, ks=4, vt=5, st=5, shift=0, bins=nb: lib.clo_hip_histogram(
        keys, vals, out, numel, ks, 0, vt, st, 0, shift, bins, 0, 0, None, 0, q.stream)
    assert call(out=None) == CLO_HIP_EARGS
    assert call(out=o.ptr + 2) == CLO_HIP_EARGS                      # hist_out: aligned to the sum type
    assert call(out=o.ptr + 4, st=7) == CLO_HIP_EARGS
    assert call(bins=0) == CLO_HIP_EARGS
    assert call(bins=1 << 32) == CLO_HIP_EARGS
    assert call(numel=1 << 32) == CLO_HIP_EARGS
    assert call(shift=32) == CLO_HIP_EARGS
    assert call(ks=1, shift=8) == CLO_HIP_EARGS
    assert call(keys=None) == CLO_HIP_EARGS
    assert call(keys=k.ptr + 2) == CLO_HIP_EARGS                     # keys and values: aligned to their element
    assert call(vals=v.ptr + 4, vt=7, st=7) == CLO_HIP_EARGS
    for kw in (dict(ks=3), dict(ks=16), dict(vt=9), dict(st=9), dict(st=10), dict(vt=3), dict(vt=7, st=5), dict(st=8), dict(st=11),
               dict(vals=None, st=3)):
        assert call(**kw) == CLO_HIP_EUNSUPPORTED, kw
    q.finish()
    assert (o.read(q, np.uint8, nb * 8 + 64) == 0x5A).all()           # none of them touched hist_out
    assert call(numel=0, keys=None, vals=None) == 0                   # numel 0: the fill alone
    q.finish()
    got = o.read(q, np.uint8, nb * 8 + 64)
    assert not got[:nb * 4].any() and (got[nb * 4:] == 0x5A).all()
    assert lib.clo_hip_histogram(None, None, o.ptr, 0, 4, 0, 5, 5, 0, 0, nb, 1, 0, None, 0, q.stream) == 0   # accumulating: nothing at all
    q.finish()
    assert (o.read(q, np.uint8, nb * 8 + 64)[nb * 4:] == 0x5A).all()
    for x in (k, v, o):
        x.close()
