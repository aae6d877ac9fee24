"""CloBucket (include/clo_bucket.h) on the GPU against the numpy model of tests/bucket_model.py, bit for bit. Every array
is a view inside a larger allocation with guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs are pre-filled with the pattern, and after every call the rows and the offsets equal
the model's and the guards and every input are unchanged. With T = bucket_tile: sizes around the tile edges x bin counts
on both sides of the one-pass / two-pass border; the row patterns (one bin, the rest alone, below lower, bins descending
by row, alternating, uniform, 90 % in one bin, one row of the rest at every tile edge); shift 0 and B - 1; lower
non-zero, negative, and with a range that runs past the type's maximum; every form, both count types, all eight key
types; element-aligned views; one object large, small, large; two objects on two streams; the host-data form; the thin
ABI's status codes; the counter scan's capacities; the offsets chained into SegSort and SegReduce with no host wait; the
histogram's counts; clo_hip_bucket captured into a graph and replayed on changed keys; indices above 2^31."""
import numpy as np
import pytest

from bucket_model import COUNT_NP, bin_or_rest, bucket
from test_gpu_histogram import Region, key_at

pytestmark = pytest.mark.gpu

NP = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
      "long": np.int64, "ulong": np.uint64}
KEY_TYPES = tuple(NP)
# value forms: keys only; 4-byte values; 8-byte values; indices with keys_out; indices alone
_VS = {"keys": 0, "v4": 4, "v8": 8, "arg": 4, "arg_only": 4}
MODES = tuple(_VS)
SIZES = lambda T: (0, 1, 63, 64, 65, T - 1, T, T + 1, 2 * T + 1, 5 * T + 3)
BIN_COUNTS = (1, 2, 3, 255, 256, 257, 4096, 65535)
PATTERNS = ("one bin", "all rest", "all below", "descending", "alternating", "uniform", "90 % in one", "rest at tile edges")


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def tile_of(dev, kt, mode="keys"):
    t = dev[0].bucket_tile(np.dtype(NP[kt]).itemsize, _VS[mode])
    assert t > 0 and t % 1024 == 0
    return t


def values_for(mode, n):
    """Values that carry the row's index; the 8-byte ones with a non-zero high word that differs per row."""
    if mode == "v4":
        return np.arange(n, dtype=np.uint32) ^ np.uint32(0x5A000000)
    if mode == "v8":
        i = np.arange(n, dtype=np.uint64)
        return ((np.uint64(0xC0DE0000) + (i * np.uint64(2654435761) & np.uint64(0xFFFF))) << np.uint64(32)) | i
    return None


def bins_of_pattern(pattern, n, T, num_bins, seed):
    """The bin of every row; num_bins: the rest above the range, -1: below lower."""
    rng = np.random.default_rng(seed)
    i = np.arange(n, dtype=np.int64)
    if pattern == "one bin":
        return np.full(n, num_bins // 2, np.int64)
    if pattern == "all rest":
        return np.full(n, num_bins, np.int64)
    if pattern == "all below":
        return np.full(n, -1, np.int64)
    if pattern == "descending":                                     # the first row into the last bin: every row moves the farthest
        return (n - 1 - i) * num_bins // max(n, 1)
    if pattern == "alternating":
        return np.where(i % 2 == 0, num_bins - 1, 0)
    if pattern == "uniform":
        return rng.integers(-1, num_bins + 1, n)
    if pattern == "90 % in one":
        return np.where(rng.random(n) < 0.9, num_bins // 3, rng.integers(-1, num_bins + 1, n))
    assert pattern == "rest at tile edges"
    b = rng.integers(0, num_bins, n)
    b[(i % T == 0) | (i % T == T - 1)] = num_bins
    return b


def keys_for(kt, b, num_bins, lower, shift, seed):
    """Keys of type kt whose bins are b (num_bins: above the range, -1: below lower; each replaced by the other where
    the type has no such key, and by bin 0 where it has neither), with random bits below the shift."""
    rng = np.random.default_rng(seed)
    info = np.iinfo(NP[kt])
    b = np.asarray(b, np.int64).copy()
    above_ok = int(lower) + (num_bins << shift) <= info.max
    below_ok = int(lower) > info.min
    if not above_ok:
        b[b == num_bins] = -1 if below_ok else 0
    if not below_ok:
        b[b == -1] = num_bins if above_ok else 0
    low = rng.integers(0, 1 << shift, b.size, dtype=np.uint64) if shift else np.zeros(b.size, np.uint64)
    d = (b.astype(np.uint64) << np.uint64(shift)) + low             # (b == -1 wraps; replaced below)
    d = np.minimum(d, np.uint64(info.max - int(lower)))             # the last bin the type reaches may be cut short
    room_above = info.max - int(lower) - (num_bins << shift) if above_ok else 0
    d = np.where(b == num_bins, (np.uint64(num_bins) << np.uint64(shift)) + rng.integers(0, min(room_above, 1000) + 1, b.size, dtype=np.uint64), d)
    room_below = int(lower) - info.min - 1 if below_ok else 0
    d = np.where(b == -1, (-1 - rng.integers(0, min(room_below, 1000) + 1, b.size, dtype=np.int64)).view(np.uint64), d)
    keys = key_at(kt, lower, d)
    want = np.where(b == -1, num_bins, b)
    assert np.array_equal(bin_or_rest(keys, lower, shift, num_bins), want), "the keys do not have the bins asked for"
    return keys


def run_bucket(dev, kt, keys, mode, num_bins, lower=0, shift=0, ct="uint", what="", offs=(0, 0, 0, 0, 0), obj=None, q=None):
    """One call on views at byte offsets offs = (keys_in, values_in, keys_out, values_out, offsets_out); checks
    everything and returns the model's offsets."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    dt = np.dtype(NP[kt])
    keys = np.ascontiguousarray(keys, dtype=dt)
    n, vs, cs = keys.size, _VS[mode], np.dtype(COUNT_NP[ct]).itemsize
    what = "%s %s %s, %d bins, lower %d, shift %d, n = %d, %s" % (kt, mode, ct, num_bins, lower, shift, n, what)
    vals = values_for(mode, n)
    s = obj or clo.Bucket(ctx, kt, vs, ct)
    k_r = Region(rdev, keys.nbytes, offs[0], keys, 0)
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if vals is not None else None
    ko_r = Region(rdev, n * dt.itemsize, offs[2], None, 2) if mode != "arg_only" else None
    vo_r = Region(rdev, n * vs, offs[3], None, 2) if vs else None
    of_r = Region(rdev, (num_bins + 1) * cs, offs[4], None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert s.with_device_data(q, k_r.view, view(v_r), view(ko_r), view(vo_r), of_r.view, n, lower, shift, num_bins), what
        q.finish()
        want_k, want_v, perm, want_off = bucket(keys, vals, lower, shift, num_bins, ct)
        of_r.check(want_off, what + ": offsets_out")
        if ko_r:
            ko_r.check(want_k, what + ": keys_out")
        if vo_r:
            vo_r.check(want_v if vals is not None else perm, what + ": values_out")   # the model's permutation itself
        k_r.check(keys, what + ": keys_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return want_off
    finally:
        for r in (k_r, v_r, ko_r, vo_r, of_r):
            if r:
                r.close()
        if obj is None:
            s.close()


@pytest.mark.parametrize("num_bins", BIN_COUNTS)
def test_sizes_and_bin_counts(dev, num_bins):
    """The ten sizes x this bin count; the patterns, the value forms and the count types take turns."""
    T = tile_of(dev, "uint")
    for j, n in enumerate(SIZES(T)):
        pattern = PATTERNS[(j + num_bins) % len(PATTERNS)]
        mode = MODES[(j + num_bins // 3) % len(MODES)]
        b = bins_of_pattern(pattern, n, T, num_bins, 100 * num_bins + j)
        keys = keys_for("uint", b, num_bins, 1000, 0, j)
        run_bucket(dev, "uint", keys, mode, num_bins, 1000, 0, ("uint", "ulong")[j % 2], pattern)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_patterns(dev, pattern):
    """Every pattern at 2 T + 1 and 5 T + 3 rows with 3, 255, 256 and 4096 bins, as indices with the keys and alone."""
    T = tile_of(dev, "uint", "arg")
    for j, num_bins in enumerate((3, 255, 256, 4096)):
        n = (2 * T + 1, 5 * T + 3)[j % 2]
        b = bins_of_pattern(pattern, n, T, num_bins, 7 + j)
        keys = keys_for("uint", b, num_bins, 77, 3, 50 + j)
        run_bucket(dev, "uint", keys, ("arg", "arg_only")[j % 2], num_bins, 77, 3, what=pattern)


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types_shifts_and_lowers(dev, kt):
    """Every key type: shift 0 and B - 1; lower 0, non-zero, negative for signed keys, the type's minimum, and one under
    which lower + (num_bins << shift) lies past the type's maximum, with keys below lower that the wrapped difference
    would put in range."""
    info = np.iinfo(NP[kt])
    B = 8 * np.dtype(NP[kt]).itemsize
    T = tile_of(dev, kt, "v8")
    n = 2 * T + 5
    case = 0
    for num_bins in (3, 255, 256, 1000):
        lowers = [0, 5, info.min, info.max - 40] + ([-7, -100] if info.min < 0 else [])
        for lower in lowers:
            for shift in (0, 2, B - 1):
                mode = MODES[case % len(MODES)]
                ct = ("uint", "ulong")[case % 2]
                case += 1
                # the bins the type can reach from this lower at this shift
                reach = min(num_bins, ((info.max - lower) >> shift) + 1)
                b = np.random.default_rng(case).integers(-1, num_bins + 1, n)
                b = np.where((b >= reach) & (b < num_bins), b % reach, b)
                keys = keys_for(kt, b, num_bins, lower, shift, case)
                run_bucket(dev, kt, keys, mode, num_bins, lower, shift, ct)
    # raw keys over the type's whole range, whatever bins they fall in: the range runs past the maximum
    rng = np.random.default_rng(3)
    keys = rng.integers(info.min, info.max, n, dtype=NP[kt], endpoint=True)
    for num_bins, shift in ((200, max(B - 8, 0)), (65535, max(B - 16, 0)), (300, 0)):
        lower = info.max - (100 << shift)
        run_bucket(dev, kt, keys, "arg", num_bins, lower, shift, what="raw keys, a range past the maximum")
        run_bucket(dev, kt, keys, "v4", num_bins, info.min, shift, what="raw keys from the minimum")


@pytest.mark.parametrize("mode", MODES)
def test_every_form_and_count_type(dev, mode):
    for ct in ("uint", "ulong"):
        for kt in ("uchar", "ushort", "uint", "ulong"):
            T = tile_of(dev, kt, mode)
            for num_bins in (16, 300):
                n = 3 * T + 9
                b = bins_of_pattern("uniform", n, T, min(num_bins, 200), 11)
                keys = keys_for(kt, b, min(num_bins, 200), 3, 0, 12)        # uchar: the bins it has
                run_bucket(dev, kt, keys, mode, num_bins, 3, 0, ct)


def test_element_aligned_views(dev):
    """Every array one element past a 16-byte boundary: nothing may assume more than the element's alignment."""
    cases = (("uchar", "v8", (1, 8, 1, 8, 4)), ("char", "arg", (1, 0, 1, 4, 4)), ("ushort", "v4", (2, 4, 2, 4, 4)), ("uint", "keys", (4, 0, 4, 0, 4)),
             ("uint", "v4", (4, 4, 4, 4, 4)), ("int", "arg", (4, 0, 4, 4, 4)), ("ulong", "v8", (8, 8, 8, 8, 8)), ("long", "arg_only", (8, 0, 0, 4, 8)),
             ("short", "keys", (2, 0, 2, 0, 4)))
    for i, (kt, mode, offs) in enumerate(cases):
        T = tile_of(dev, kt, mode)
        n = 2 * T + 37
        for num_bins in (100, 700):
            reach = min(num_bins, 120)
            b = np.random.default_rng(i).integers(-1, reach + 1, n)
            b[b == reach] = num_bins
            keys = keys_for(kt, b, num_bins, 1, 0, 8 + i)
            run_bucket(dev, kt, keys, mode, num_bins, 1, 0, "ulong" if offs[4] == 8 else "uint", "views at %s" % (offs,), offs=offs)


def test_one_object_large_small_large(dev):
    """The workspace grows, is reused by a smaller call, and grows again; one and two passes on the same object."""
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    s = clo.Bucket(ctx, "uint", 4)
    try:
        for j, (n, num_bins) in enumerate(((40 * T + 3, 200), (5, 3), (0, 3), (30 * T + 1, 5000), (70 * T + 7, 255), (3 * T, 65535))):
            b = bins_of_pattern(PATTERNS[j % len(PATTERNS)], n, T, num_bins, j)
            keys = keys_for("uint", b, num_bins, 9, 1, 30 + j)
            run_bucket(dev, "uint", keys, "v4" if j % 2 == 0 else "arg", num_bins, 9, 1, what="call %d" % j, obj=s)
    finally:
        s.close()


def test_two_objects_on_two_streams(dev):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds."""
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    n = 150 * T + 9
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("v4", 200), ("arg", 3000))
    objs = [clo.Bucket(ctx, "uint", 4) for _ in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (mode, num_bins) in enumerate(specs):
                keys = keys_for("uint", bins_of_pattern("uniform", n, T, num_bins, 10 * rnd + i), num_bins, 0, 2, 50 + 10 * rnd + i)
                vals = values_for(mode, n)
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, keys.nbytes, 0, keys, 0), Region(rdev, vals.nbytes, 0, vals, 1) if vals is not None else None,
                        Region(rdev, keys.nbytes, 0, None, 2), Region(rdev, 4 * n, 0, None, 2), Region(rdev, 4 * (num_bins + 1), 0, None, 1)]
                sent.append((keys, vals, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (keys, vals, regs) in enumerate(sent):
                view = lambda r: r.view if r is not None else None
                assert objs[i].with_device_data(qs[i], regs[0].view, view(regs[1]), regs[2].view, regs[3].view, regs[4].view, n, 0, 2, specs[i][1])
            for i in range(2):
                qs[i].finish()
            for i, (keys, vals, regs) in enumerate(sent):
                wk, wv, perm, woff = bucket(keys, vals, 0, 2, specs[i][1])
                what = "round %d, object %d" % (rnd, i)
                regs[4].check(woff, what + ": offsets_out")
                regs[2].check(wk, what + ": keys_out")
                regs[3].check(wv if vals is not None else perm, what + ": values_out")
                for r in regs:
                    if r:
                        r.close()
    finally:
        for x in objs + qs:
            x.close()


@pytest.mark.parametrize("mode", MODES)
def test_host_data_form(dev, mode):
    """The host-data form on the caller's queue, with a queue of its own for the transfers, and with no queue at all."""
    clo, ctx, q = dev
    T = tile_of(dev, "int", mode)
    n = 2 * T + 9
    qc = clo.Queue(ctx)
    try:
        for ct in ("uint", "ulong"):
            for num_bins in (40, 900):
                keys = keys_for("int", bins_of_pattern("uniform", n, T, num_bins, 1), num_bins, -50, 1, 2)
                vals = values_for(mode, n)
                s = clo.Bucket(ctx, "int", _VS[mode], ct)
                for qe, qcomm in ((q, None), (q, qc), (None, None)):
                    ko, vo, off = s.with_host_data(keys, vals, -50, 1, num_bins, keys_out=mode != "arg_only", q_exec=qe, q_comm=qcomm)
                    wk, wv, perm, woff = bucket(keys, vals, -50, 1, num_bins, ct)
                    assert (ko is None) == (mode == "arg_only") and (vo is None) == (mode == "keys")
                    assert off.dtype == woff.dtype and np.array_equal(off, woff)
                    if ko is not None:
                        assert np.array_equal(ko, wk)
                    if vo is not None:
                        assert np.array_equal(vo, wv if vals is not None else perm)
                s.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    n = 1000
    need = lib.clo_hip_bucket_workspace_bytes(n, 4, 4, 300)
    assert need > 0 and need % 256 == 0 and need >= lib.clo_hip_bucket_workspace_bytes(n, 4, 4, 255) > 0
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 400, 2 * n + 4, dtype=np.uint32)
    ki = Region(dev, 8 * n + 16, 0, keys, 0)
    vi, ko, vo = (Region(dev, 16 * n + 16, 0, None, i) for i in range(3))
    off = Region(dev, 8 * 70000, 0, None, 0)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(k_p, v_p, ko_p, vo_p, off_p=off.ptr, numel=n, ks=4, sg=0, vs=4, cs=4, lower=0, shift=0, bins=300, w=ws.ptr, wb=need):
        return lib.clo_hip_bucket(k_p, v_p, ko_p, vo_p, off_p, numel, ks, sg, vs, cs, lower, shift, bins, w, wb, s)

    try:
        full = (ki.ptr, vi.ptr, ko.ptr, vo.ptr)
        for bins in (0, 65536, 1 << 20):
            assert call(*full, bins=bins) == EARGS, bins
        for ks, vs in ((3, 4), (16, 4), (0, 0), (4, 2), (4, 16)):
            assert call(*full, ks=ks, vs=vs) == EUNSUPPORTED, (ks, vs)
            assert lib.clo_hip_bucket_tile(ks, vs) == 0 and lib.clo_hip_bucket_workspace_bytes(n, ks, vs, 300) == 0
        for cs in (0, 2, 16):
            assert call(*full, cs=cs) == EUNSUPPORTED
        assert call(*full, shift=32) == EARGS and call(*full, shift=8, ks=1) == EARGS
        assert call(*full, off_p=None) == EARGS and call(*full, off_p=off.ptr + 2) == EARGS and call(*full, off_p=off.ptr + 4, cs=8) == EARGS
        assert call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, ko.ptr, vo.ptr) == EARGS                                              # the keys are read
        assert call(ki.ptr, vi.ptr, ko.ptr, None) == EARGS                                              # values_out with value_size 4
        assert call(ki.ptr, vi.ptr, None, vo.ptr) == EARGS                                              # keys_out outside the arg form
        assert call(ki.ptr, None, None, None, vs=0) == EARGS
        assert call(ki.ptr, None, ko.ptr, vo.ptr, vs=8) == EARGS                                        # the arg form is 4-byte
        assert call(ki.ptr, vi.ptr, ko.ptr, None, vs=0) == EARGS and call(ki.ptr, None, ko.ptr, vo.ptr, vs=0) == EARGS   # values with value_size 0
        for i in range(4):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        args = list(full)
        args[1] += 4
        assert call(*args, vs=8) == EARGS                                                               # 4-aligned is not 8-aligned
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: off by 64, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short by a byte
        assert call(*full, wb=lib.clo_hip_bucket_workspace_bytes(n, 4, 4, 255)) == EWORKSPACE           # what one pass needs is not what two need
        q.finish()
        for r in (ko, vo, off):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size, one pass and two; numel 0 needs no workspace and
        # no inputs, and still writes the offsets
        for bins in (300, 255):
            wb = lib.clo_hip_bucket_workspace_bytes(n, 4, 4, bins)
            assert call(*full, bins=bins, wb=wb, cs=8) == 0
            q.finish()
            got = off.base.read(q, np.uint8, off.host.size)[off.at:off.at + 8 * (bins + 1)].view(np.uint64)
            assert np.array_equal(got, bucket(keys[:n], None, 0, 0, bins, "ulong")[3])
        assert call(None, None, ko.ptr, None, vs=0, numel=0, bins=7, w=None, wb=0) == 0
        q.finish()
        assert not off.base.read(q, np.uint8, off.host.size)[off.at:off.at + 32].any()
    finally:
        ws.close()
        for r in (ki, vi, ko, vo, off):
            r.close()


def test_the_counter_scan_crosses_a_group(dev):
    """The counter scan gives BUCKET_SCAN_GROUP counters (digits x tiles) to a work-group: with 256 digits the 17th tile
    is the first whose counters a second group takes; with 3 bins (4 digits) it is tile 1025."""
    clo = dev[0]
    T = tile_of(dev, "uint")
    G = clo.BUCKET_SCAN_GROUP
    for num_bins, mode in ((255, "arg"), (4000, "v4"), (3, "arg_only")):
        digits = min(num_bins + 1, 256)
        n = (G // digits) * T + 1
        assert -(-n // T) * digits > G >= (-(-(n - 1) // T)) * digits                  # the smallest numel that crosses it
        b = bins_of_pattern("uniform", n, T, num_bins, num_bins)
        run_bucket(dev, "uint", keys_for("uint", b, num_bins, 0, 0, 1), mode, num_bins, what="%d counters" % (-(-n // T) * digits))


def test_the_counter_scan_takes_a_second_trip(dev):
    """The one work-group that scans the groups' sums takes BUCKET_SCAN_TRIP of them per trip: 256 digits x 32 769 tiles
    is the smallest input with one sum more. uchar keys are their own bins; the indices alone."""
    clo = dev[0]
    T = tile_of(dev, "uchar", "arg_only")
    n = clo.BUCKET_SCAN_GROUP * clo.BUCKET_SCAN_TRIP // 256 * T + 1
    assert -(-(-(-n // T) * 256) // clo.BUCKET_SCAN_GROUP) == clo.BUCKET_SCAN_TRIP + 1
    keys = np.random.default_rng(9).integers(0, 256, n, dtype=np.uint8)
    run_bucket(dev, "uchar", keys, "arg_only", 255, 0, 0, what="%d tiles" % -(-n // T))


def test_offsets_chain_into_segsort_and_segreduce(dev):
    """bucket -> SegSort(form="offsets") -> SegReduce(form="offsets") on one queue with no host wait in between: the rows
    sorted by value inside every bin, and the sum of the values of every bin; against the numpy composition."""
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    n = 9 * T + 5
    rng = np.random.default_rng(21)
    for num_bins, ct in ((37, "uint"), (1500, "ulong")):
        cdt = COUNT_NP[ct]
        keys = keys_for("uint", bins_of_pattern("uniform", n, T, num_bins, 3), num_bins, 10, 4, 4)
        vals = rng.integers(0, 1 << 20, n, dtype=np.uint32)
        k_r, v_r = Region(dev, 4 * n, 0, keys, 0), Region(dev, 4 * n, 0, vals, 1)
        ko_r, vo_r = Region(dev, 4 * n, 0, None, 2), Region(dev, 4 * n, 0, None, 2)
        of_r = Region(dev, (num_bins + 1) * np.dtype(cdt).itemsize, 0, None, 1)
        so_r, sv_r = Region(dev, 4 * n, 0, None, 0), Region(dev, 4 * n, 0, None, 0)
        ag_r, n1_r, n2_r = Region(dev, 8 * num_bins, 0, None, 1), Region(dev, 8, 0, None, 2), Region(dev, 8, 0, None, 2)
        bk = clo.Bucket(ctx, "uint", 4, ct)
        srt = clo.SegSort("offsets", ctx, "uint", 4, ct)                 # sorts the VALUES of every bin, the keys riding along
        red = clo.SegReduce("sum", "offsets", ctx, "uint", "ulong", ct)
        try:
            assert bk.with_device_data(q, k_r.view, v_r.view, ko_r.view, vo_r.view, of_r.view, n, 10, 4, num_bins)
            assert srt.with_device_data(q, of_r.view, None, vo_r.view, ko_r.view, sv_r.view, so_r.view, n1_r.view, num_bins, n)
            assert red.with_device_data(q, of_r.view, None, vo_r.view, ag_r.view, n2_r.view, num_bins, n)
            q.finish()
            wk, wv, _, woff = bucket(keys, vals, 10, 4, num_bins, ct)
            total = int(woff[-1])
            assert 0 < total < n
            of_r.check(woff, "offsets_out")
            sk, sv = wk[:total].copy(), wv[:total].copy()
            sums = np.zeros(num_bins, np.uint64)
            for b in range(num_bins):
                lo, hi = int(woff[b]), int(woff[b + 1])
                o = np.argsort(wv[lo:hi], kind="stable")
                sv[lo:hi], sk[lo:hi] = wv[lo:hi][o], wk[lo:hi][o]
                sums[b] = wv[lo:hi].astype(np.uint64).sum()
            n1_r.check(np.array([total], np.uint64), "segsort: num_out")
            n2_r.check(np.array([total], np.uint64), "segreduce: num_out")
            sv_r.check(sv, "segsort: the values of every bin, sorted")
            so_r.check(sk, "segsort: their keys")
            ag_r.check(sums, "segreduce: the sums of the bins")
        finally:
            for x in (k_r, v_r, ko_r, vo_r, of_r, so_r, sv_r, ag_r, n1_r, n2_r, bk, srt, red):
                x.close()


def test_offsets_are_the_histogram(dev):
    """np.diff(offsets_out) is this library's Histogram of the same keys under the same mapping."""
    clo, ctx, q = dev
    T = tile_of(dev, "short")
    n = 6 * T + 11
    keys = np.random.default_rng(8).integers(-32768, 32767, n, dtype=np.int16, endpoint=True)
    for num_bins, lower, shift in ((200, -3000, 5), (255, -32768, 8), (256, -32768, 8), (5000, 10, 2), (65535, -32768, 0)):
        h = clo.Histogram(ctx, "short")
        counts = h.with_host_data(keys, None, lower, shift, num_bins, q_exec=q)
        h.close()
        b = clo.Bucket(ctx, "short", 4)
        _, _, off = b.with_host_data(keys, None, lower, shift, num_bins, q_exec=q)
        b.close()
        assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), counts.astype(np.int64)), (num_bins, lower, shift)
        assert np.array_equal(off, run_bucket(dev, "short", keys, "keys", num_bins, lower, shift))


@pytest.mark.parametrize("mode,num_bins", [("keys", 100), ("v4", 255), ("arg", 256), ("arg_only", 3000)])
def test_graph_capture_and_replay(dev, mode, num_bins):
    """clo_hip_bucket captured from one client stream (a linear graph) after one eager warm-up and replayed three times,
    the keys rewritten and the outputs refilled with a canary before each replay (the protocol of
    test_gpu_graph_capture.py): the rows and the offsets follow the buffers."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T = tile_of(dev, "uint", mode)
    n, vs = 3 * T + 5, _VS[mode]
    valued = mode == "v4"
    need = lib.clo_hip_bucket_workspace_bytes(n, 4, vs, num_bins)
    made = [GC.Mem(gdev, x) for x in (4 * n, 4 * n, 4 * n, 4 * n, 4 * (num_bins + 1), need)]
    ki, vi, ko, vo, off, ws = made
    vals = values_for("v4", n)
    seen = set()

    def load(r):
        keys = keys_for("uint", bins_of_pattern(PATTERNS[(3 + 2 * r) % len(PATTERNS)], n, T, num_bins, 200 + r), num_bins, 6, 1, r)
        for m in (ko, vo, off):
            m.fill()
        ki.put(keys)
        vi.put(vals)
        want = (keys,) + bucket(keys, vals if valued else None, 6, 1, num_bins)
        seen.add(want[4].tobytes())
        return want

    def enqueue():
        return lib.clo_hip_bucket(ki.ptr, vi.ptr if valued else None, ko.ptr if mode != "arg_only" else None, vo.ptr if vs else None, off.ptr, n,
                                  4, 0, vs, 4, 6, 1, num_bins, ws.ptr, need, q.stream)

    def verify(r, want):
        keys, wk, wv, perm, woff = want
        tag = "%s, %d bins, round %d" % (mode, num_bins, r)
        GC.same(off.get(np.uint32, num_bins + 1), woff, tag + ": offsets_out")
        GC.same(ko.get(np.uint32, n), wk if mode != "arg_only" else GC.canary(np.uint32, n), tag + ": keys_out")
        GC.same(vo.get(np.uint32, n), (wv if valued else perm) if vs else GC.canary(np.uint32, n), tag + ": values_out")
        GC.same(ki.get(np.uint32, n), keys, tag + ": keys_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(seen) >= 4, len(seen)                                # the offsets differed between the replays
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def test_indices_above_2p31(dev):
    """numel = 2^31 + T + 3 uchar keys into 3 bins and the rest, the indices alone, checked on the device: the offsets
    are torch's counts; every row's key has the bin of the bucket the row lies in; and inside every bucket the indices
    ascend strictly. Together: the model's permutation. The head and the tail of every bucket are compared with the
    first and the last indices torch finds for it, the latter above 2^31."""
    import torch
    clo, ctx, q = dev
    T = tile_of(dev, "uchar", "arg_only")
    n = (1 << 31) + T + 3
    free = torch.cuda.mem_get_info()[0]
    if free < (24 << 30):
        pytest.skip("needs about 20 GiB of free device memory (2 GiB of keys, 8 GiB of indices, torch's scratch), %.1f GiB are free" % (free / 2 ** 30))
    lower, shift, num_bins = 10, 4, 3
    g = torch.Generator(device="cuda").manual_seed(31)
    keys = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        keys[lo:hi] = torch.randint(0, 100, (hi - lo,), dtype=torch.uint8, device="cuda", generator=g)

    def bins(k):                                                        # CloHistogram's mapping, the rest as bin num_bins
        d = k.to(torch.int32) - lower
        b = d >> shift
        return torch.where((d >= 0) & (b < num_bins), b, torch.full_like(b, num_bins))

    counts = torch.zeros(num_bins + 1, dtype=torch.int64, device="cuda")
    for lo in range(0, n, step):
        counts += torch.bincount(bins(keys[lo:min(lo + step, n)]), minlength=num_bins + 1)
    want_off = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts, 0)))
    assert int(want_off[-1]) == n
    out = torch.full((n,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")
    off = torch.full((num_bins + 1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    as_buffer = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
    bufs = [as_buffer(t) for t in (keys, out, off)]
    s = clo.Bucket(ctx, "uchar", 4, "ulong")
    try:
        assert s.with_device_data(q, bufs[0], None, None, bufs[1], bufs[2], n, lower, shift, num_bins)
        q.finish()
        assert bool((off == want_off[:num_bins + 1]).all()), (off.tolist(), want_off.tolist())
        edges = [int(x) for x in want_off.tolist()]
        first, last = bins(keys[:1 << 20]), bins(keys[(1 << 31) + 1:])                                  # the last T + 2 rows
        for b in range(num_bins + 1):
            lo_b, hi_b = edges[b], edges[b + 1]
            assert hi_b - lo_b > (1 << 28)
            for lo in range(lo_b, hi_b, step):
                hi = min(lo + step, hi_b)
                idx = out[lo:hi].to(torch.int64) & 0xFFFFFFFF                                           # the indices are uint
                assert bool((idx[1:] > idx[:-1]).all()), "bucket %d: the indices do not ascend" % b
                if lo > lo_b:
                    assert int(idx[0]) > (int(out[lo - 1]) & 0xFFFFFFFF)
                assert bool((bins(keys[idx]) == b).all()), "bucket %d holds a row of another bin" % b
                del idx
            head = torch.nonzero(first == b).flatten()[:1000]
            tail = torch.nonzero(last == b).flatten()[-300:] + ((1 << 31) + 1)
            assert head.numel() == 1000 and tail.numel() == 300 and int(tail[0]) > (1 << 31)
            assert bool(((out[lo_b:lo_b + 1000].to(torch.int64) & 0xFFFFFFFF) == head).all()), "bucket %d: its head" % b
            assert bool(((out[hi_b - 300:hi_b].to(torch.int64) & 0xFFFFFFFF) == tail).all()), "bucket %d: its tail" % b
    finally:
        for x in bufs + [s]:
            x.close()
        del keys, out
        torch.cuda.empty_cache()
