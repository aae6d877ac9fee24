"""The order in which cl_ops_amd/csrc/hip/clo_hip_fscan.hip adds, restated in numpy: what the reduce / scan the tile
sums / apply launches of `fs_scan` compute for any pair of types clo_hip_scan_exclusive_typed accepts, bit for bit.
Every addition is done in the sum type (numpy adds two arrays of one type in that type; for half it adds in float32
and rounds to half once, which is the correctly rounded half sum because 24 >= 2 * 11 + 2). The contract:

  conversion     every element is converted to the sum type by a C cast, numpy's `astype` (a floating-point element
                 that an integer sum type cannot hold is undefined in C: callers stay inside the range);
  tile           256 threads x 16 consecutive elements; slots past the end of the array count as +0;
  thread sum     a thread adds its 16 elements left to right, starting from +0;
  wave scan      the 64 thread sums of a wave are scanned by the shuffle tree: for off = 1, 2, 4, 8, 16, 32 the lanes
                 with lane >= off do incl += incl[lane - off] (all of them on the values of the step before);
  wave sums      the inclusive value of lane 63; the four are added left to right from +0, which gives the base of
                 every wave and, after the fourth, the total of the tile;
  thread offset  base + (the inclusive value of the lane below, +0 for lane 0); never `incl - mine`;
  tile offset    added to that: (base + excl) + tile_excl, +0 where there is one tile only;
  outputs        the running value, then run += v[i], left to right;
  upper levels   the tile totals are scanned by the same procedure one level up (4096 totals per upper tile), with the
                 branches of fs_scan: one tile -> one launch; up to 4096 tiles -> their totals scanned as one tile; more
                 -> the totals reduced once more, those scanned as one tile, and applied on the way down.

For an integer sum type every order gives the same wrapped sums, so the model equals numpy_ops.scan_cast_expected
there (tests/test_fscan_model_cpu.py asserts it). The functions below are the steps, so that a test can replace one
of them by a deliberately different one and show that its inputs tell the two apart."""
import numpy as np

THREADS, ITEMS, WAVE = 256, 16, 64
WAVES = THREADS // WAVE
TILE = THREADS * ITEMS                     # 4096


def convert(a, sdt):
    """(sum type) element, as the kernel's C cast."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a).astype(sdt)


def in_tiles(v):
    """v padded with +0 to whole tiles, one plane per slot of a thread: p[i][tile, thread] (ITEMS, tiles, THREADS)."""
    tiles = -(-v.size // TILE)
    p = np.zeros(tiles * TILE, v.dtype)
    p[:v.size] = v
    return np.ascontiguousarray(p.reshape(tiles, THREADS, ITEMS).transpose(2, 0, 1))


def thread_sums(p):
    mine = np.zeros(p.shape[1:], p.dtype)
    for i in range(ITEMS):
        mine = mine + p[i]
    return mine


def wave_scan(mine):
    """Inclusive scan of every wave's thread sums by the shuffle tree: (tiles, WAVES, WAVE)."""
    incl = mine.reshape(-1, WAVES, WAVE).copy()
    off = 1
    while off < WAVE:
        incl[:, :, off:] = incl[:, :, off:] + incl[:, :, :-off]       # (the right side is evaluated before the store)
        off *= 2
    return incl


def block_parts(mine):
    """fs_block_exclusive: (base of every wave (tiles, WAVES, 1), exclusive value inside the wave (tiles, WAVES, WAVE),
    total of the tile (tiles,))."""
    incl = wave_scan(mine)
    run = np.zeros(incl.shape[0], mine.dtype)
    base = np.empty(incl.shape[:2] + (1,), mine.dtype)
    for w in range(WAVES):
        base[:, w, 0] = run
        run = run + incl[:, w, WAVE - 1]
    excl = np.zeros_like(incl)
    excl[:, :, 1:] = incl[:, :, :-1]
    return base, excl, run


def thread_offsets(base, excl, tile_excl):
    """(base + excl) + tile_excl: (tiles, THREADS)."""
    return (base + excl).reshape(-1, THREADS) + tile_excl[:, None]


def tile_parts(v):
    """What clo_fscan_reduce_kernel and clo_fscan_apply_kernel both compute of an array, with the same instructions
    in the same order (so the model computes it once per level): the padded elements and fs_block_exclusive's results."""
    p = in_tiles(v)
    return (p,) + block_parts(thread_sums(p))


def apply_parts(parts, n, tile_excl=None):
    """The rest of clo_fscan_apply_kernel: the tile's offset (+0 without one) folded into every thread's, then the
    running sums."""
    p, base, excl, _ = parts
    run = thread_offsets(base, excl, np.zeros(p.shape[1], p.dtype) if tile_excl is None else tile_excl)
    out = np.empty_like(p)
    for i in range(ITEMS):
        out[i] = run
        run = run + p[i]
    return out.transpose(1, 2, 0).reshape(-1)[:n]


def scan_converted(v):
    """fs_scan on elements already in the sum type."""
    if v.size == 0:
        return v.copy()
    with np.errstate(over="ignore", invalid="ignore"):        # (integer sums wrap, inf - inf is a NaN: both are results)
        level0 = tile_parts(v)
        t1 = level0[3].size                                    # the reduce launch: one total per tile
        if t1 <= 1:
            return apply_parts(level0, v.size)
        level1 = tile_parts(level0[3])
        t2 = level1[3].size
        if t2 <= 1:
            sums1 = apply_parts(level1, t1)
        else:
            level2 = tile_parts(level1[3])
            assert level2[3].size <= 1, "more than 2^36 elements: the library refuses"
            sums1 = apply_parts(level1, t1, apply_parts(level2, t2))
        return apply_parts(level0, v.size, sums1)


def scan(a, sdt):
    """The exclusive scan of `a` into sum type `sdt` with the bits the library gives."""
    return scan_converted(convert(a, np.dtype(sdt)))


# ---------------------------------------------------------------------------------------------------------------------
# the inputs and shapes of tests/test_gpu_float_scan.py; tests/test_fscan_model_cpu.py shows what they can tell apart
# ---------------------------------------------------------------------------------------------------------------------

SUM_TYPES = ("half", "float", "double")
NP = {"half": np.float16, "float": np.float32, "double": np.float64}
ONE_TILE = (1, 15, 16, 17, 63 * 16 + 1, 1024, 1025, 4095, 4096)
TWO_LEVELS = (4097, 8193, 64 * 4096 - 1, 64 * 4096 + 1, 1 << 24)      # (2^24: exactly one full upper tile)
THREE_LEVELS = ((1 << 24) + 1, (1 << 24) + 64 * 4096 + 17)
SIZES = ONE_TILE + TWO_LEVELS + THREE_LEVELS
TELESCOPE_BOUND = {"half": 1 << 10, "float": 1 << 23, "double": 1 << 52}


def telescoping_steps(st, n):
    """Integers d[0 .. n] in [0, B]: the input is a[i] = d[i + 1] - d[i]. Every partial sum of the tree is a sum over
    a contiguous range, d[r] - d[l], an integer of magnitude <= B that the sum type holds exactly: the scan is
    d[i] - d[0] whatever the order, and an element lost or counted twice shows at every position behind it."""
    return np.random.default_rng([1, np.dtype(NP[st]).itemsize, n]).integers(0, TELESCOPE_BOUND[st], n + 1, endpoint=True)


def telescoping(st, n):
    d = telescoping_steps(st, n)
    return (d[1:] - d[:-1]).astype(NP[st])


def uniform(st, n, *seed):
    return (np.random.default_rng([2, np.dtype(NP[st]).itemsize, n] + list(seed)).random(n) - 0.5).astype(NP[st])


def rounding(st, n):
    """Differences of neighbouring uniform numbers, (u[i + 1] - u[i]) / 3 rounded to the type (a third, so that a
    double element has a full mantissa too): the elements lie in (-1/3, 1/3) and so does every sum over a range, up
    to rounding. Nearly every addition rounds, and no running sum
    grows until it swallows what is added to it (sums of independent uniform elements do, in half within some ten
    thousand of them): the order of the additions shows in the low bits at every position of an array of any length.
    The first tile's numbers come from a generator of their own, the first of the seeds 0, 1, 2, ... at which the
    tile's four wave sums give other bits as (w0 + w1) + (w2 + w3) than left to right: a regrouped tile total then
    shows at out[4096] at the latest, also where the array has two tiles only."""
    sdt = NP[st]
    u = np.random.default_rng([3, np.dtype(sdt).itemsize, n]).random(n + 1)
    for seed in range(256 if n > TILE else 0):
        u[:TILE] = np.random.default_rng([4, np.dtype(sdt).itemsize, n, seed]).random(TILE)
        w = wave_scan(thread_sums(in_tiles(((u[1:TILE + 1] - u[:TILE]) / 3).astype(sdt))))[0, :, WAVE - 1]
        if ((w[0] + w[1]) + w[2]) + w[3] != (w[0] + w[1]) + (w[2] + w[3]):
            break
    return ((u[1:] - u[:-1]) / 3).astype(sdt)


def same_bits(got, want):
    """Equal bit for bit; a NaN equals any NaN at the same position (IEEE 754 leaves the sign and payload of a NaN
    that an operation makes to the implementation, and x86 sets the sign of the one it makes for inf - inf)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    if got.dtype.kind != "f":
        return np.array_equal(got, want)
    u = "u%d" % got.dtype.itemsize
    gn, wn = np.isnan(got), np.isnan(want)
    return np.array_equal(gn, wn) and np.array_equal(got.view(u)[~gn], want.view(u)[~wn])
