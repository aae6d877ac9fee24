"""The order in which cl_ops_amd/csrc/hip/clo_hip_segfsum.hip adds, restated in numpy: what CloSegFSum
(include/clo_segfsum.h) computes for any of its four pairs of types, bit for bit. Every addition is done in the sum type
(numpy adds two arrays of one type in that type). The contract, with T = 4352 steps per tile, 256 lanes of 17 steps, waves
of 64 lanes, and the carry scan's trips of 4096 tiles (256 threads x 16 states):

  conversion   every row is converted to the sum type by a C cast, numpy's `astype` (exact for the four pairs);
  steps        the m clipped ends c_r = min(e_r, n) are merged with the rows 0 .. n - 1, an end first when c_r <= j: row j
               is taken at step j + #{r < m : c_r <= j}, segment r closes at step c_r + r; steps past m + n take nothing;
  first walk   a lane adds the rows of its 17 steps left to right from +0, starting over from +0 after a close: the
               lane's state is (it closed, the sum since its last close); a step without a row adds +0;
  network      the 64 lane states of a wave: every lane takes the state 1, 2, 4, 8 lanes below it inside its row of 16
               lanes, then rows 1 and 3 take lane 15 of the row below, then rows 2 and 3 take lane 31; taking l into r is
               (l.h | r.h, r.h ? r.a : l.a + r.a), and a lane without a source takes (0, +0);
  waves        the four wave totals (lane 63) are combined left to right from (0, +0): what lies before every wave,
               and the tile's state;
  second walk  a lane starts from (before its wave) combined with (the network's result one lane down, (0, +0) for lane
               0), adds its rows one by one, and at a close the running sum is the segment's and the lane starts over
               from +0;
  carry        the tiles' states in trips of 4096: a thread combines its 16 states left to right from (0, +0); network;
               the waves left to right from the RUNNING state of the trips before; a thread walks its 16 tiles from
               (before its wave) combined with (one lane down); tile t's carry is the open sum of the tiles before it;
  fix-up       the first segment that closes in a tile gets sum = sum + carry.

For an integer sum type every order gives the same wrapped sums, so the model then equals segreduce_model.segreduce
(tests/test_segfsum_cpu.py asserts it): that pins which row reaches which segment independently of floating point. The
functions in STAGES are the steps, so that a test can replace one of them by a deliberately different one and show that
its inputs tell the two apart."""
import numpy as np

from expand_model import FORMS, ends_of  # noqa: F401
from fscan_model import same_bits  # noqa: F401

THREADS, ITEMS, WAVE = 256, 17, 64
WAVES = THREADS // WAVE
TILE = THREADS * ITEMS                     # 4352
CARRY_ITEMS = 16
CARRY_TRIP = THREADS * CARRY_ITEMS         # 4096 tiles per trip
NETWORK = ("shr1", "shr2", "shr4", "shr8", "bcast15", "bcast31")

NP = {"half": np.float16, "float": np.float32, "double": np.float64}
PAIRS = (("half", "float"), ("float", "float"), ("float", "double"), ("double", "double"))   # value -> sum


def convert(a, sdt):
    """(sum type) row, as the kernel's C cast."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.ascontiguousarray(a).astype(sdt)


def combine(lh, la, rh, ra):
    """The state l taken into the state r from the left."""
    return lh | rh, np.where(rh, ra, la + ra)


# ---- the stages ----

def step_positions(c, n):
    """(row_step[n], close_step[m]) for the clipped ends c (ascending, int64)."""
    j = np.arange(n, dtype=np.int64)
    return j + np.searchsorted(c, j, "right"), c + np.arange(c.size, dtype=np.int64)


def lane_walk(close, x):
    """The first walk. close, x: (ITEMS, tiles, THREADS). -> (h, a) of every lane."""
    h = np.zeros(close.shape[1:], bool)
    a = np.zeros(x.shape[1:], x.dtype)
    for k in range(ITEMS):
        h = h | close[k]
        a = np.where(close[k], a.dtype.type(0), a + x[k])
    return h, a


def network(h, a, steps=NETWORK):
    """The inclusive segmented scan of every wave: h, a of shape (.., WAVE) -> the same shape."""
    shape = h.shape
    h = h.reshape(-1, 4, 16).copy()
    a = a.reshape(-1, 4, 16).copy()
    for s in steps:
        lh = np.zeros_like(h)
        la = np.zeros_like(a)
        if s.startswith("shr"):
            off = int(s[3:])
            lh[:, :, off:] = h[:, :, :-off]
            la[:, :, off:] = a[:, :, :-off]
        elif s == "bcast15":
            for row in (1, 3):
                lh[:, row, :] = h[:, row - 1, 15:16]
                la[:, row, :] = a[:, row - 1, 15:16]
        else:
            for row in (2, 3):
                lh[:, row, :] = h[:, 1, 15:16]
                la[:, row, :] = a[:, 1, 15:16]
        h, a = combine(lh, la, h, a)
    return h.reshape(shape), a.reshape(shape)


def waves(th, ta, run_h=None, run_a=None):
    """th, ta: the wave totals (g, WAVES). -> (before_h, before_a) of shape (g, WAVES) and (all_h, all_a) of shape (g,),
    combined left to right from the running state ((0, +0) where none is given)."""
    bh = np.zeros(th.shape[0], bool) if run_h is None else run_h
    ba = np.zeros(ta.shape[0], ta.dtype) if run_a is None else run_a
    before_h, before_a = np.empty_like(th), np.empty_like(ta)
    for w in range(WAVES):
        before_h[:, w], before_a[:, w] = bh, ba
        bh, ba = combine(bh, ba, th[:, w], ta[:, w])
    return before_h, before_a, bh, ba


def one_lane_down(h, a):
    """(.., WAVE) -> the state of the lane below, (0, +0) for lane 0."""
    eh, ea = np.zeros_like(h), np.zeros_like(a)
    eh[..., 1:], ea[..., 1:] = h[..., :-1], a[..., :-1]
    return eh, ea


def second_walk(close, x, in_a):
    """close, x: (ITEMS, tiles, THREADS); in_a: (tiles, THREADS). -> at[k] = the running sum before step k: the
    segment's sum where step k closes."""
    at = np.empty_like(x)
    run = in_a
    for k in range(ITEMS):
        at[k] = run
        run = np.where(close[k], run.dtype.type(0), run + x[k])
    return at


def carry_thread(sh, sa):
    """A thread's CARRY_ITEMS states (g, CARRY_ITEMS) left to right from (0, +0)."""
    h = np.zeros(sh.shape[0], bool)
    a = np.zeros(sa.shape[0], sa.dtype)
    for j in range(CARRY_ITEMS):
        h, a = combine(h, a, sh[:, j], sa[:, j])
    return h, a


def carry_waves(th, ta, run_h, run_a):
    """The four wave totals of a trip after the running state of the trips before."""
    return waves(th, ta, run_h, run_a)


def carry(tile_h, tile_a, stages=None):
    """The exclusive segmented scan of the tiles' states: the open sum of the tiles before every tile."""
    S = dict(STAGES, **(stages or {}))
    tiles = tile_h.size
    out = np.empty_like(tile_a)
    run_h, run_a = np.zeros(1, bool), np.zeros(1, tile_a.dtype)
    for base in range(0, tiles, CARRY_TRIP):
        cnt = min(CARRY_TRIP, tiles - base)
        sh = np.zeros(CARRY_TRIP, bool)
        sa = np.zeros(CARRY_TRIP, tile_a.dtype)
        sh[:cnt], sa[:cnt] = tile_h[base:base + cnt], tile_a[base:base + cnt]
        sh, sa = sh.reshape(THREADS, CARRY_ITEMS), sa.reshape(THREADS, CARRY_ITEMS)
        mh, ma = S["carry_thread"](sh, sa)
        ih, ia = S["network"](mh.reshape(1, WAVES, WAVE), ma.reshape(1, WAVES, WAVE))
        bh, ba, all_h, all_a = S["carry_waves"](ih[:, :, WAVE - 1], ia[:, :, WAVE - 1], run_h, run_a)
        eh, ea = one_lane_down(ih, ia)
        h, a = combine(bh[:, :, None], ba[:, :, None], eh, ea)
        h, a = h.reshape(THREADS), a.reshape(THREADS)
        res = np.empty((THREADS, CARRY_ITEMS), tile_a.dtype)
        for j in range(CARRY_ITEMS):
            res[:, j] = a
            h, a = combine(h, a, sh[:, j], sa[:, j])
        out[base:base + cnt] = res.reshape(-1)[:cnt]
        run_h, run_a = all_h, all_a
    return out


def fixup(sums, first, carries):
    """sums[first[t]] = sums[first[t]] + carries[t] for the tiles in which a segment closes (first[t] >= 0)."""
    has = first >= 0
    sums[first[has]] = sums[first[has]] + carries[has]
    return sums


STAGES = {"step_positions": step_positions, "lane_walk": lane_walk, "network": network, "waves": waves,
          "second_walk": second_walk, "carry_thread": carry_thread, "carry_waves": carry_waves, "fixup": fixup}


def segfsum_converted(c, v, stages=None):
    """The m sums of rows v (already in the sum type) for the clipped ends c (int64, ascending)."""
    S = dict(STAGES, **(stages or {}))
    m, n = c.size, v.size
    if m == 0:
        return np.zeros(0, v.dtype)
    with np.errstate(over="ignore", invalid="ignore"):        # (integer sums wrap, inf - inf is a NaN: both are results)
        tiles = -(-(m + n) // TILE)
        row_step, close_step = S["step_positions"](c, n)
        x = np.zeros(tiles * TILE, v.dtype)
        x[row_step] = v
        close = np.zeros(tiles * TILE, bool)
        close[close_step] = True
        x = np.ascontiguousarray(x.reshape(tiles, THREADS, ITEMS).transpose(2, 0, 1))
        close = np.ascontiguousarray(close.reshape(tiles, THREADS, ITEMS).transpose(2, 0, 1))
        lh, la = S["lane_walk"](close, x)
        ih, ia = S["network"](lh.reshape(tiles, WAVES, WAVE), la.reshape(tiles, WAVES, WAVE))
        bh, ba, all_h, all_a = S["waves"](ih[:, :, WAVE - 1], ia[:, :, WAVE - 1])
        eh, ea = one_lane_down(ih, ia)
        _, in_a = combine(bh[:, :, None], ba[:, :, None], eh, ea)
        at = S["second_walk"](close, x, in_a.reshape(tiles, THREADS))
        sums = at.transpose(1, 2, 0).reshape(-1)[close_step].copy()
        carries = carry(all_h, all_a, stages)
        # the first segment that closes in every tile: segment r closes in tile close_step[r] // T
        first = np.full(tiles, -1, np.int64)
        t_of = close_step // TILE
        r = np.arange(m - 1, -1, -1, dtype=np.int64)
        first[t_of[::-1]] = r                                  # (the smallest r of a tile is stored last)
        return S["fixup"](sums, first, carries)


def clipped_ends(form, counts_or_offsets, n, num_in=None):
    ends, m = ends_of(form, counts_or_offsets, num_in)
    return np.minimum(ends, np.uint64(n)).astype(np.int64), (int(ends[-1]) if m else 0)


def segfsum(form, counts_or_offsets, values, sum_type, num_in=None, stages=None):
    """(sums, total): the m sums in the sum type (a name of NP, or a numpy type) with the bits the library gives, and
    the unclamped total."""
    sdt = np.dtype(NP.get(sum_type, sum_type))
    v = convert(values, sdt)
    c, total = clipped_ends(form, counts_or_offsets, v.size, num_in)
    return segfsum_converted(c, v, stages), total


def depth(tiles):
    """D: an upper bound on the number of additions any row passes through on its way into a sum."""
    in_tile = ITEMS + len(NETWORK) + (WAVES - 1) + 1 + (ITEMS - 1)          # first walk, network, waves before, lanes below, second walk
    if tiles <= 1:
        return in_tile
    open_sum = ITEMS + len(NETWORK) + WAVES                                  # into the tile's open sum
    trips = -(-tiles // CARRY_TRIP)
    last = (WAVES - 1) + 1 + (CARRY_ITEMS - 1)                               # waves before, lanes below, the thread's walk
    if trips == 1:
        in_carry = CARRY_ITEMS + len(NETWORK) + last
    else:
        in_carry = CARRY_ITEMS + len(NETWORK) + WAVES + WAVES * (trips - 2) + last
    return max(in_tile, open_sum + in_carry + 1)                             # and the fix-up


# ---------------------------------------------------------------------------------------------------------------------
# the inputs and shapes of tests/test_gpu_segfsum.py; tests/test_segfsum_cpu.py shows what they can tell apart
# ---------------------------------------------------------------------------------------------------------------------

ROWS = (0, 1, 16, 17, 18, 1087, 1088, 1089, TILE - 1, TILE, TILE + 1, 2 * TILE + 5)
LAYOUTS = ("one", "ones", "17", "geometric", "second_empty", "gaps", "three_tiles", "tile_edges", "totals_above", "num_in_below")
TELESCOPE_BOUND = {"float": 1 << 23, "double": 1 << 52}
ROUNDING_SEED = 0     # the first seed at which every deliberately different stage of tests/test_segfsum_cpu.py shows


def layout(name, n, seed=0):
    """(counts (uint64), num_in or None) of layout `name` over n rows."""
    rng = np.random.default_rng([11, LAYOUTS.index(name), n, seed])

    def geometric(total):
        out = []
        while sum(out) < total:
            out.append(int(rng.geometric(1.0 / 16)))
        return out

    num_in = None
    if name == "one":
        c = [n]
    elif name == "ones":
        c = [1] * n
    elif name == "17":
        c = [17] * (n // 17) + ([n % 17] if n % 17 else [])
    elif name == "geometric":
        c = geometric(n)
        if c:
            c[-1] -= sum(c) - n
    elif name == "second_empty":
        g = geometric(n)
        if g:
            g[-1] -= sum(g) - n
        c = [x for pair in zip(g, [0] * len(g)) for x in pair]
    elif name == "gaps":
        c = [n // 2] + [0] * (4 * TILE + 5) + [n - n // 2]
    elif name == "three_tiles":
        c = [min(3, n), max(n - 6, 0), max(min(3, n - 3), 0)] if n >= 6 else [0, n, 0]
    elif name == "tile_edges":
        # closes on the last and on the first step of every tile: segment r closes at step c_r + r
        c, rows, r, t = [], 0, 0, 1
        while True:
            want = t * TILE - 1 - r                            # c_r for a close at step t T - 1
            if want > n:
                break
            c += [want - rows, 0]                              # ... and the next at step t T
            rows, r, t = want, r + 2, t + 1
        c.append(n - rows)
    elif name == "totals_above":
        c = geometric(n + 40) + [5, 0, 7]
    else:
        c = geometric(n) + [3, 0, 2]
        num_in = len(c) * 2 // 3
    return np.array(c, np.uint64), num_in


def source(form, counts, count_type=np.uint32, base=0):
    """counts -> the counts or the offsets (from `base`) in the count type."""
    if form == "counts":
        return counts.astype(count_type)
    return (np.concatenate((np.zeros(1, np.uint64), np.cumsum(counts, dtype=np.uint64))) + np.uint64(base)).astype(count_type)


def telescoping_steps(st, n):
    """Integers d[0 .. n] in [0, B]: the rows are d[i + 1] - d[i]. Every partial sum of the tree is a sum over a
    contiguous range, d[r] - d[l], an integer of magnitude <= B that the sum type holds exactly: a segment's sum is
    d[end] - d[start] whatever the order, and a row lost or counted twice shows."""
    return np.random.default_rng([1, np.dtype(NP[st]).itemsize, n]).integers(0, TELESCOPE_BOUND[st], n + 1, endpoint=True)


def telescoping(vt, st, n):
    """Rows of value type vt whose partial sums in sum type st are exact (half values: differences below 2^11)."""
    if vt == "half":
        d = np.cumsum(np.random.default_rng([1, 2, n]).integers(-2047, 2048, n + 1))
        return (d[1:] - d[:-1]).astype(np.float16)
    bound = "float" if vt == "float" else st
    d = telescoping_steps(bound, n)
    return (d[1:] - d[:-1]).astype(NP[vt])


def rounding(vt, n, seed=ROUNDING_SEED):
    """Differences of neighbouring uniform numbers, (u[i + 1] - u[i]) / 3 rounded to the value type: the rows lie in
    (-1/3, 1/3) and so does every sum over a range, up to rounding. Nearly every addition rounds, and no running sum
    grows until it swallows what is added to it: the order of the additions shows in the low bits of every segment that
    is long enough to have an order."""
    u = np.random.default_rng([3, np.dtype(NP[vt]).itemsize, n, seed]).random(n + 1)
    return ((u[1:] - u[:-1]) / 3).astype(NP[vt])


def rows_for(vt, st, n, seed=ROUNDING_SEED):
    """Rounding rows for the pair vt -> st. Where the sum type is wider than the value type, rows of one magnitude add
    without rounding (halves below 1/3 are multiples of 2^-24, which a float sum below 1 holds exactly; floats likewise
    in a double), and no order would show. There the rows are spread over more binades than the sum type has bits: half
    rows over 2^-12 .. 2^14, float rows over 2^-39 .. 2^0, so that the large rows set the sums' exponent and the
    additions of the middle ones round."""
    if np.dtype(NP[vt]).itemsize == np.dtype(NP[st]).itemsize:
        return rounding(vt, n, seed)
    rng = np.random.default_rng([6, np.dtype(NP[vt]).itemsize, n, seed])
    u = rng.random(n + 1)
    k = rng.integers(-12, 15, n) if vt == "half" else -rng.integers(0, 40, n)
    return ((u[1:] - u[:-1]) / 3 * np.exp2(k)).astype(NP[vt])


# The rows of the GPU test of (2 * 4096 + 108) tiles, per sum type: rows_for("float", st, rows, seed), the first seed at
# which adding the running state of a trip last instead of first (test_segfsum_cpu.py: _running_last) changes a bit of the
# sum of the segment that runs through the whole second trip. (The other layout of that test cannot show it: its long
# segments close in the first wave of a trip, where nothing lies between the running state and the lanes.) Found by
# running the model with and without that stage for seeds 0, 1, 2, ...: float 4 (0 to 3 give equal bits), double 2.
TRIP_SEEDS = {"float": 4, "double": 2}


def mixed(vt, n, seed=0):
    """Mixed signs and magnitudes over some twenty binades: cancellation inside the segments."""
    rng = np.random.default_rng([5, np.dtype(NP[vt]).itemsize, n, seed])
    span = 6 if vt == "half" else 20
    with np.errstate(over="ignore"):
        return ((rng.random(n) - 0.5) * np.exp2(rng.integers(-span, span, n))).astype(NP[vt])
