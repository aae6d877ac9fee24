"""The strata of the CloSegScan fuzz (tests/test_gpu_segscan_fuzz.py), computed from the numpy model alone so that
tests/test_segscan_cpu.py can say on the CPU what they reach. 216 strata: every dimension's values dealt out evenly and
shuffled by one seed (form x count type x type pair x op x kind x length distribution x clip x num_in), each with
n <= 4 T rows, T the tile (merge steps) passed in. strata_lanes() is a second family of 96 with lengths at the scale of a
lane and a wave of the tile sweep, n <= 3 T rows, and an in_place dimension; strata() and SEED are not touched by it."""
import numpy as np

from segscan_model import FORMS, NP, OPS, PAIRS

SEED = 20231
STRATA = 216
DISTS = ("ones", "geometric", "half_empty", "long", "edge", "single")
CLIPS = ("exact", "above", "below")          # total == n, total > n (segments clipped), total < n (tail rows untouched)
NUM_INS = ("absent", "below", "above")


def _deal(rng, values):
    reps = -(-STRATA // len(values))
    idx = np.tile(np.arange(len(values)), reps)[:STRATA]
    rng.shuffle(idx)
    return [values[i] for i in idx]


def _counts(rng, dist, T):
    if dist == "ones":
        return np.ones(int(rng.integers(1, 3 * T)), np.int64)
    if dist == "geometric":
        return rng.geometric(1 / 16.0, int(rng.integers(1, T // 5))).astype(np.int64) - (rng.random(1)[0] < 0.5)
    if dist == "half_empty":
        c = rng.geometric(1 / 16.0, int(rng.integers(2, T // 5))).astype(np.int64)
        c[rng.random(c.size) < 0.5] = 0
        return c
    if dist == "long":
        return rng.integers(1, 3 * T // 2, int(rng.integers(1, 4))).astype(np.int64)
    if dist == "single":
        return np.array([int(rng.integers(1, 4 * T - 8))], np.int64)
    # "edge": segment 0 closes on the last step of tile 0, the empty segment 1 on the first step of tile 1, segment 2
    # runs through tile 2, in which nothing closes; short segments and empties follow
    rest = rng.geometric(1 / 8.0, int(rng.integers(1, 40))).astype(np.int64)
    rest[rng.random(rest.size) < 0.3] = 0
    return np.concatenate((np.array([T - 1, 0, 2 * T + 3], np.int64), rest))


LANE_SEED = 20232
LANE_STRATA = 96
LANE_DISTS = ("empty_runs", "near_period", "wave_blocks", "lone_rows")
LANE_ITEMS, LANE_WAVE = 17, 64              # the kernel's merge steps per lane and lanes per wave (tests/segscan_lane_model.py)


def _deal_n(rng, values, n):
    idx = np.tile(np.arange(len(values)), -(-n // len(values)))[:n]
    rng.shuffle(idx)
    return [values[i] for i in idx]


def _lane_counts(rng, dist, T):
    """Lengths at the scale of a lane (17 merge steps) and a wave (64 lanes), at most 3 T rows and 3 T segments."""
    block = LANE_ITEMS * LANE_WAVE
    if dist == "near_period":                                                  # a close every 16 to 20 steps
        return rng.integers(15, 20, int(rng.integers(20, 3 * T // 19))).astype(np.int64)
    out, rows, segs = [], 0, 0
    limit = int(rng.integers(T // 2, 5 * T // 2))                              # merge steps, before the last piece
    while rows + segs < limit:
        if dist == "empty_runs":                                               # 1 to 40 empty segments between short ones
            piece = np.concatenate((rng.integers(1, 9, int(rng.integers(1, 6))), np.zeros(int(rng.integers(1, 41)), np.int64)))
        elif dist == "wave_blocks":                                            # short segments up to a random step, then one or two waves' worth of empties
            piece = np.concatenate((rng.integers(1, 30, int(rng.integers(1, 60))), np.zeros(block * int(rng.integers(1, 3)), np.int64)))
        else:                                                                  # "lone_rows": one row between long runs of empties
            piece = np.concatenate((np.zeros(int(rng.integers(100, 1500)), np.int64), [1]))
        out.append(piece.astype(np.int64))
        rows, segs = rows + int(piece.sum()), segs + piece.size
    out.append(rng.integers(1, 20, int(rng.integers(1, 9))).astype(np.int64))  # rows behind the last run of empties
    return np.concatenate(out)


def strata_lanes(T):
    """A second family beside strata(), which it leaves as it is: 96 strata with n <= 3 T rows whose lengths are at the
    scale of the lanes (runs of 1 to 40 empty segments between short segments; lengths uniform in 15 .. 19; blocks of one
    or two times 64 x 17 empty segments at a random step (two: a whole wave of closes wherever they start); a single row
    between long runs of empties), and one more dimension, in_place: dealt among the strata whose value and sum widths
    match, false in the others. The dicts are those of strata() with in_place added."""
    rng = np.random.default_rng(LANE_SEED)
    N = LANE_STRATA
    dims = dict(form=_deal_n(rng, FORMS, N), count_type=_deal_n(rng, ("uint", "ulong"), N), pair=_deal_n(rng, PAIRS, N), op=_deal_n(rng, OPS, N),
                inclusive=_deal_n(rng, (False, True), N), dist=_deal_n(rng, LANE_DISTS, N), clip=_deal_n(rng, CLIPS, N), num_mode=_deal_n(rng, NUM_INS, N))
    same = [s for s in range(N) if np.dtype(NP[dims["pair"][s][0]]).itemsize == np.dtype(NP[dims["pair"][s][1]]).itemsize]
    in_place = dict(zip(same, _deal_n(rng, (True, False), len(same))))
    out = []
    for s in range(N):
        d = {k: v[s] for k, v in dims.items()}
        counts = _lane_counts(rng, d["dist"], T)
        while counts.sum() > 3 * T - 8 or counts.size > 3 * T:
            counts = counts[:-1]
        m_h = counts.size
        num_in = None if d["num_mode"] == "absent" else m_h + 5 if d["num_mode"] == "above" else max(m_h - max(m_h // 4, 1), 0)
        total = int(counts[:num_in].sum()) if num_in is not None else int(counts.sum())
        n = total if d["clip"] == "exact" else max(total - int(rng.integers(1, 40)), 0) if d["clip"] == "above" else total + int(rng.integers(1, 8))
        cdt = np.uint32 if d["count_type"] == "uint" else np.uint64
        base = int(rng.integers(0, 1000)) * int(rng.integers(0, 2))
        src = counts.astype(cdt) if d["form"] == "counts" else (np.concatenate(([0], np.cumsum(counts))) + base).astype(cdt)
        vt, st = d["pair"]
        info = np.iinfo(NP[vt])
        pool = np.array([info.min, info.max, info.min + 1, info.max - 1, 0, 1, 5, 77], dtype=NP[vt])
        values = np.where(rng.random(n) < 0.5, rng.choice(pool, n), rng.integers(0, 100, n).astype(NP[vt])).astype(NP[vt])
        d.update(value_type=vt, sum_type=st, src=src, num_in=num_in, values=values, n=n, m_h=m_h, in_place=in_place.get(s, False))
        del d["pair"]
        out.append(d)
    return out


def strata(T):
    """A list of dicts: form, count_type, value_type, sum_type, op, inclusive, dist, clip, num_mode, src (counts or
    offsets in the count type), num_in (None or an int), values (in the value type), n."""
    rng = np.random.default_rng(SEED)
    dims = dict(form=_deal(rng, FORMS), count_type=_deal(rng, ("uint", "ulong")), pair=_deal(rng, PAIRS), op=_deal(rng, OPS),
                inclusive=_deal(rng, (False, True)), dist=_deal(rng, DISTS), clip=_deal(rng, CLIPS), num_mode=_deal(rng, NUM_INS))
    out = []
    for s in range(STRATA):
        d = {k: v[s] for k, v in dims.items()}
        counts = np.maximum(_counts(rng, d["dist"], T), 0)
        while counts.sum() > 4 * T - 8:                                        # n <= 4 T whatever the clip adds
            counts = counts[:-1]
        m_h = counts.size
        num_in = None if d["num_mode"] == "absent" else m_h + 5 if d["num_mode"] == "above" else max(m_h - max(m_h // 4, 1), 0)
        total = int(counts[:num_in].sum()) if num_in is not None else int(counts.sum())
        n = total if d["clip"] == "exact" else max(total - int(rng.integers(1, 40)), 0) if d["clip"] == "above" else total + int(rng.integers(1, 8))
        cdt = np.uint32 if d["count_type"] == "uint" else np.uint64
        base = int(rng.integers(0, 1000)) * int(rng.integers(0, 2))
        src = counts.astype(cdt) if d["form"] == "counts" else (np.concatenate(([0], np.cumsum(counts))) + base).astype(cdt)
        vt, st = d["pair"]
        info = np.iinfo(NP[vt])
        # extremes among small numbers: sums wrap, the signed and the unsigned orders differ
        pool = np.array([info.min, info.max, info.min + 1, info.max - 1, 0, 1, 5, 77], dtype=NP[vt])
        values = np.where(rng.random(n) < 0.5, rng.choice(pool, n), rng.integers(0, 100, n).astype(NP[vt])).astype(NP[vt])
        d.update(value_type=vt, sum_type=st, src=src, num_in=num_in, values=values, n=n, m_h=m_h)
        del d["pair"]
        out.append(d)
    return out
