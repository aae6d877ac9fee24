"""The strata of the CloSegScan fuzz (tests/test_gpu_segscan_fuzz.py), computed from the numpy model alone so that
tests/test_segscan_cpu.py can say on the CPU what they reach. 216 strata: every dimension's values dealt out evenly and
shuffled by one seed (form x count type x type pair x op x kind x length distribution x clip x num_in), each with
n <= 4 T rows, T the tile (merge steps) passed in."""
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
