"""The constructed inputs of tests/test_gpu_segscan_lanes.py, numpy only, so that tests/test_segscan_lane_reach_cpu.py can
say through tests/segscan_lane_model.py which branch of the kernels each of them reaches. A case is written as the merge
itself: a list of ("r", k) for k rows and ("c", k) for k closes, in the order of the steps; the counts follow from it (a
close that follows a close ends an empty segment; rows behind the last close belong to no segment: the total is below n).
Every case names the rows the values' extremes are planted at: just before its runs of closes and before the tile and wave
edges it is aimed at."""
import numpy as np

from segscan_lane_model import ITEMS, WAVE
from segscan_model import FORMS, NP, OPS, PAIRS

PERIODS = (16, 17, 18)


def size(t):
    return np.dtype(NP[t]).itemsize


def rotate(number, k, value_size):
    """Run k of 6 of case `number`: the three ops x a 32-bit and a 64-bit sum type, and a kind, a form, a count type and
    a type pair of those widths in turn. value_size: None, or what the case fixes (8: the sum type is a 64-bit one)."""
    op = OPS[k % 3]
    wide = bool(k // 3) or value_size == 8
    turn = number + k
    vs = value_size or (4 if not wide else (4, 8)[turn % 2])
    pairs = [p for p in PAIRS if size(p[0]) == vs and size(p[1]) == (8 if wide else 4)]
    return op, bool(turn // 2 % 2), FORMS[(turn + k // 3) % 2], ("uint", "ulong")[turn // 3 % 2], pairs[(turn // 2 if wide and not value_size else turn) % len(pairs)]


class Case:
    def __init__(self, name, runs, value_size=None, align=0, extra_plants=()):
        self.name, self.value_size, self.align = name, value_size, align
        kinds = np.concatenate([np.full(k, kind == "c") for kind, k in runs if k > 0])      # True: the step closes a segment
        rows_before = np.cumsum(~kinds) - ~kinds                                            # rows among the steps before each step
        at = rows_before[kinds]                                                             # the end of every segment
        self.counts = np.diff(np.concatenate(([0], at))).astype(np.int64)
        self.n = int((~kinds).sum())
        self.m = int(kinds.sum())
        self.kinds = kinds
        # the row before every run of closes, and the ones the case adds
        first = np.flatnonzero(kinds & ~np.concatenate(([False], kinds[:-1])))
        plants = {int(rows_before[s]) - 1 for s in first if rows_before[s] > 0}
        plants |= {int(r) for r in extra_plants if 0 <= r < self.n}
        self.plants = sorted(plants)

    def row_before_step(self, step):
        """The last row among the steps before `step` (-1: none)."""
        return int((~self.kinds[:step]).sum()) - 1

    def values(self, vt, op, base):
        """base with, at every planted row, the extreme the op is after (the other one for a sum) and the other extreme one
        row before it: a carry that wrongly passes a close, or wrongly stops, changes every later row of the segment."""
        v = base[:self.n].copy()
        info = np.iinfo(NP[vt])
        hit, other = (info.min, info.max) if op == "min" else (info.max, info.min)
        for r in self.plants:
            v[r] = hit
            if r > 0 and r - 1 not in self.plants:
                v[r - 1] = other
        return v


def lane_cases(T):
    """SWEEP: lanes, waves and tiles."""
    W = WAVE * ITEMS
    assert T == 4 * W
    out = []
    # tile 0 is rows only and leaves its segment open; in tile 1 the segment closes on the last step of wave 0, wave 1 is
    # closes only, wave 2 rows only, wave 3 closes in the middle and on the tile's last step
    runs = [("r", T), ("r", W - 1), ("c", 1), ("c", W), ("r", W), ("r", 500), ("c", 1), ("r", W - 502), ("c", 1)]
    c = Case("a wave of closes, a wave of rows", runs)
    c.plants = sorted(set(c.plants) | {c.row_before_step(T), c.row_before_step(T + 3 * W)})
    out.append(c)
    # the same with the waves of closes and of rows in the tile's first and last wave
    runs = [("r", T - 5), ("c", 1), ("r", 4), ("c", W), ("r", 2 * W - 3), ("c", 3), ("r", W)]
    out.append(Case("the first wave closes, the last is rows", runs + [("r", 40), ("c", 1)]))
    # an open segment, then T closes that fill tile 1 exactly, then rows: tile 2 starts from the identity
    runs = [("r", T), ("c", T), ("r", 100), ("c", 1), ("r", 30), ("c", 1)]
    c = Case("a tile of closes behind an open segment", runs)
    c.plants = sorted(set(c.plants) | {T - 2})
    out.append(c)
    # one tile and 5 * 17 + 3 steps: lane 5 of tile 1 has 3 steps, the lanes behind it none
    runs = [("r", T - 20), ("c", 2), ("r", 18), ("r", 5 * ITEMS), ("r", 1), ("c", 1), ("r", 1)]
    out.append(Case("a last lane of 3 steps", runs + []))
    runs = [("r", 9), ("c", 1), ("r", 3)]                                                   # 13 steps: lane 0 has 13, no other lane any
    out.append(Case("one lane of 13 steps", runs))
    # total below n: tile 0 stores 100 of its rows, tile 1 none of its T, tile 2 none
    runs = [("r", 60), ("c", 1), ("r", 40), ("c", 3), ("r", T - 104), ("r", T), ("r", 55)]
    out.append(Case("rows beyond the total", runs))
    # closes on a lane's steps 0 and 16 with rows between them, in every lane of a wave; then every other step
    runs = []
    for _ in range(WAVE):
        runs += [("c", 1), ("r", ITEMS - 2), ("c", 1)]
    for _ in range(W // 2):
        runs += [("r", 1), ("c", 1)]
    runs += [("r", 2 * W + 7), ("c", 1)]
    out.append(Case("closes on a lane's first and last step", runs))
    return out


def period_cases(T):
    """Segments of 16, 17 and 18 rows in turn: 17 + 18 + 19 = 54 steps a round, 3 modulo 17, so that the closes drift
    through all 17 steps of the lanes."""
    rounds = (T + 300) // 54
    runs = []
    for _ in range(rounds):
        for length in PERIODS:
            runs += [("r", length), ("c", 1)]
    return [Case("lengths 16, 17 and 18 in turn", runs)]


def tails_cases(T):
    """TAILS. Tile 0 is `empties` closes, rows, one close and `count` rows that stay open into tile 1, where 50 rows later
    their segment closes: what TAILS reduces behind tile 0's last close is what tile 1 starts from. The address of
    values + c modulo 16 is set by the array's (align) and by the place of the close (empties)."""
    out = []
    k = 0
    for vs in (4, 8):
        per = 16 // vs
        for residue in range(0, 16, vs):
            head = ((16 - residue) % 16) // vs
            shapes = [("behind the body", head + per * (5 + k % 3) + per - 1), ("nothing behind the body", head + per * (7 + k % 2))]
            if residue:
                shapes.append(("a head and no body", head + per - 1))
            if residue == vs:
                shapes.append(("more than 256 vectors", head + per * 300 + 1))
            if residue == 0:
                shapes += [("fewer than one vector", 1), ("more than 256 vectors", per * 258)]
            for what, count in shapes:
                align = vs * (k % per)
                k += 1
                # c = T - 1 - count - ... : (align + c * vs) % 16 == residue
                want_c = ((residue - align) % 16) // vs
                empties = (T - 1 - count - want_c) % per
                rows = T - 1 - count - empties
                assert rows > 0 and (align + rows * vs) % 16 == residue
                runs = [("c", empties), ("r", rows), ("c", 1), ("r", count), ("r", 50), ("c", 1), ("r", 9), ("c", 1)]
                # an extreme in the last row of the stretch, and nowhere else in it
                c = Case("tails: %d-byte values, residue %d, %s" % (vs, residue, what), runs, vs, align, extra_plants=(T - 1 - empties - 1,))
                out.append(c)
    # the last close is the tile's last step: nothing behind it; every close before the tile's first row: the whole tile
    runs = [("r", T - 1), ("c", 1), ("c", 6), ("r", T - 6), ("r", 20), ("c", 1)]
    out.append(Case("tails: a close on the last step, closes before the first row", runs, 4, 8, extra_plants=(T - 2, 2 * T - 8)))
    runs = [("r", T - 3), ("c", 3), ("c", 2), ("r", T - 2), ("r", 33), ("c", 1)]
    out.append(Case("tails: 8-byte values, a close on the last step, closes before the first row", runs, 8, 0, extra_plants=(T - 4, 2 * T - 6)))
    return out


def carry_cases(T):
    """CARRY: 1, 15, 16, 17, 31, 32 and 33 tiles of segments of 1451 rows (1452 steps: the 48th lies across the step
    16 T, from the 16th tile into the 17th), every seventh segment followed by an empty one; every tile closes something
    and leaves rows open."""
    out = []
    for tiles in (1, 15, 16, 17, 31, 32, 33):
        steps = (tiles - 1) * T + 1000
        runs, at, k = [], 0, 0
        while at + 1452 + 1 <= steps:
            runs += [("r", 1451), ("c", 2 if k % 7 == 6 else 1)]
            at += 1452 + (k % 7 == 6)
            k += 1
        if steps - at > 1:
            runs += [("r", steps - at - 1), ("c", 1)]
        c = Case("carry: %d tiles" % tiles, runs)
        edges = [c.row_before_step(t * T) for t in range(1, tiles)]                         # the last row of every tile
        c.plants = sorted(set(c.plants[::5]) | {r for r in edges if r >= 0})
        out.append(c)
    return out


def all_cases(T):
    return lane_cases(T) + period_cases(T) + tails_cases(T) + carry_cases(T)
