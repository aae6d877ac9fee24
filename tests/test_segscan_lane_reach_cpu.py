"""What the constructed inputs of tests/test_gpu_segscan_lanes.py (tests/segscan_lane_cases.py) reach below the level of
the tile, said on the CPU through tests/segscan_lane_model.py: every branch of SWEEP's lanes and waves, of the division of
TAILS' stretch and of CARRY's two load paths is reached by a case that is built to reach it, named in the assertion. The
lane model is checked against merge_steps on every case, its constants against the library's getter."""
import numpy as np
import pytest

import cl_ops_amd as clo
from segscan_lane_cases import Case, PERIODS, all_cases, carry_cases, lane_cases, period_cases, rotate, size, tails_cases
from segscan_lane_model import CARRY_ITEMS, ITEMS, WAVE, close_steps, lanes
from segscan_model import FORMS, OPS, PAIRS, merge_steps

T = clo.segscan_tile(4, 4)
W = WAVE * ITEMS
FULL = (1 << ITEMS) - 1


def model(case, form="counts"):
    src = case.counts if form == "counts" else np.concatenate(([0], np.cumsum(case.counts))) + 77
    return lanes(form, src, case.n, T, value_size=case.value_size or 4, align=case.align)


@pytest.fixture(scope="module")
def models():
    return {c.name: (c, model(c)) for c in all_cases(T)}


def test_the_constants_are_the_librarys():
    assert T == clo.segscan_tile(4, 8) == clo.segscan_tile(8, 8) and T % ITEMS == 0
    assert T // ITEMS == 256 == 4 * WAVE                                        # CLO_SEG_THREADS, four waves
    assert clo.segreduce_tile(4, 4) == T                                        # the carry layouts of the other files are in these steps
    assert CARRY_ITEMS == 16 and 256 * CARRY_ITEMS == 4096                      # a trip of the carry scan


def test_the_lane_model_agrees_with_the_merge(models):
    names = [c.name for c in all_cases(T)]
    assert len(set(names)) == len(names)
    for name, (c, L) in models.items():
        for form in ("counts", "offsets"):
            Lf = L if form == "counts" else model(c, form)
            close, m, total = merge_steps("counts", c.counts, c.n)
            assert m == c.m and np.array_equal(np.flatnonzero(c.kinds), close), name       # the case is the merge it was written as
            assert Lf.tiles == -(-(c.m + c.n) // T), name
            per_tile = np.bincount(close // T, minlength=Lf.tiles)
            assert np.array_equal(Lf.na, per_tile) and np.array_equal(Lf.ne.sum(axis=1), per_tile), name
            assert np.array_equal(Lf.wave_closes.sum(axis=1), per_tile), name
            assert int(Lf.nb.sum()) == c.n == int(Lf.nr.sum()), name
            assert int(Lf.cnt.sum()) == c.m + c.n == int(Lf.steps.sum()), name
            assert np.array_equal(close_steps(Lf), close), name                            # every lane's mask, bit by bit
            assert (Lf.b0 + Lf.nb <= c.n).all() and (Lf.a0 + Lf.na <= c.m).all(), name
            assert (Lf.c >= Lf.b0).all() and (Lf.c + Lf.count == Lf.b0 + Lf.nb).all(), name
            assert (Lf.head + Lf.nvec * Lf.per + (Lf.rest - Lf.head) == Lf.count).all() and (Lf.rest < 2 * Lf.per).all(), name
            assert int(Lf.nstore.sum()) == min(total, c.n), name
        assert c.n <= 33 * T and all(0 <= r < c.n for r in c.plants), name


def test_a_case_written_as_steps():
    c = Case("x", [("c", 2), ("r", 3), ("c", 1), ("r", 2), ("c", 2), ("r", 1)])
    assert c.counts.tolist() == [0, 0, 3, 2, 0] and c.n == 6 and c.m == 5 and c.plants == [2, 4]
    assert c.row_before_step(0) == -1 and c.row_before_step(3) == 0 and c.row_before_step(11) == 5


def test_sweep_lanes_and_waves(models):
    c, L = models["a wave of closes, a wave of rows"]
    name = c.name
    assert L.tiles == 2 and L.na[0] == 0 and L.nb[0] == T, name + ": a tile with na == 0"
    assert (L.ne[1][WAVE:2 * WAVE] == ITEMS).all() and (L.nr[1][WAVE:2 * WAVE] == 0).all(), name + ": lanes with ne == 17"
    assert (L.closes[1][WAVE:2 * WAVE] == FULL).all(), name
    assert L.wave_closes[1].tolist() == [1, W, 0, 2], name + ": a wave of closes, a wave without one between waves with closes"
    assert L.nr[1][:WAVE].sum() == W - 1 and L.nr[1][2 * WAVE:].sum() > W, name + ": rows before and after the wave of closes"
    assert ((L.ne[1] == 0) & (L.steps[1] == ITEMS)).any(), name + ": a lane with ne == 0 and 17 steps"
    assert L.closes[1][WAVE - 1] == 1 << (ITEMS - 1), name + ": a close on bit 16"
    assert L.closes[1][WAVE] & 1, name + ": a close on bit 0"
    assert not c.kinds[T - 1] and not c.kinds[T], name + ": the segment is open across the tile edge"
    assert c.kinds[-1] and L.count[1] == 0 and L.na[1] > 0, name + ": TAILS with count == 0"
    assert L.count[0] == L.nb[0] == T and L.na[0] == 0, name + ": TAILS with count == nb, na == 0"

    c, L = models["the first wave closes, the last is rows"]
    assert L.wave_closes[1].tolist() == [W, 0, 3, 0] and L.wave_closes[0][3] == 1, c.name
    assert L.tiles == 3 and L.nb[2] == 40, c.name

    c, L = models["a tile of closes behind an open segment"]
    name = c.name
    assert L.tiles == 3 and L.nb[1] == 0 and L.cnt[1] == T and L.nb[0] > 0 and L.nb[2] > 0, name + ": a tile with nb == 0 between tiles with rows"
    assert not c.kinds[T - 1] and c.kinds[T], name + ": a segment is open before it"
    assert L.na[1] == T and L.count[1] == 0, name + ": its state is (closed, identity): tile 2 starts from the identity"
    assert (L.wave_closes[1] == W).all(), name

    c, L = models["a last lane of 3 steps"]
    name = c.name
    assert L.cnt[1] == 5 * ITEMS + 3 and L.steps[1][5] == 3, name + ": a lane with 0 < steps < 17"
    assert (L.steps[1][6:] == 0).all() and L.cnt[1] > 0, name + ": lanes with steps == 0"
    assert L.ne[1][5] == 1 and L.closes[1][5] == 2, name
    assert 0 < L.nstore[1] < L.nb[1], name + ": 0 < nstore < nb"
    c, L = models["one lane of 13 steps"]
    assert L.tiles == 1 and L.steps[0][0] == 13 and (L.steps[0][1:] == 0).all() and L.closes[0][0] == 1 << 9, c.name

    c, L = models["rows beyond the total"]
    name = c.name
    assert L.tiles == 3 and 0 < L.nstore[0] == 100 < L.nb[0], name + ": 0 < nstore < nb"
    assert L.nstore[1] == 0 and L.nb[1] == T and L.nstore[2] == 0 < L.nb[2], name + ": nstore == 0, nb > 0"

    c, L = models["closes on a lane's first and last step"]
    name = c.name
    assert (L.closes[0][:WAVE] == (1 | 1 << (ITEMS - 1))).all(), name + ": bits 0 and 16"
    assert (L.closes[0][WAVE:2 * WAVE] & 0x1ffff).tolist() == [0x0aaaa if i % 2 == 0 else 0x15555 for i in range(WAVE)], name
    assert L.wave_closes[0].tolist() == [2 * WAVE, W // 2, 0, 0], name


def test_the_closes_drift_through_every_step_of_a_lane(models):
    (c,) = period_cases(T)
    assert sum(p + 1 for p in PERIODS) % ITEMS == 3 and c.counts[:6].tolist() == list(PERIODS) * 2
    L = models[c.name][1]
    bits = (L.closes[0][:, None] >> np.arange(ITEMS)) & 1
    assert (bits.sum(axis=0) > 0).all(), c.name + ": all 17 positions within one tile"
    assert L.ne[0].min() == 0 and L.ne[0].max() == 1, c.name                              # closes 17, 18 and 19 steps apart: a lane has one or none


def test_tails(models):
    seen = {4: {}, 8: {}}
    for c in tails_cases(T):
        L = models[c.name][1]
        vs = c.value_size
        assert L.tiles >= 2 and L.count[0] > 0 or "last step" in c.name, c.name
        if "last step" in c.name:
            continue
        assert L.c[0] + L.count[0] == L.b0[0] + L.nb[0] and L.na[1] > 0 and L.nr[1][0] == ITEMS, c.name   # tile 1 starts inside the stretch
        d = seen[vs].setdefault(int(L.residue[0]), set())
        d.add("rest > 0" if L.rest[0] > 0 else "rest == 0")
        if L.rest[0] == L.head[0]:
            d.add("rest == head")
        if L.head[0] > 0 and L.nvec[0] == 0:
            d.add("head, no body")
        if L.nvec[0] > 256:
            d.add("nvec > 256")
        if 0 < L.count[0] < L.per:
            d.add("count < PER")
        if c.align:
            d.add("moved by the array")
        if (L.c[0] * vs) % 16:
            d.add("moved by the close")
        assert c.row_before_step(T) in c.plants, c.name                                     # an extreme in the stretch's last row
    for vs, residues in ((4, (0, 4, 8, 12)), (8, (0, 8))):
        assert sorted(seen[vs]) == list(residues), "every residue of values + c modulo 16, %d-byte values" % vs
        for r in residues:
            assert {"rest > 0", "rest == head"} <= seen[vs][r], (vs, r, seen[vs][r])
            assert r == 0 or "head, no body" in seen[vs][r], (vs, r)
        every = set().union(*seen[vs].values())
        assert {"nvec > 256", "count < PER", "moved by the array", "moved by the close"} <= every, (vs, every)
    for vs in (4, 8):
        c, L = models["tails: %sa close on the last step, closes before the first row" % ("8-byte values, " if vs == 8 else "")]
        assert L.count[0] == 0 and L.na[0] > 0 and c.kinds[T - 1], c.name + ": count == 0 with na > 0"
        assert L.count[1] == L.nb[1] > 0 and L.na[1] > 0 and L.c[1] == L.b0[1], c.name + ": count == nb with na > 0"
        assert L.residue[1] != 0 and L.head[1] > 0, c.name
    c, L = models["a wave of closes, a wave of rows"]
    assert L.count[0] == L.nb[0] and L.na[0] == 0, c.name + ": count == nb with na == 0"


def test_carry(models):
    reached = set()
    for c in carry_cases(T):
        L = models[c.name][1]
        reached.add(int(L.tiles))
        assert (L.na > 0).all() and (L.count[:-1] > 0).all(), c.name + ": every tile closes something and all but the last leave rows open"
        assert L.vector.tolist() == [(i + 1) * CARRY_ITEMS <= L.tiles for i in range(L.vector.size)], c.name
        assert L.last_thread == (L.tiles - 1) // CARRY_ITEMS, c.name
        if L.tiles > CARRY_ITEMS:
            assert not c.kinds[CARRY_ITEMS * T - 1] and not c.kinds[CARRY_ITEMS * T], c.name + ": a segment from tile 15 into tile 16"
    assert reached == {1, 15, 16, 17, 31, 32, 33}
    on = {int(models[c.name][1].tiles): bool(models[c.name][1].vector[-1]) for c in carry_cases(T)}
    assert on == {1: False, 15: False, 16: True, 17: False, 31: False, 32: True, 33: False}   # the thread that holds the last tile
    L = models["carry: 17 tiles"][1]
    assert L.vector.tolist() == [True, False], "a thread on the vector path next to one on the scalar path"
    L = models["carry: 31 tiles"][1]
    assert L.vector.tolist() == [True, False] and L.tiles - CARRY_ITEMS == 15, "15 states on the scalar path behind 16 on the vector path"


def test_every_case_is_small():
    cases = all_cases(T)
    for c in lane_cases(T) + period_cases(T) + tails_cases(T):
        assert c.n + c.m <= 3 * T, c.name
    assert max(c.n + c.m for c in cases) <= 33 * T


def test_the_rotation_meets_everything():
    """The six runs of every case: each op with a 32-bit and with a 64-bit sum type (8-byte values: 64-bit ones); over the
    cases every kind, form, count type and type pair."""
    seen = set()
    for number in range(len(all_cases(T))):
        runs = [rotate(number, k, None) for k in range(6)]
        assert {(r[0], size(r[4][1])) for r in runs} == {(op, w) for op in OPS for w in (4, 8)}
        seen |= {(r[1], r[2], r[3]) for r in runs} | {r[4] for r in runs}
        assert {(r[0], size(r[4][0]), size(r[4][1])) for r in (rotate(number, k, 8) for k in range(6))} == {(op, 8, 8) for op in OPS}
        assert {(r[0], size(r[4][0]), size(r[4][1])) for r in (rotate(number, k, 4) for k in range(6))} == {(op, 4, w) for op in OPS for w in (4, 8)}
        assert sum(size(r[4][0]) == size(r[4][1]) for r in runs) >= 2               # ... and at least two of them run again in place
    assert seen == {(i, f, c) for i in (False, True) for f in FORMS for c in ("uint", "ulong")} | set(PAIRS)
