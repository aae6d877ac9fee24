"""What the stratified fuzz of tests/test_gpu_fuzz.py reaches, checked without a GPU: over the committed seeds every
stratum of every family's table (every kernel instantiation) is drawn, the random parts cover what they promise (sizes
0, 1, tile +- 1 and non-multiples of the tile, a run longer than two tiles, objects reused for a larger and a smaller
call, views off their alignment, the wrap trap), and the vectorised models agree with plain Python loops on the
generator's own odd inputs (NaN payloads, unsorted keys, wrapping sums)."""
import numpy as np
import pytest

import test_gpu_fuzz as F
from rbk_model import rbk
from sbk_model import sbk, sbk_loop, identity

FAMILIES = ["rbk", "sbk", "hist", "merge"]
_ALL = {}


def cases_of(family):
    if family not in _ALL:
        _ALL[family] = [c for seed in range(F.SEEDS[family]) for c in F.draw_cases(family, seed)]
    return _ALL[family]


def test_the_tables_hold_every_instantiation():
    assert len(F.STRATA["rbk"]) == 4 * (1 + 2 + 4 * 3) == 60
    assert len(F.STRATA["sbk"]) == 4 * (2 + 4 * 3) * 2 == 112
    assert len(F.STRATA["hist"]) == 4 * 2 * 6 * 3 == 144
    assert len(F.STRATA["merge"]) == 11 * 5 == 55
    for f in FAMILIES:
        assert len(set(F.STRATA[f])) == len(F.STRATA[f])
        assert F.SEEDS[f] * F.CASES[f] >= 2 * len(F.STRATA[f])
        assert 60 <= F.CASES[f] <= 80


@pytest.mark.parametrize("family", FAMILIES)
def test_every_stratum_is_drawn(family):
    """The stratum is worked out from the arguments of the call (stratum_of), not from a label the generator left."""
    drawn = {}
    for c in cases_of(family):
        drawn.setdefault(F.stratum_of(c), []).append(c)
    missing = [s for s in F.STRATA[family] if s not in drawn]
    assert not missing, "%s: never drawn: %r" % (family, missing)
    assert set(drawn) == set(F.STRATA[family])
    new = {F.stratum_of(c) for c in cases_of(family) if not c["reuse"]}
    assert new == set(F.STRATA[family])                  # each with an object of its own at least once


@pytest.mark.parametrize("family", FAMILIES)
def test_draw_cases_is_a_pure_function(family):
    assert F.draw_cases(family, 0) == F.draw_cases(family, 0)
    assert F.draw_cases(family, 0) != F.draw_cases(family, 1)
    assert repr(F.draw_cases(family, 1)) == repr(cases_of(family)[F.CASES[family]:2 * F.CASES[family]])


@pytest.mark.parametrize("family", FAMILIES)
def test_sizes_offsets_and_reuse(family):
    cases = cases_of(family)
    sizes = [(n, c["tile"]) for c in cases for n in ((c["na"], c["nb"]) if family == "merge" else (c["n"],))]
    for special in (lambda n, t: n == 0, lambda n, t: n == 1, lambda n, t: n == t - 1, lambda n, t: n == t + 1, lambda n, t: n == t,
                    lambda n, t: n > 4 * t, lambda n, t: n > 1 << 18):
        assert any(special(n, t) for n, t in sizes)
    assert sum(1 for n, t in sizes if n % t) > len(sizes) // 2               # never only tile multiples
    assert all(n <= (1 << 20) + 6 for n, t in sizes)
    offs = {o for c in cases for o in c["offs"]}
    assert all(0 <= o <= 31 for o in offs) and len(offs) > 16 and any(o % 2 for o in offs) and max(offs) >= 28
    # an object reused: about half of the cases, its constructor arguments unchanged, sizes up and down
    total = lambda c: c["na"] + c["nb"] if family == "merge" else c["n"]
    reused = [(a, b) for a, b in zip(cases, cases[1:]) if b["reuse"]]
    assert len(cases) // 3 <= len(reused) <= 2 * len(cases) // 3
    assert all(a["object"] == b["object"] and a["seed"] == b["seed"] for a, b in reused)
    assert any(total(b) > 4 * total(a) > 0 for a, b in reused) and any(total(a) > 4 * total(b) > 0 for a, b in reused)
    # a small call after a large one on the same object (the tile states of the large one are still in its scratch), and back
    assert sum(1 for a, b in reused if total(a) > 8 * a["tile"] and total(b) < 2 * a["tile"]) >= 2
    assert sum(1 for a, b in reused if total(b) > 8 * a["tile"] and total(a) < 2 * a["tile"]) >= 2


def rbk_loop(keys, values, op, sum_dtype):
    """The definition of reduce by key, element by element in Python integers."""
    dt = np.dtype(sum_dtype)
    bits = 8 * dt.itemsize
    mask = (1 << bits) - 1
    wrap = lambda x: (x & mask) - (1 << bits) if dt.kind == "i" and (x & mask) >> (bits - 1) else x & mask
    bk = keys.view("u%d" % keys.itemsize)
    heads, aggr = [], []
    for i in range(keys.size):
        x = wrap(1 if values is None else int(values[i]))                        # the C cast (sum type) value
        if i == 0 or bk[i] != bk[i - 1]:
            heads.append(i)
            aggr.append(x)
        else:
            aggr[-1] = wrap(aggr[-1] + x) if op == "sum" else min(aggr[-1], x) if op == "min" else max(aggr[-1], x)
    return keys[heads], np.array([a & mask for a in aggr], dtype="u%d" % dt.itemsize).view(dt), len(heads)


@pytest.mark.parametrize("family", ["rbk", "sbk"])
def test_by_key_inputs_and_the_models_against_loops(family):
    cases = cases_of(family)
    small = [c for c in cases if c["n"] <= 5000]
    assert len(small) >= len(cases) // 6
    seen = set()
    for c in cases:
        keys, values = F.by_key_inputs(c)
        assert keys.size == c["n"] and keys.dtype == np.dtype(F.TR._NP[c["kt"]]) and (values is None) == (c["vt"] is None)
        if c["n"] > 2 * c["tile"] + 1:
            assert F.longest_run(keys) > 2 * c["tile"], c
            seen.add("long")
        if keys.dtype.kind == "f" and keys.size:
            b = keys.view("u%d" % keys.itemsize)
            seen.update(("nan",) if np.isnan(keys).any() and len(set(b[np.isnan(keys)].tolist())) > 1 else ())
            seen.update(("zeros",) if len(set(b[keys == 0].tolist())) > 1 else ())
        seen.add(c["structure"]["kind"])
        if c["n"] > 5000:
            continue
        sdt = np.dtype(F.TR._NP[c["st"]])
        if family == "rbk":
            wk, wa, m = rbk(keys, values, c["op"], sdt)
            lk, la, lm = rbk_loop(keys, values, c["op"], sdt)
            assert m == lm and np.array_equal(wk.view(np.uint8), lk.view(np.uint8)) and wa.dtype == la.dtype and np.array_equal(wa, la), c
        else:
            got, want = sbk(keys, values, c["op"], sdt, c["inclusive"]), sbk_loop(keys, values, c["op"], sdt, c["inclusive"])
            assert got.dtype == want.dtype and np.array_equal(got, want), c
            if not c["inclusive"] and c["n"]:
                assert got[0] == identity(c["op"], sdt)
    assert seen >= {"long", "nan", "zeros", "mixture", "unsorted"}, seen
    # the sums do wrap somewhere: a 32-bit sum of full-range values over a long run
    assert any(c["vt"] == "uint" and c["st"] == "uint" and c["op"] == "sum" and c["n"] > c["tile"] for c in cases)


def test_histogram_cases():
    cases = cases_of("hist")
    seen = set()
    for c in cases:
        info = np.iinfo(F.TH._NP[c["kt"]])
        assert info.min <= c["lower"] <= info.max and 0 <= c["shift"] < info.bits and c["num_bins"] >= 1
        if c["lower"] + (c["num_bins"] << c["shift"]) > info.max + 1:
            seen.add("wrap trap")
        seen.add(c["layout"])
        seen.add("accumulate" if c["accumulate"] else "overwrite")
        seen.add("shift %s" % ("0" if c["shift"] == 0 else "B-1" if c["shift"] == info.bits - 1 else "between"))
        if c["n"] <= 5000:
            keys, values, prior = F.hist_inputs(c)
            assert keys.size == c["n"] and keys.dtype == np.dtype(F.TH._NP[c["kt"]]) and prior.size == c["num_bins"]
            assert prior.dtype == np.dtype(F.TH._NP[c["st"]]) and (values is None) == (c["vt"] is None)
            want = F.TH.histogram(keys, values, prior.dtype, c["lower"], c["shift"], c["num_bins"])
            if want.any():
                seen.add("counted")
            if c["vt"] is None:
                assert int(want.sum()) <= c["n"]
    assert seen >= {"wrap trap", "uniform", "skewed", "sorted", "handful", "accumulate", "overwrite", "shift 0", "shift B-1", "shift between", "counted"}, seen


def test_merge_cases():
    from merge_model import order_key
    cases = cases_of("merge")
    assert {c["ranges"] for c in cases} == {"overlapping", "a_below_b", "b_below_a", "interleaved"}
    assert any(c["na"] == 0 for c in cases) and any(c["nb"] == 0 for c in cases) and all(c["na"] + c["nb"] for c in cases)
    for c in cases:
        if c["na"] + c["nb"] > 20000:
            continue
        a, b = F.merge_inputs(c)
        assert a.size == c["na"] and b.size == c["nb"] and a.dtype == b.dtype == np.dtype(F.TM._NP[c["kt"]])
        for x in (a, b):                                  # both inputs are in the merge's order
            k = order_key(x)
            assert bool(np.all(k[:-1] <= k[1:])), c
        if c["ranges"] == "a_below_b" and a.size and b.size:
            assert order_key(a)[-1] <= order_key(b)[0]
        if c["ranges"] == "b_below_a" and a.size and b.size:
            assert order_key(b)[-1] <= order_key(a)[0]
