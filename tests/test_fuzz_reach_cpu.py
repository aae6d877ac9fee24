"""What the stratified fuzz of tests/test_gpu_fuzz.py reaches, checked without a GPU: over the committed seeds every
stratum of every family's table (every kernel instantiation) is drawn, the random parts cover what they promise (sizes
0, 1, tile +- 1 and non-multiples of the tile, a run longer than two tiles, objects reused for a larger and a smaller
call, views off their alignment, the wrap trap), and the vectorised models agree with plain Python loops on the
generator's own odd inputs (NaN payloads, unsorted keys, wrapping sums). For search, the set operations and select:
every haystack, needle, range, run and threshold kind is seen, every (key type, pred), (op, pred) and (op, form) of
select is drawn, the inputs are in the library's order wherever the case promises it, and search_model, setop_model
and select_model equal element-by-element loops written from the headers' definitions. For top-k: every key and cut
kind, every (key type, which) and (form, order, which), a call whose keys can be loaded as vectors and whose values
cannot (and the reverse), a cut inside a tie run that takes a whole tile of equal keys, tie runs across a tile edge with
the cut before and behind the edge, no "sorted" case above the cap and none refused, and topk_model against a plain loop
over (order key, index) pairs. For expand, the segmented reduction and the segmented sort: every structure kind, every
placement of num_in, of the capacity or the rows and of the offsets' base, a long segment across a tile edge, tiles on both
sides of expand's switch, wrapped sums and extremes carried in from another tile, every key kind x key size of the
segmented sort and what the move masks of its cases cover, and the three models against plain loops."""
import numpy as np
import pytest

import test_gpu_fuzz as F
from merge_model import order_key
from rbk_model import rbk
from sbk_model import sbk, sbk_loop, identity
from expand_model import expand
from search_model import search
from segreduce_model import segreduce
from segsort_model import segsort
from select_model import select
from setop_model import setop
from topk_model import topk

FAMILIES = ["rbk", "sbk", "hist", "merge", "search", "setop", "select", "topk", "expand", "segreduce", "segsort"]
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
    assert len(F.STRATA["search"]) == 11 * 2 * 2 == 44
    assert len(F.STRATA["setop"]) == 11 * 5 * 4 == 220
    assert len(F.STRATA["select"]) == 11 * 5 * 2 + 11 == 121
    assert len(F.STRATA["topk"]) == 11 * (5 * 2 + 1) == 121
    assert len(F.STRATA["expand"]) == 2 * 2 * 5 == 20
    assert len(F.STRATA["segreduce"]) == 2 * 2 * 12 * 3 == 144
    assert len(F.STRATA["segsort"]) == 11 * 5 * 2 * 2 == 220
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
    two = {"merge": ("na", "nb"), "setop": ("na", "nb"), "search": ("nh", "nn")}.get(family, ("n",))
    sizes = [(c[k], c["L"] if k == "nh" else c["tile"]) for c in cases for k in two]       # (the haystack's unit is L)
    for special in (lambda n, t: n == 0, lambda n, t: n == 1, lambda n, t: n == t - 1, lambda n, t: n == t + 1, lambda n, t: n == t,
                    lambda n, t: n > 4 * t, lambda n, t: n > 1 << 18):
        assert any(special(n, t) for n, t in sizes)
    assert sum(1 for n, t in sizes if n % t) > len(sizes) // 2               # never only tile multiples
    assert all(n <= (1 << 20) + 6 for n, t in sizes)
    offs = {o for c in cases for o in c["offs"]}
    if family == "segreduce":                                                # (no array of it has elements below 4 bytes: every multiple of 4)
        assert offs == set(range(0, 32, 4))
    else:
        assert all(0 <= o <= 31 for o in offs) and len(offs) > 16 and any(o % 2 for o in offs) and max(offs) >= 28
    # an object reused: about half of the cases, its constructor arguments unchanged, sizes up and down
    total = lambda c: sum(c[k] for k in two)
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


def in_order(x):
    k = order_key(x)
    return bool(np.all(k[:-1] <= k[1:]))


def search_loop(hay, ndl, upper):
    """clo_search.h: the number of haystack keys < the needle (upper: <= it), counted one by one."""
    oh, on = [int(x) for x in order_key(hay)], [int(x) for x in order_key(ndl)]
    return [sum(1 for h in oh if (h <= x if upper else h < x)) for x in on]


def test_search_cases():
    cases = cases_of("search")
    seen, looped = set(), 0
    for c in cases:
        P, L = c["P"], c["L"]
        seen.add(("nh", [e(P, L) for e in F._HAY_EDGES].index(c["nh"])) if c["nh"] in [e(P, L) for e in F._HAY_EDGES] else "nh off the edges")
        if c["nh"] + c["nn"] > 40000:
            continue
        hay, ndl = F.search_inputs(c)
        dt = np.dtype(F.TSE._NP[c["kt"]])
        assert hay.size == c["nh"] and ndl.size == c["nn"] and hay.dtype == ndl.dtype == dt
        assert in_order(hay) and (in_order(ndl) or not c["sorted"]), c
        seen.update((("hay", c["hay"]), ("needles", c["needles"])))
        oh, on = order_key(hay), order_key(ndl)
        bits = lambda x: set(x.view("u%d" % dt.itemsize).tolist())
        if c["hay"] == "equal" and c["nh"]:
            assert len(bits(hay)) == 1
        if c["hay"] == "tie_run":                                     # longer than L, and a pivot of the general path inside it
            at, ln = c["tie"]
            assert ln > L and len(bits(hay[at:at + ln])) == 1 and any(at <= k * c["nh"] // P < at + ln for k in range(1, P)), c
        if c["needles"] == "hits" and c["nn"]:
            assert bits(ndl) <= bits(hay)
        if c["needles"] == "neighbours" and c["nn"]:
            near = {(x + d) % (1 << (8 * dt.itemsize)) for x in oh.tolist() for d in (-1, 1)}
            assert set(on.tolist()) <= near
            if dt.kind == "f" and np.isnan(ndl).any() and not bits(ndl[np.isnan(ndl)]) <= bits(hay):
                seen.add("a NaN payload next to a key")
            zero = lambda x, neg: bool(((x == 0) & (np.signbit(x) == neg)).any())
            if dt.kind == "f" and ((zero(ndl, True) and zero(hay, False)) or (zero(ndl, False) and zero(hay, True))):
                seen.add("the other zero")                             # -0 and +0 are neighbours in the library's order
        if c["needles"] == "below" and c["nn"] and on.max() < oh[0]:
            seen.add("all below")
        if c["needles"] == "above" and c["nn"] and on.min() > oh[-1]:
            seen.add("all above")
        if c["needles"] == "one_key" and c["nn"] > 50:
            assert np.bincount(np.unique(on, return_inverse=True)[1]).max() > 0.8 * c["nn"]
        if not c["nn"]:
            seen.add("no needles")
        if c["nh"] * c["nn"] <= 400000:
            looped += 1
            assert search(hay, ndl, c["upper"]).tolist() == search_loop(hay, ndl, c["upper"]), c
    assert looped >= len(cases) // 6
    want = {("hay", k) for k in F.HAY_KINDS} | {("needles", k) for k in F.NEEDLE_KINDS} | {("nh", i) for i in range(len(F._HAY_EDGES))}
    assert seen >= want | {"nh off the edges", "a NaN payload next to a key", "the other zero", "all below", "all above", "no needles"}, want - seen
    # a key type other than uint with the edges P and L, on both paths
    for edge in (2, 3, 4, 5, 6, 7):
        assert any(c["kt"] != "uint" and c["nh"] == F._HAY_EDGES[edge](c["P"], c["L"]) for c in cases), edge


def setop_loop(op, a, b):
    """clo_setop.h: x occurs m times in A and n times in B, A's element is the r-th of its run and B's the s-th; the
    table says which are kept; the output is in merge order, equal keys of A before those of B."""
    oa, ob = [int(x) for x in order_key(a)], [int(x) for x in order_key(b)]
    rows = []
    for src, mine, other in ((0, oa, ob), (1, ob, oa)):
        copies, met = {}, {}
        for y in other:
            copies[y] = copies.get(y, 0) + 1
        for i, x in enumerate(mine):
            rank = met.get(x, 0)                                                # r, or s: the equal keys before this one
            met[x] = rank + 1
            there = copies.get(x, 0)                                            # n, or m
            keep = {"union": src == 0 or rank >= there, "intersection": src == 0 and rank < there, "difference": src == 0 and rank >= there,
                    "symmetric_difference": rank >= there}[op]
            if keep:
                rows.append((x, src, i))
    rows.sort()
    return [len(oa) * src + i for x, src, i in rows]


def test_setop_cases():
    cases = cases_of("setop")
    assert {c["ranges"] for c in cases} == set(F.SETOP_RANGES) and {c["runs"] for c in cases} == set(F.SETOP_RUNS)
    assert {c["long"][0] for c in cases if c["long"]} == {"a", "b", "both"} and any(c["long"] is None for c in cases)
    assert any(c["na"] == 0 for c in cases) and any(c["nb"] == 0 for c in cases) and all(c["na"] + c["nb"] for c in cases)
    for op in F.TSO.OPS:                                   # values_b given and left out, whether the op looks at it or not
        assert {c["pass_vb"] for c in cases if c["op"] == op} == {False, True}
    looped, seen = 0, set()
    for c in cases:
        if c["na"] + c["nb"] > 30000:
            continue
        a, b = F.setop_inputs(c)
        assert a.size == c["na"] and b.size == c["nb"] and a.dtype == b.dtype == np.dtype(F.TM._NP[c["kt"]])
        assert in_order(a) and in_order(b), c
        oa, ob = order_key(a), order_key(b)
        if c["ranges"] == "a_eq_b":
            assert np.array_equal(oa, ob)
        if c["ranges"] == "a_subset_b":                   # as multisets
            ua, ca = np.unique(oa, return_counts=True)
            ub, cb = np.unique(ob, return_counts=True)
            assert set(ua.tolist()) <= set(ub.tolist()) and all(ca <= cb[np.searchsorted(ub, ua)])
        if not c["long"] and a.size and b.size:
            if c["ranges"] == "a_below_b":
                assert oa[-1] <= ob[0]
            if c["ranges"] == "b_below_a":
                assert ob[-1] <= oa[0]
        if c["long"]:
            where, la, lb = c["long"]
            longest = lambda o: int(np.unique(o, return_counts=True)[1].max()) if o.size else 0
            if c["ranges"] in F.SETOP_RANGES[:4]:
                assert longest(oa) >= la and longest(ob) >= lb and (la > 2 * c["tile"] or where == "b") and (lb > 2 * c["tile"] or where == "a"), c
                if where == "both":
                    x = np.unique(oa, return_counts=True)
                    x = x[0][x[1].argmax()]
                    if int((oa == x).sum()) != int((ob == x).sum()) > 2 * c["tile"]:
                        seen.add("one key longer than two tiles in both, of different lengths")
            else:
                assert longest(ob) > 2 * c["tile"]
            seen.add("long " + where)
        if c["runs"] == "distinct" and a.dtype.itemsize >= 4 and a.size > 100 and not c["long"] and c["ranges"] == "overlapping":
            assert np.unique(oa).size > 0.8 * a.size
            seen.add("mostly distinct")
        if c["runs"] == "short" and a.size > 100 and np.unique(oa).size < 0.8 * a.size:
            seen.add("short runs")
        if c["na"] + c["nb"] <= 5000:
            looped += 1
            wk, p = setop(c["op"], a, b)
            assert p.tolist() == setop_loop(c["op"], a, b), c
            assert np.array_equal(wk.view(np.uint8), np.concatenate((a, b))[p].view(np.uint8))
            seen.add(c["op"])
    assert looped >= len(cases) // 8
    assert seen >= {"long a", "long b", "long both", "one key longer than two tiles in both, of different lengths", "mostly distinct", "short runs"} | set(F.TSO.OPS), seen


def select_loop(op, pred, keys, fot):
    """clo_select.h: kept iff the flag is not 0, or iff the key <pred> the threshold in the library's order."""
    if pred == "flagged":
        kept = [int(f) != 0 for f in np.asarray(fot).view(np.uint8)]
    else:
        t = int(order_key(np.array([fot], dtype=keys.dtype))[0])
        kept = [{"lt": x < t, "le": x <= t, "gt": x > t, "ge": x >= t, "eq": x == t, "ne": x != t}[pred] for x in (int(x) for x in order_key(keys))]
    rows = [i for i, k in enumerate(kept) if k]
    return rows + ([i for i, k in enumerate(kept) if not k] if op == "partition" else []), len(rows)


def test_select_cases():
    cases = cases_of("select")
    kts, preds, ops = F.TM.KEY_TYPES, F.TSL.PREDS, F.TSL.OPS
    assert {(c["kt"], c["pred"]) for c in cases} == {(kt, pred) for kt in kts for pred in preds}                       # the 77
    assert {(c["op"], c["pred"]) for c in cases} == {(op, pred) for op in ops for pred in preds}                       # the 14
    assert {(c["op"], c["mode"]) for c in cases} == {(op, m) for op in ops for m in F.TSL.MODES + ("arg_no_keys",)}
    assert all(c["pred"] == "flagged" for c in cases if c["mode"] == "arg_no_keys")
    assert {c["pattern"] for c in cases} == set(F.TSL.PATTERNS) and {c["keys"] for c in cases} == set(F.SELECT_KEYS)
    assert {c["threshold"] for c in cases if c["pred"] != "flagged"} == set(F.THRESHOLDS)
    # a CloSelect really reused: the (op, pred) of the case before on the same object, at a size of its own
    again = [(a, b) for a, b in zip(cases, cases[1:]) if b["reuse"] and (a["op"], a["pred"]) == (b["op"], b["pred"])]
    assert len(again) >= 20 and any(b["n"] > 4 * a["n"] > 0 for a, b in again) and any(a["n"] > 4 * b["n"] > 0 for a, b in again)
    flags, looped, seen = set(), 0, set()
    for c in cases:
        if c["n"] > 40000:
            continue
        keys, fot = F.select_inputs(c)
        dt = np.dtype(F.TM._NP[c["kt"]])
        assert keys.size == c["n"] and keys.dtype == dt
        mask = F.TSL.mask_of(c["pattern"], c["n"], c["tile"], c["data_seed"])
        p, k = select(c["op"], c["pred"], keys, fot)
        if c["pred"] == "flagged":
            assert fot.dtype == np.uint8 and fot.size == c["n"] and k == int(mask.sum())
            flags.update(fot.tolist())
        else:
            u = "u%d" % dt.itemsize
            thr = np.array([fot], dtype=dt).reshape(1)              # what run_select hands to the device: the same bits
            assert fot.dtype == dt and thr.view(u)[0] == np.array(fot).reshape(1).view(u)[0]
            t, ok = int(order_key(thr)[0]), order_key(keys)
            top = (1 << (8 * dt.itemsize)) - 1
            occurs = bool((ok == t).any())
            if c["threshold"] == "present" and c["n"] > 200 and 50 < k < c["n"] - 50:
                assert occurs, c
            if c["threshold"] == "between" and c["n"] > 1:
                assert not occurs
                if ok.min() < t < ok.max():
                    seen.add("between two keys that occur")
            if c["threshold"] == "least":
                assert t == 0
                if dt.kind == "f":
                    assert np.isnan(thr[0]) and np.signbit(thr[0]) and thr.view(u)[0] == top                        # -NaN, the largest payload
                seen.add("least, " + ("among the keys" if occurs else "below every key"))
            if c["threshold"] == "greatest":
                assert t == top
                seen.add("greatest, " + ("among the keys" if occurs else "above every key"))
            if k == int(mask.sum()) and 0 < k < c["n"]:
                seen.add("the pattern kept by a comparison")
        if c["n"] <= 5000:
            looped += 1
            lp, lk = select_loop(c["op"], c["pred"], keys, fot)
            assert k == lk and p.tolist() == lp, c
    assert flags == set(range(256))                        # flags take every byte value
    assert looped >= len(cases) // 6
    assert seen >= {"between two keys that occur", "least, among the keys", "least, below every key", "greatest, among the keys", "greatest, above every key",
                    "the pattern kept by a comparison"}, seen


def topk_loop(which, order, keys, k):
    """clo_topk.h: the first m = min(k, numel) of the stable sort by the key's order (unsigned by bits, signed by value,
    IEEE by sign, then magnitude bits: -0 below +0, NaNs at the ends by payload), the largest first for "largest", the
    lower index first among equal keys; in that order or by index. (rows, the index of the m-th chosen element)."""
    dt = keys.dtype
    if dt.kind == "f":
        bits = 8 * dt.itemsize
        mag = lambda raw: raw & ((1 << (bits - 1)) - 1)
        o = [-(mag(raw) + 1) if raw >> (bits - 1) else mag(raw) for raw in keys.view("u%d" % dt.itemsize).tolist()]
    else:
        o = [int(x) for x in keys.tolist()]
    pairs = sorted((-x if which == "largest" else x, i) for i, x in enumerate(o))[:min(k, len(o))]
    rows = [i for _, i in pairs]
    return (sorted(rows) if order == "input" else rows), (rows[-1] if rows else None)


def test_topk_cases():
    cases = cases_of("topk")
    kts, W = F.TM.KEY_TYPES, F.TT.WHICH
    assert len(cases) == 4 * 62 == 248
    assert {c["keys"] for c in cases} == set(F.TOPK_KEYS) and {c["cut"] for c in cases} == set(F.TOPK_CUTS)
    assert {(c["kt"], c["which"]) for c in cases} == {(kt, w) for kt in kts for w in W}                                # the 22
    forms = {(m, o, w) for m in F.TT.MODES for o in F.TT.ORDERS for w in W} | {("kth_only", None, w) for w in W}       # the 22
    assert {F.stratum_of(c)[1:] + (c["which"],) for c in cases} == forms
    assert all(c["kth"] for c in cases if c["mode"] == "kth_only") and all(c["order"] == "input" for c in cases if c["mode"] == "kth_only")
    for m in F.TT.MODES:                                   # kth_out given and NULL next to every form
        assert {c["kth"] for c in cases if c["mode"] == m} == {False, True}, m
    assert {c["digit"] for c in cases if c["keys"] == "one_digit"} >= set(range(8))                     # every digit of the widest key
    # a CloTopK really reused: the (which, order) of the case before on the same object, at a size of its own
    again = [(a, b) for a, b in zip(cases, cases[1:]) if b["reuse"] and (a["which"], a["order"]) == (b["which"], b["order"])]
    assert len(again) >= 20 and any(b["n"] > 4 * a["n"] > 0 for a, b in again) and any(a["n"] > 4 * b["n"] > 0 for a, b in again)
    # keys that vector loads take and values that they do not, and the reverse: kvec and vvec are decided apart
    for m in ("v4", "v8"):
        mixed = {(c["offs"][0] % 16 == 0, c["offs"][1] % 16 == 0) for c in cases if c["mode"] == m and c["n"] > c["tile"]}
        assert mixed >= {(True, False), (False, True)}, (m, mixed)
    # kth_out at an odd offset of a multi-byte key next to outputs on a 16-byte boundary
    assert any(c["kth"] and c["offs"][4] % 16 and c["offs"][2] % 16 == 0 and c["offs"][3] % 16 == 0 and c["mode"] in ("v4", "v8", "arg") for c in cases)
    seen, looped, calls, at_cap = set(), 0, 0, 0
    for c in cases:
        keys, k = F.topk_inputs(c)
        n, tile, which, order = c["n"], c["tile"], c["which"], c["order"]
        dt = np.dtype(F.TM._NP[c["kt"]])
        assert keys.size == n and keys.dtype == dt and keys.flags.c_contiguous and k >= 0
        assert F.topk_inputs(c)[1] == k                                    # the GPU runner resolves the same cut
        m = min(k, n)
        if order == "sorted":                                              # never refused ...
            assert m <= c["cap"], c
            at_cap += m == c["cap"]
        calls += m > 0
        assert m > 0 or n == 0 or k == 0, c                                # ... and every other case is a device call
        if dt.kind == "f" and n:
            b = keys.view("u%d" % dt.itemsize)
            seen.update(("nan payloads",) if len(set(b[np.isnan(keys)].tolist())) > 2 else ())
            seen.update(("both zeros",) if len(set(b[keys == 0].tolist())) > 1 else ())
        x = order_key(keys)
        x = ~x if which == "largest" else x
        if c["keys"] == "reversed" and n > 100 and which == "smallest" and bool(np.all(x[:-1] >= x[1:])):
            seen.add("the winners at the end")
        if c["keys"] == "one_digit" and n > 1000:
            assert np.unique(x).size <= 256 and np.unique(x >> x.dtype.type(8 * c["digit"])).size <= 256 and np.unique(x).size > 100
        if c["keys"] == "few":
            assert np.unique(x).size <= 5
        if m:
            t = np.sort(x)[m - 1]
            eq = np.flatnonzero(x == t)                                    # the tie run of the k-th key, by index
            take = m - int((x < t).sum())                                  # how many of it are taken
            assert 1 <= take <= eq.size
            kinds = {"run_first": take == 1, "run_last": take == eq.size, "next_run_first": take == 1 or k > n, "run_inside": 1 < take < eq.size or eq.size < 3}
            if c["cut"] in kinds and not (order == "sorted" and m == c["cap"]):
                assert kinds[c["cut"]], c
            if 1 < take < eq.size:
                seen.add("a cut strictly inside a run")
                if c["mode"] != "kth_only" and order == "input" and eq.size > 2 * tile and take >= tile and eq[0] // tile == 0:
                    seen.add("a whole tile of equal keys is taken")       # room >= the tile in the run's first tile
            if c["mode"] != "kth_only" and take < eq.size and eq[0] // tile != eq[-1] // tile:
                last = eq[take - 1]                                        # the last equal element taken
                if last // tile == eq[0] // tile:
                    seen.add("the cut before the tile edge")
                else:
                    seen.add("the cut behind the tile edge")
                if eq[take] // tile != last // tile:
                    seen.add("the cut on the tile edge")
            if c["mode"] != "kth_only" and n > 2 * tile and take == eq.size and eq[0] // tile != eq[-1] // tile:
                seen.add("all of a run across tiles")
        if n <= 5000:
            looped += 1
            for o in ((order,) if c["mode"] != "kth_only" else F.TT.ORDERS):
                p, kth = topk(which, o, keys, k)
                rows, last = topk_loop(which, o, keys, k)
                assert p.tolist() == rows, c
                assert kth.tobytes() == (keys[last:last + 1].tobytes() if rows else b""), c
    assert looped >= len(cases) // 6
    assert calls >= 200 and at_cap >= 2, (calls, at_cap)
    assert seen >= {"nan payloads", "both zeros", "the winners at the end", "a cut strictly inside a run", "a whole tile of equal keys is taken",
                    "the cut before the tile edge", "the cut behind the tile edge", "all of a run across tiles"}, seen


# ---- expand, the segmented reduction and the segmented sort ----

def _segmented_common(family, resolve):
    """What the three generators promise alike; resolve(c) -> (counts, rows or capacity, num_in, base). Returns the
    resolved cases."""
    cases = cases_of(family)
    assert {c["place"] for c in cases} == set(F.PLACES) and {c["num_in"] for c in cases} == set(F.NUM_INS) and {c["base"] for c in cases} == set(F.BASES)
    assert {(c["form"], c["ct"]) for c in cases} == {(f, t) for f in ("counts", "offsets") for t in ("uint", "ulong")}
    assert {c["segments"]["empty"] for c in cases} == set(F.SEG_EMPTY)
    seen, out = set(), []
    for c in cases:
        counts, rows, num_in, base = resolve(c)
        m, total = counts.size, int(counts.sum())
        assert counts.dtype == np.int64 and (counts >= 0).all() and total + (m if family == "segreduce" else 0) == c["n"], c
        assert m >= 1 or (family == "segreduce" and c["n"] == 0)
        taken = total if num_in is None else int(counts[:num_in].sum())
        assert {"at": rows == taken, "below": rows < taken or taken == 0, "above": rows > taken}[c["place"]], c
        assert {"absent": num_in is None, "below": num_in is not None and (num_in < m or m == 0), "at": num_in == m, "above": num_in is not None and num_in > m}[c["num_in"]], c
        if c["form"] == "offsets":
            src = F.TSS.source("offsets", c["ct"], counts, base)
            assert np.array_equal(np.diff(src.astype(np.uint64)), counts.astype(np.uint64)), c       # the base wraps nothing
            if c["base"] == "top":
                seen.add("a uint array that ends at 2^32 - 1" if c["ct"] == "uint" and int(src[-1]) == (1 << 32) - 1 else "a ulong base above 2^40")
        if m > total > 0:
            seen.add("more segments than rows")
        z = np.flatnonzero(np.diff(np.concatenate(([1], (counts == 0).astype(np.int8), [1]))))
        if z.size and (counts == 0).any() and int(np.diff(z).max()) > c["L"] and (counts == 0)[z[np.diff(z).argmax()]]:
            seen.add("a run of more than L empty segments")
        if c["segments"]["long"] and int(counts.max()) > 2 * c["tile"]:
            r = int(counts.argmax())
            s0 = int(counts[:r].sum()) + (r if family == "segreduce" else 0)                           # its first row, or merge step
            if s0 // c["tile"] != (s0 + int(counts[r]) - 1) // c["tile"] and s0 + int(counts[r]) <= rows + (r if family == "segreduce" else 0):
                seen.add("a segment longer than two tiles across a tile edge")
        if m > 20 and (counts == 0).mean() > 0.4:
            seen.add("half of the segments empty")
        if m == 1:
            seen.add("one segment")
        out.append((c, counts, rows, num_in, base))
    assert seen >= {"a uint array that ends at 2^32 - 1", "a ulong base above 2^40", "more segments than rows", "a run of more than L empty segments",
                    "a segment longer than two tiles across a tile edge", "half of the segments empty", "one segment"}, seen
    small = [x for x in out if x[0]["n"] <= 5000 and x[1].size <= 20000]
    assert len(small) >= len(cases) // 6
    return out, small


def expand_loop(form, src, capacity, num_in):
    """clo_expand.h: segment r owns the rows [e_(r-1), e_r); row j < min(total, capacity) gets r and j - e_(r-1)."""
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    seg, rank, at = [], [], 0
    for r in range(m):
        for k in range(counts[r]):
            if at + k < capacity:
                seg.append(r)
                rank.append(k)
        at += counts[r]
    return seg, rank, at


def test_expand_cases():
    resolved, small = _segmented_common("expand", F.expand_inputs)
    cases = [x[0] for x in resolved]
    assert {tuple(c["outs"]) for c in cases} == set(F.TE.SUBSETS) and {tuple(c["outs"]) for c in cases if not c["vs"]} == {o for o in F.TE.SUBSETS if not o[0]}
    seen = set()
    for c, counts, capacity, num_in, base in resolved:
        T, L = c["tile"], c["L"]
        taken = counts if num_in is None else counts[:num_in]
        ends = np.cumsum(taken)
        rows = min(int(ends[-1]) if ends.size else 0, capacity)
        if rows:                                                      # the ends that fall into each tile of output rows
            per_tile = np.bincount(ends[ends <= rows] // T, minlength=rows // T + 1)
            seen.update(("a tile with more than L ends",) if per_tile.max() > L else ())
            seen.update(("a tile with ends, L at the most",) if ((per_tile > 0) & (per_tile <= L)).any() else ())
    assert seen == {"a tile with more than L ends", "a tile with ends, L at the most"}, seen
    for c, counts, capacity, num_in, base in small:
        src = F.TE.source(c["form"], c["ct"], counts, base)
        seg, rank, total = expand(c["form"], src, capacity, num_in)
        ls, lr, lt = expand_loop(c["form"], src, capacity, num_in)
        assert total == lt and seg.tolist() == ls and rank.tolist() == lr, c


def segreduce_loop(op, form, src, values, sum_type, num_in):
    """clo_segreduce.h: the sum modulo 2^bits, the minimum or the maximum of the rows [min(e_(r-1), n), min(e_r, n)) after the C
    cast to the sum type; the identity for a segment without rows."""
    dt = np.dtype(F.TSR.NP[sum_type])
    bits = 8 * dt.itemsize
    mask = (1 << bits) - 1
    wrap = lambda x: (x & mask) - (1 << bits) if dt.kind == "i" and (x & mask) >> (bits - 1) else x & mask
    src = [int(x) for x in src]
    counts = [b - a for a, b in zip(src, src[1:])] if form == "offsets" else src
    m = len(counts) if num_in is None else min(len(counts), num_in)
    v = [wrap(int(x)) for x in values]
    ident = {"sum": 0, "min": int(np.iinfo(dt).max), "max": int(np.iinfo(dt).min)}[op]
    out, at = [], 0
    for r in range(m):
        rows = v[min(at, len(v)):min(at + counts[r], len(v))]
        at += counts[r]
        out.append(ident if not rows else wrap(sum(rows)) if op == "sum" else min(rows) if op == "min" else max(rows))
    return np.array([x & mask for x in out], dtype="u%d" % dt.itemsize).view(dt), at


def test_segreduce_cases():
    resolved, small = _segmented_common("segreduce", lambda c: (lambda r: (r[0], r[1].size, r[2], r[3]))(F.segreduce_inputs(c)))
    seen = set()
    for c, counts, rows, num_in, base in resolved:
        vals = F.segreduce_inputs(c)[1]
        assert vals.size == rows and vals.dtype == np.dtype(F.TSR.NP[c["vt"]])
        T = c["tile"]
        taken = counts if num_in is None else counts[:num_in]
        ends = np.minimum(np.cumsum(taken), rows)
        starts = np.concatenate(([0], ends[:-1]))
        info = np.iinfo(vals.dtype)
        for r in np.flatnonzero(ends - starts > 200).tolist():
            seg = vals[starts[r]:ends[r]]
            close = (int(ends[r]) + r) // T                                   # the tile of the merge step that closes the segment
            for ext, name in ((info.min, "min"), (info.max, "max")):
                at = np.flatnonzero(seg == ext)
                if at.size == 1 and (int(starts[r]) + int(at[0]) + r) // T != close and not (seg == (info.min + 1 if name == "min" else info.max - 1)).all():
                    seen.add("the %s of a segment lies in a tile other than the one it closes in" % name)
                    if c["op"] == name:
                        seen.add("... and the op is " + name)
        if c["op"] == "sum" and c["st"] in ("int", "uint") and rows:
            wide = np.add.reduceat(vals.astype(np.int64), starts[ends > starts]) if (ends > starts).any() else np.zeros(0, np.int64)
            if (np.abs(wide) >= 1 << 32).any():
                seen.add("a wrapped 32-bit sum")
    assert seen >= {"the min of a segment lies in a tile other than the one it closes in", "the max of a segment lies in a tile other than the one it closes in",
                    "... and the op is min", "... and the op is max", "a wrapped 32-bit sum"}, seen
    for c, counts, rows, num_in, base in small:
        vals = F.segreduce_inputs(c)[1]
        src = F.TSR.source(c["form"], c["ct"], counts, base)
        aggr, total = segreduce(c["op"], c["form"], src, vals, c["st"], num_in)
        la, lt = segreduce_loop(c["op"], c["form"], src, vals, c["st"], num_in)
        assert total == lt and aggr.dtype == la.dtype and np.array_equal(aggr, la), c


def test_segsort_cases():
    import cl_ops_amd as clo
    import test_segsort_cpu as SC
    resolved, small = _segmented_common("segsort", lambda c: (lambda r: (r[0], r[1].size, r[2], r[3]))(F.segsort_inputs(c)))
    cases = [x[0] for x in resolved]
    kts, sizes = list(F.TSS.KEY_NP), (1, 2, 4, 8)
    size_of = lambda c: np.dtype(F.TSS.KEY_NP[c["kt"]]).itemsize
    assert {(c["keys"], size_of(c)) for c in cases} == {(k, s) for k in F.SEGSORT_KEYS for s in sizes}
    assert {(c["kt"], c["mode"]) for c in cases} == {(kt, m) for kt in kts for m in F.TSS.MODES}
    assert {(c["form"], c["ct"], size_of(c)) for c in cases} == {(f, t, s) for f in ("counts", "offsets") for t in ("uint", "ulong") for s in sizes}
    for s in sizes:                                                            # every byte of every key size varies alone somewhere
        assert {c["digit"] for c in cases if c["keys"] == "one byte varies" and size_of(c) == s} == set(range(s)), s
    T = clo.segsort_tile(4, 0)
    seen = set()
    for c, counts, rows, num_in, base in resolved:
        assert c["tile"] == T
        keys = F.segsort_inputs(c)[1]
        assert keys.size == rows and keys.dtype == np.dtype(F.TSS.KEY_NP[c["kt"]]) and keys.flags.c_contiguous
        taken = counts if num_in is None else counts[:num_in]
        ends = np.minimum(np.cumsum(taken), rows)
        starts = np.concatenate(([0], ends[:-1]))
        ok = order_key(keys)
        if c["keys"] in ("sorted", "reversed") and rows > 1:
            d = np.diff(ok.astype(object)) if rows < 3000 else np.diff(ok.astype(np.float64))
            assert (d >= 0).all() if c["keys"] == "sorted" else (d <= 0).all(), c
        if c["keys"] == "all equal" and rows:
            assert np.unique(ok).size == 1
        if c["keys"] == "few":
            assert np.unique(ok).size <= 8
        if c["keys"] == "one byte varies" and rows > 1000:
            assert 100 < np.unique(ok).size <= 256 and np.unique(ok >> ok.dtype.type(8 * c["digit"])).size <= 256
        if c["keys"] == "sorted per segment" and rows:
            p, _ = segsort(c["form"], F.TSS.source(c["form"], c["ct"], counts, base), keys, num_in)
            assert np.array_equal(p, np.arange(p.size, dtype=np.uint32)), c   # already the answer
        if keys.dtype.kind == "f" and rows:
            b = keys.view("u%d" % keys.itemsize)
            seen.update(("nan payloads of both signs",) if len(set(b[np.isnan(keys)].tolist())) > 2 and len(set(np.signbit(keys[np.isnan(keys)]).tolist())) == 2 else ())
            seen.update(("both zeros",) if len(set(b[keys == 0].tolist())) > 1 else ())
        cross = np.flatnonzero((ends > starts) & (starts // T != (np.maximum(ends, 1) - 1) // T))      # only these have a mask
        segs = [(int(starts[r]), int(ends[r]), SC.move_mask(int(starts[r]), int(ends[r]), T)) for r in cross.tolist()]
        for s0, e0, mask in segs:
            assert mask
            seen.add("an %s number of moves" % ("odd" if bin(mask).count("1") % 2 else "even"))
            if "0" in bin(mask)[2:].rstrip("0"):                               # a pass at rest between two moves
                seen.add("a mask with a gap")
            if mask.bit_length() - 1 >= 6:
                seen.add("a highest bit of 6 or more")
        if SC.opposite_moves_in_one_tile(segs, T):
            seen.add("a tile whose two boundary segments move in opposite directions")
    assert seen >= {"nan payloads of both signs", "both zeros", "an odd number of moves", "an even number of moves", "a mask with a gap", "a highest bit of 6 or more",
                    "a tile whose two boundary segments move in opposite directions"}, seen
    for c, counts, rows, num_in, base in small:
        keys = F.segsort_inputs(c)[1]
        src = F.TSS.source(c["form"], c["ct"], counts, base)
        p, total = segsort(c["form"], src, keys, num_in)
        lp, lt = SC._loop(c["form"], src, keys, num_in)
        assert total == lt and p.tolist() == lp, c
