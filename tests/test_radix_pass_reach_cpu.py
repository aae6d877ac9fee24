"""What the cases of tests/test_gpu_radix_pass.py reach inside clo_radix4_pair_kernel, proved without a GPU by the model
of tests/radix_pass_model.py: the path of every case (checked against the library's own host functions, so that a moved
threshold fails here instead of silently losing reach), and per stratum — element size x (LB, HB) x tile shape x digit
stream or none — the branches of the scatter that its launches take."""
import numpy as np
import pytest

import radix_pass_model as M
import test_gpu_radix_pass as G

PAIR_SET = sorted(set(M.PAIRS.values()))                 # the six (LB, HB)
STRATA = ([(es, lb, hb, "pair512", False) for es in (1, 2, 4, 8) for lb, hb in PAIR_SET]
          + [(8, lb, hb, "pair1024", False) for lb, hb in PAIR_SET] + [(8, 4, 4, "pair1024", True)]
          + [(4, 4, 4, "pair1024", False), (4, 4, 4, "pair1024", True)])
_SIM = {}


def elements_of(case):
    a = G.keys_of(case)
    if case["op"] == "kv":
        return (a.astype(np.uint64) << np.uint64(32)) | G.values_of(case).astype(np.uint64)
    return a


def sim(case):
    """[(pass, record)] of the case, computed once. Every pass is analysed tile by tile, except at 2^26 elements, where
    the first pass, the aimed one and the last are (the others are still run, and say whether they move anything)."""
    if case["id"] not in _SIM:
        es, shift = G.sim_geometry(case)
        a = elements_of(case)
        only = None if a.size < G.N_BIG4 else {0, case["pstar"], len(M.schedule(a.size, es, shift, case["bits"], case["db"])) - 1}
        recs, out = M.simulate(a, es, shift, case["bits"], case["kind"], case["db"], only)
        if a.size < G.N_BIG8:                            # the model sorts: its passes end in the stable order of the key
            assert np.array_equal(out, a[M.stable_order(a, shift, case["bits"], case["kind"])]), case["id"]
        # pass p* meets the digits as make_keys wrote them: an even tile is written without the generator's random stream
        if case["family"] in ("one_digit_per_tile", "single_mixed"):
            d = recs[case["pstar"]][0]
            tile = M.shape(a.size, es)[2]
            t = (a.size - 1) // tile // 2 * 2
            f = M.forward(a[t * tile:(t + 1) * tile], shift, case["bits"], case["kind"])
            assert (M.pass_digit(f, d) == (7 * t) % (d["mask"] + 1)).all(), case["id"]
        _SIM[case["id"]] = recs
    return _SIM[case["id"]]


def case_path(case):
    es, _ = G.sim_geometry(case)
    return M.path(case["n"], es, case["db"], 0 if case["sweep0"] else None)


def stratum_of(case, d):
    es, _ = G.sim_geometry(case)
    return (es, d["LB"], d["HB"], case_path(case), d["dig"])


@pytest.fixture(scope="module")
def reach():
    """stratum -> list of (case, pass, record) of every launch of every case."""
    out = {s: [] for s in STRATA}
    for c in G.CASES:
        for d, r in sim(c):
            if r["analysed"]:
                out[stratum_of(c, d)].append((c, d, r))
    return out


def test_the_table_names_every_family_size_and_field():
    assert {c["family"] for c in G.CASES} == set(M.FAMILIES)
    for es in (1, 2, 4, 8):
        small = [c for c in G.CASES if c["op"] == "keys" and c["es"] == es and c["n"] < G.N_BIG8]
        assert {c["n"] for c in small} == set(G.small_sizes(es)) and min(G.small_sizes(es)) > 1024 * M.items_of(es)
        assert {c["db"] for c in small} == set(range(1, 9))
        assert {c["family"] for c in small if c["kind"] == 0} >= {"single_mixed", "short_runs", "two_runs", "one_digit_per_tile"}
    assert {c["family"] for c in G.CASES if c["n"] < G.N_BIG8 and c["op"] == "keys"} == set(M.FAMILIES)
    fields4 = {(c["shift"], c["bits"]) for c in G.CASES if c["op"] == "keys" and c["es"] == 4 and c["n"] < G.N_BIG8}
    assert fields4 >= {(0, 32), (3, 29), (5, 12), (0, 20)}
    big8 = [c for c in G.CASES if c["op"] == "keys" and c["n"] == G.N_BIG8]
    assert {M.PAIRS[c["db"]] for c in big8} == set(PAIR_SET) and all(c["es"] == 8 and 12 <= c["bits"] <= 24 for c in big8)
    assert {c["family"] for c in big8} == {"single_mixed", "short_runs", "two_runs"}
    big4 = [(c["db"], c["shift"], c["bits"], c["family"]) for c in G.CASES if c["n"] == G.N_BIG4]
    assert big4 == [(4, 3, 29, "short_runs"), (8, 5, 20, "two_runs"), (4, 0, 32, "single_mixed")]
    assert sum(c["misaligned"] for c in G.CASES) * 2 in range(len(G.CASES) - 4, len(G.CASES) + 5)     # half of them
    assert max(c["n"] for c in G.CASES if c["sweep0"]) <= 17 * 8192 and all(c["n"] in (G.N_BIG8, G.N_BIG4) for c in G.CASES if not c["sweep0"])


def test_every_case_is_on_the_pair_passes_and_the_library_agrees(monkeypatch):
    from cl_ops_amd._hip import lib
    try:
        for sweep0 in (True, False):
            if sweep0:
                monkeypatch.setenv("CLO_RADIX_SWEEP", "0")
            else:
                monkeypatch.delenv("CLO_RADIX_SWEEP", raising=False)
            monkeypatch.delenv("CLO_RADIX_NO_DIGITS", raising=False)
            lib.clo_hip_env_refresh()
            for c in G.CASES:
                if c["sweep0"] != sweep0:
                    continue
                es, _ = G.sim_geometry(c)
                want = "pair1024" if c["n"] >= G.N_BIG8 else "pair512"
                assert case_path(c) == want, c["id"]
                assert lib.clo_hip_radix_polls(c["n"], es, c["db"]) == 0, c["id"]
                big44 = want == "pair1024" and c["db"] in (4, 8)
                assert lib.clo_hip_radix_takes_first_digits(c["n"], es, 0, c["db"]) == (1 if big44 else 0), c["id"]
                assert any(d["dig"] for d in M.schedule(c["n"], es, 0, 8 * es, c["db"])) == big44
            # and on both sides of every threshold the model's path is the library's
            for es in (1, 2, 4, 8):
                small_max = 1024 * M.items_of(es)
                big = M.big_tile_bytes(es) // es
                tile = 512 * M.items_of(es)
                for n in (small_max, small_max + 1, 256 * tile, 256 * tile + 1, big - 1, big, 2 * tile, tile + 1):
                    for db in (3, 4, 8):
                        p = M.path(n, es, db, 0 if sweep0 else None)
                        assert lib.clo_hip_radix_polls(n, es, db) == (1 if M.sweep_applies(n, es, db, 0 if sweep0 else None) else 0), (n, es, db)
                        if p != "one_launch":
                            assert (p == "sweep") == bool(lib.clo_hip_radix_polls(n, es, db))
                        takes = lib.clo_hip_radix_takes_first_digits(n, es, 0, db)
                        assert takes == (1 if (M.big_tiles(n, es) and db in (4, 8) and not M.sweep_applies(n, es, db, 0 if sweep0 else None)) else 0), (n, es, db)
    finally:
        monkeypatch.undo()
        lib.clo_hip_env_refresh()


def test_the_passes_before_the_aimed_one_are_copies():
    """Unsigned keys of the four tile-wise families have zero bits below pass p*: every earlier launch finds all its
    tiles `single` and moves nothing (sim() checks that pass p* then meets the digits as make_keys wrote them)."""
    seen = 0
    for c in G.CASES:
        if c["family"] not in ("one_digit_per_tile", "single_mixed", "short_runs", "two_runs"):
            continue
        recs = sim(c)
        for d, r in recs[:c["pstar"]]:
            assert r["identity"] and r["constant"] and (not r["analysed"] or r["split_full"] == r["split_partial"] == 0), (c["id"], d["p"])
            seen += 1
    assert seen > 100


def test_every_stratum_is_reached(reach):
    for s in STRATA:
        es, lb, hb, path, dig = s
        launches = reach[s]
        assert launches, s
        aimed = [c for c, d, r in launches if d["p"] == c["pstar"]]
        assert aimed, "no case aims at %r" % (s,)
        vec = 1 if es == 8 else 4
        recs = [r for _, _, r in launches]
        assert any(r["single_full"] and r["single_partial"] and (r["split_full"] or r["split_partial"]) for r in recs), \
            "%r: no launch with a single full tile, a single partial tile and a split tile" % (s,)
        lengths = set().union(*(r["run_lengths"] for r in recs))
        if vec == 4:
            assert set().union(*(r["vector_residues"] for r in recs)) == {0, 1, 2, 3}, s
            assert set().union(*(r["cuts"] for r in recs)) == {1, 2, 3}, s
        else:
            assert {1, 2} <= lengths and any(r["item_edge"] for r in recs), s
        assert 1 in lengths, s
        assert any(r["whole_tile_run"] for r in recs), s
        assert any(r["all_digits"] for r in recs), s
        assert any(r["partial_groups"] for r in recs) and any(r["split_partial"] for r in recs), s


def test_the_families_do_what_their_names_say(reach):
    """Per family, at the pass it aims at (so that a family dropped from the table is missed here, by name)."""
    by = {}
    for c in G.CASES:
        by.setdefault(c["family"], []).append((c, sim(c)[c["pstar"]]))
    for c, (d, r) in by["one_digit_per_tile"]:
        assert r["split_full"] == r["split_partial"] == 0 and r["tiles"] == r["single_full"] + r["single_partial"] and r["whole_tile_run"], c["id"]
    assert any(not r["identity"] for c, (d, r) in by["one_digit_per_tile"])           # whole tiles change places
    for c, (d, r) in by["single_mixed"]:
        assert r["single_full"] and r["split_full"] and r["single_partial"] == 1, c["id"]
    for c, (d, r) in by["short_runs"]:
        assert {1, 2, 3, 4, 5} <= r["run_lengths"] and r["single_full"] == 0, c["id"]
        assert r["all_digits"] == (d["mask"] + 1 == 1 << (d["LB"] + d["HB"])), c["id"]
    for c, (d, r) in by["two_runs"]:
        es, _ = G.sim_geometry(c)
        _, items, tile, _ = M.shape(c["n"], es)
        cs = M.two_runs_lengths(items, tile)
        want = {cs[t % len(cs)] for t in range(c["n"] // tile)}           # (the full tiles)
        assert want <= r["run_lengths"] and {tile - x for x in want} <= r["run_lengths"], c["id"]
        if c["n"] // tile >= len(cs):
            assert want == set(cs) and (es == 8 or r["cuts"] == {1, 2, 3}), c["id"]
    whole = [c for c, _ in by["sorted"] + by["reversed"] + by["skew90"]]
    assert {(G.sim_geometry(c)[0] if c["op"] == "keys" else 0, c["kind"]) for c in whole if c["kind"]} >= \
        {(1, 1), (2, 1), (2, 2), (4, 1), (4, 2), (8, 1), (8, 2)}
    for c, (d, r) in by["reversed"]:
        assert not r["identity"], c["id"]
    for c, (d, r) in by["skew90"]:
        assert max(r["run_lengths"]) > 0.8 * min(c["n"], M.shape(c["n"], G.sim_geometry(c)[0])[2]), c["id"]


def test_over_the_whole_table(reach):
    last = [(c, d, r) for s in STRATA for c, d, r in reach[s] if d["last"]]
    assert any(d["mask_hi"] == 0 and d["p"] == c["pstar"] and d["p"] > 0 for c, d, r in last)
    assert any(d["lo_bits"] < d["LB"] and d["p"] == c["pstar"] for c, d, r in last)
    assert any(d["mask_hi"] == 0 and c["n"] == G.N_BIG4 for c, d, r in last)
    # both ways of gathering four next digits on 4-byte big tiles, each on split tiles and with a digit above 127 next
    for how in ("perm", "shifts"):
        hits = [(c, d, r) for c, d, r in reach[(4, 4, 4, "pair1024", True)] if d["gather"] == how]
        assert any(r["split_full"] for c, d, r in hits), how
        assert any(r["single_full"] for c, d, r in hits) or how == "shifts", how
    assert all(d["gather"] is None for s in STRATA if s[0] != 4 or not s[4] for c, d, r in reach[s])
    # the key transforms: forward in the first launch, inverse in the last, signed and IEEE
    kinds = {(G.sim_geometry(c)[0], c["es"], c["op"], c["kind"]) for c in G.CASES if c["kind"]}
    assert kinds >= {(1, 1, "keys", 1), (2, 2, "keys", 1), (2, 2, "keys", 2), (4, 4, "keys", 1), (4, 4, "keys", 2), (8, 8, "keys", 1), (8, 8, "keys", 2)}
    assert kinds >= {(8, 1, "kv", 1), (8, 2, "kv", 2), (8, 4, "kv", 1), (8, 4, "kv", 2)}
    for c in G.CASES:
        if c["kind"]:
            es, shift = G.sim_geometry(c)
            a = elements_of(c)
            f = M.forward(a, shift, c["bits"], c["kind"])
            assert not np.array_equal(f, a) and np.array_equal(M.inverse(f, shift, c["bits"], c["kind"]), a)
            top = (f >> f.dtype.type(shift + c["bits"] - 1)) & f.dtype.type(1)
            assert (top.min() == 0 and top.max() == 1) or c["family"] == "one_digit_per_tile", c["id"]       # both signs
    # key-value passes: keys of 1, 2 and 4 bytes on both tile shapes, aimed at the pass that reads the arrays and at the
    # one that writes them; values and argsort; keys_out or none; one pass in place
    kv = [c for c in G.CASES if c["op"] == "kv"]
    for ks in (1, 2, 4):
        for path in ("pair512", "pair1024"):
            mine = [c for c in kv if c["es"] == ks and case_path(c) == path]
            assert {c["family"] for c in mine} >= {"short_runs", "two_runs", "single_mixed"}
            assert any(c["pstar"] == 0 for c in mine) and any(c["pstar"] == len(sim(c)) - 1 for c in mine)
            assert {c["values"] for c in mine} == {True, False} and {c["keys_out"] for c in mine} == {True, False}
        assert {c["n"] for c in kv if c["es"] == ks} >= {2 * 4096 + 1, 9 * 4096 + 3, G.N_BIG8}
    assert all(c["db"] in (4, 8) for c in kv)
    assert [c for c in kv if c["inplace"] and c["es"] == 1 and c["db"] == 8 and len(sim(c)) == 1]


def test_no_vector_of_a_full_tile_ends_outside_the_array(reach):
    """The scatter's guard `gi0 <= n - VEC` on a vector whose first and last digit agree never fails in any launch of
    any case, and no input can make it fail: the vector lies inside one run of its tile, and with correct counters
    the run's destination [toff, toff + count) lies inside [0, n), so its last element's index is below n. The guard
    is there for counters that are wrong, which is why no case reaches its other side."""
    for s in STRATA:
        for c, d, r in reach[s]:
            assert r["guard_fails"] == 0, (c["id"], d["p"])
