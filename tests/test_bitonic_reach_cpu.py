"""What the cases of tests/test_gpu_bitonic_schedule.py reach, proved without a GPU by the model of
tests/bitonic_schedule_model.py. A stratum is (element size) x (key mode 0-3, or run-time compiled `get_key`, or
run-time compiled `compare`) x (kernel family) x (steps); it counts as reached where its pass lies in the LAST stage of a
case's sort, at the smallest size at which that happens. The strata come from walking the model over every size up to
2^24 and every CLO_BITONIC_MERGE2; the kernels the code instantiates and no sort up to 2^24 ends with are named in
UNREACHED with the reason. Besides: both sides of the row-size branches of s2_cost and every term of use_m2 decide the
cut of some case's last stage, the cuts DESIGN 4.3 quotes, and that no row of the table is idle — every single row
taken out leaves something unreached."""
import itertools

import pytest

import bitonic_schedule_model as M
import test_gpu_bitonic_schedule as G

MAX_LOG2 = 24
MERGE2_MODES = (1, 0, 2)
JIT_KINDS = ("get_key", "compare")

# Kernels that exist and end no sort of at most 2^24 elements: (element size, family, steps) -> why
UNREACHED = {
    (1, "strided2", 9): "32-byte rows are costed 250: 2 + 7 is cheaper at every size",
    (1, "strided2", 10): "16-byte rows are costed 250: 3 + 7 is cheaper at every size",
    (2, "strided2", 10): "32-byte rows are costed 250: 3 + 7 is cheaper at every size",
    (8, "strided", 6): "6 steps right above the tile are one two-level pass (79 against 81); 6 plain steps first come at 14 = 6 + 8 steps, 2^27 elements",
}


def aot_universe(es, mode):
    """(family, steps) of every kernel tiled_run<E, MODE> can launch."""
    q, klf = M.q_of(es), M.klf_of(es)
    out = {("step", 1), ("presort", klf * (klf + 1) // 2), ("merge", klf)}
    out |= {("tile_rt", kl * (kl + 1) // 2) for kl in range(q, klf)}
    out |= {("strided", ns) for ns in range(1, M.qs_of(es, mode) + 1)}
    out |= {("strided2", b2) for b2 in range(q + 2, 2 * q + 1)}
    if mode:
        out.add(("merge2", klf + 1))
    return out


def aot_strata(es, mode):
    """(family, steps) -> smallest log2 numel whose last stage has it, under any CLO_BITONIC_MERGE2."""
    out = {}
    for T in range(1, MAX_LOG2 + 1):
        for m2 in MERGE2_MODES:
            for l in M.last_stage(M.aot_schedule(es, mode, 1 << T, m2)):
                out.setdefault((l.family, l.steps), T)
    return out


def jit_strata(es):
    out = {}
    for T in range(1, MAX_LOG2 + 1):
        for l in M.last_stage(M.jit_schedule(es, 1 << T)):
            out.setdefault((l.family, l.steps), T)
    return out


def s2_deciders(es, mode, T, m2):
    """{(side, as_side)}: the last stage's cut changes when the two-level passes on `side` of s2_cost's row-size branches
    are costed as `as_side` would cost them — that side of the branch decides the cut."""
    base = M.last_stage(M.aot_schedule(es, mode, 1 << T, m2))
    return {(a, b) for a, b in itertools.permutations(M.S2_SIDES, 2)
            if M.last_stage(M.aot_schedule(es, mode, 1 << T, m2, (a, b))) != base}


def requirements():
    """Everything the table has to reach: name -> predicate over a row of G.ROWS or G.JIT_ROWS."""
    req = {}
    for es in (1, 2, 4, 8):
        for mode in G.MODES[es]:
            for (family, steps), T in aot_strata(es, mode).items():
                req[("aot", es, mode, family, steps)] = (es, mode, T)
        for (family, steps), T in jit_strata(es).items():
            for kind in JIT_KINDS:
                req[("jit", es, kind, family, steps)] = (es, kind, T)
    # decisions of the host code: whatever decides some last stage of some sort up to 2^24
    for es in (1, 2, 4, 8):
        for mode in G.MODES[es]:
            for T in range(M.klf_of(es) + 1, MAX_LOG2 + 1):
                for m2 in MERGE2_MODES:
                    d = M.m2_decider(es, mode, T, T, m2)[1]
                    if d:
                        req[("use_m2", d)] = None
                    for sides in s2_deciders(es, mode, T, m2):
                        req[("s2_cost",) + sides] = None
    for es in (1, 2, 4, 8):
        req[("not_a_power_of_two", es)] = None
    return req


def covered_by(row, req):
    """The requirements a row of the table meets."""
    out = set()
    if row[1] in JIT_KINDS:
        es, kind, T = row
        for l in M.last_stage(M.jit_schedule(es, 1 << T)):
            if req.get(("jit", es, kind, l.family, l.steps)) == (es, kind, T):
                out.add(("jit", es, kind, l.family, l.steps))
        return out
    es, mode, T, m2 = row
    numel = G.row_numel(row)
    assert M.log2u(M.nlpo2(numel)) == T
    for l in M.last_stage(M.aot_schedule(es, mode, numel, m2)):
        if req.get(("aot", es, mode, l.family, l.steps)) == (es, mode, T):
            out.add(("aot", es, mode, l.family, l.steps))
    if T > M.klf_of(es):
        d = M.m2_decider(es, mode, T, T, m2)[1]
        if d:
            out.add(("use_m2", d))
        out |= {("s2_cost",) + s for s in s2_deciders(es, mode, T, m2)}
    if row in G.NOT_POW2:
        assert mode != 0 and numel & (numel - 1)
        out.add(("not_a_power_of_two", es))
    return out


@pytest.fixture(scope="module")
def reach():
    req = requirements()
    rows = list(G.ROWS) + list(G.JIT_ROWS)
    return req, {r: covered_by(r, req) for r in rows}


def test_every_stratum_and_every_decision_is_reached(reach):
    req, cover = reach
    reached = set().union(*cover.values())
    missing = sorted(set(req) - reached, key=str)
    assert not missing, "reached by no case, or not at the smallest size: %r" % (missing,)
    # the numbers the table was sized by
    assert req[("aot", 4, 1, "strided2", 10)] == (4, 1, 24) and req[("aot", 2, 1, "strided2", 9)] == (2, 1, 23)
    assert req[("aot", 1, 1, "strided2", 8)] == (1, 1, 22)
    assert max(T for k, v in req.items() if k[0] == "jit" and k[1] != 8 for T in [v[2]]) == 21
    assert max(T for k, v in req.items() if k[0] == "jit" and k[1] == 8 for T in [v[2]]) == 20
    for es in (1, 2, 4):
        assert {k[4] for k in req if k[:2] == ("jit", es) and k[3] == "jit_strided2l"} == {6, 7, 8}
        assert {k[4] for k in req if k[:2] == ("jit", es) and k[3] == "jit_strided"} == {1, 2, 3, 4, 5}
    assert {k[4] for k in req if k[:2] == ("jit", 8) and k[3] == "jit_strided2l"} == {5, 6, 7, 8}
    assert {k[4] for k in req if k[:2] == ("jit", 8) and k[3] == "jit_strided"} == {1, 2, 3, 4}


def test_no_row_is_idle(reach):
    """Taking any one row out of the table leaves a stratum or a decision unreached."""
    req, cover = reach
    count = {}
    for r, c in cover.items():
        for k in c:
            count[k] = count.get(k, 0) + 1
    idle = [r for r, c in cover.items() if not any(count[k] == 1 for k in c)]
    assert not idle, idle


def test_what_no_case_reaches_is_named():
    """The kernels the code instantiates minus the strata that exist up to 2^24 are UNREACHED, no more and no less; a
    1-byte element has no IEEE key (make_desc refuses it), so MODES has no such mode."""
    left = set()
    for es in (1, 2, 4, 8):
        for mode in G.MODES[es]:
            left |= {(es,) + k for k in aot_universe(es, mode) - set(aot_strata(es, mode))}
        q, kl = M.q_of(es), M.JIT_TB + M.q_of(es)
        jit_universe = ({("jit_step", 1), ("jit_merge", kl)} | {("jit_tile", k * (k + 1) // 2) for k in range(q, kl + 1)}
                        | {("jit_strided", ns) for ns in range(1, q + 1)} | {("jit_strided2l", ns) for ns in range(q + 1, min(M.JIT_TB, 2 * q) + 1)})
        assert jit_universe == set(jit_strata(es)), es
    assert left == set(UNREACHED)
    assert 3 not in G.MODES[1] and M.mode_of(1, 0, 8, 1, 2) == 0
    # and at no size at all, for the three that the cost table rules out
    for es, _, b2 in [k for k in UNREACHED if k[1] == "strided2"]:
        assert M.s2_side(b2, es) == "less"
        for mode in G.MODES[es]:
            assert all(M.best_cut(h, es, mode)[1] != b2 for h in range(1, 40))


def test_both_sides_of_the_cost_branches_and_of_use_m2_decide_a_cut(reach):
    req, cover = reach
    reached = set().union(*cover.values())
    # s2_cost: `row >= 128` both ways, `row >= 64` both ways
    assert {("s2_cost", "line", "half"), ("s2_cost", "line", "less")} & reached           # a pass on whole lines wins because it is
    assert {("s2_cost", "half", "less")} <= reached                                       # the 10-step pass at 124 wins, at 250 it would not
    assert {("s2_cost", "less", "half"), ("s2_cost", "less", "line")} <= reached          # a pass at 250 loses, at 124 it would win
    # use_m2: taken for either reason, and kept away by every term alone
    assert {("use_m2", d) for d in ("forced", "saves_a_pass")} <= reached
    assert {("use_m2", "not:" + t) for t in M.M2_TERMS} <= reached
    # and the rows that are there for these hold what their comments say
    assert ("use_m2", "saves_a_pass") in cover[(4, 1, 24, 1)] and ("use_m2", "not:whole_keys") in cover[(4, 0, 24, 1)]
    assert ("use_m2", "not:four_bytes") in cover[(1, 1, 22, 1)] and ("s2_cost", "less", "half") in cover[(2, 1, 24, 1)]
    assert ("use_m2", "not:switched_on") in cover[(4, 1, 24, 0)] and ("use_m2", "not:enough_tiles") in cover[(4, 1, 15, 1)]
    assert ("use_m2", "not:saves_a_pass") in cover[(4, 1, 20, 1)]


def _cut(h, es=4, mode=1):
    return [l.steps for l in M.strided_passes(h + M.klf_of(es), h + M.klf_of(es), M.klf_of(es), es, mode)]


def test_the_cuts_the_design_quotes():
    assert _cut(11) == [4, 7] and _cut(12) == [5, 7]
    s = M.aot_schedule(4, 1, 1 << 26, 1)
    assert len(s) == 25 and [l.stage for l in s if l.family == "merge2"] == [15, 24, 25]
    assert M.label_counts(s) == {"bitonic_step": 0, "bitonic_presort": 1, "bitonic_strided": 6, "bitonic_strided2": 6, "bitonic_tile": 12}
    assert len(M.aot_schedule(4, 1, 1 << 26, 0)) == 27
    j = M.jit_schedule(4, 1 << 26)
    assert [(l.family, l.steps) for l in j if l.stage == 26] == [("jit_strided", 5), ("jit_strided2l", 8), ("jit_merge", 13)]
    assert sum(l.family in ("jit_strided", "jit_strided2l") for l in j) == 18 and sum(l.family == "jit_merge" for l in j) == 13
    assert len(M.aot_schedule(4, 1, 1 << 16, 1)) == 5                      # sbitonic's 2^16 keys in 5 launches
    assert len(M.aot_schedule(4, 1, 16, 1)) == 10 and len(M.jit_schedule(4, 16)) == 10       # below 2^Q: one launch per step
    assert len(M.jit_schedule(4, (1 << 10) - 1)) == 55                     # the flip network


def test_the_model_agrees_with_the_library_where_the_host_can_be_asked():
    """The thresholds T < Q and T < KLF through clo_hip_bitonic_lds_bytes, the padding through
    clo_hip_bitonic_padded_numel: a moved threshold fails here instead of silently losing reach."""
    from cl_ops_amd._hip import lib
    import ctypes as C
    f = lib["clo_hip_bitonic_lds_bytes"]
    f.restype, f.argtypes = C.c_size_t, [C.c_size_t, C.c_int, C.c_int]
    for es in (1, 2, 4, 8):
        q, klf = M.q_of(es), M.klf_of(es)
        for T in range(1, 20):
            for numel in {(1 << T), (1 << T) - 1, (1 << (T - 1)) + 1} - {0, 1}:
                assert lib.clo_hip_bitonic_padded_numel(numel) == M.nlpo2(numel)
                first = M.aot_schedule(es, 1, numel, 1)[0].family
                tile = {"step": 0, "tile_rt": 256 << q, "presort": 1 << klf}[first]
                assert f(numel, es, 1) == (tile + tile // 32) * es, (es, numel)


def test_the_table_rotates_layouts_views_fields_and_directions():
    rows = list(enumerate(G.ROWS))
    for es in (1, 2, 4, 8):
        mine = [(k, r) for k, r in rows if r[0] == es]
        assert {G.LAYOUTS[k % 5] for k, r in mine if r[2] >= M.klf_of(es)} == set(G.LAYOUTS)
        general = [(k, r) for k, r in mine if r[1] == 0]
        assert {G.row_field(k, es)[:3] for k, r in general} == set(G.FIELDS[es])
        assert {G.row_field(k, es)[3] for k, r in general} == ({0, 1} if es > 1 else {0})
        assert G.BOTH_DIRECTIONS_LOG2 > M.klf_of(es)                                              # both directions above the tile
        if es in (2, 4):                                              # (1-byte elements have one row above 2^21, 8-byte ones none)
            assert {G.general_direction(k) for k, r in general if r[2] > G.BOTH_DIRECTIONS_LOG2} == {0, 1}
        for k, r in general:
            assert M.mode_of(es, *G.row_field(k, es)) == 0
    assert abs(sum(k % 2 for k, _ in rows) * 2 - len(rows)) <= 1
    # two-valued and 50-valued keys both end a sort with every ahead-of-time family under general keys
    fam = {}
    for k, r in rows:
        if r[1] == 0:
            for l in M.last_stage(M.aot_schedule(*r)):
                fam.setdefault(l.family, set()).add(G.LAYOUTS[k % 5] == "two_values")
    assert all(v == {True, False} for f, v in fam.items() if f != "step"), fam


def test_the_sorter_rows_route_as_they_say():
    seen = set()
    for alg, et, kt, compare, get_key, n, how in G.SORTER_ROWS:
        got, es, spec = M.route(et, kt, compare, get_key)
        assert got == how, (et, compare, get_key)
        assert M.sorter_schedule(et, n, kt, compare, get_key)[1] is not None
        seen.add((alg, how if how == "jit" else M.mode_of(es, *spec[:4])))
    assert {h for _, h in seen} == {"jit", 0, 1, 2, 3} and {a for a, _ in seen} == {"sbitonic", "abitonic"}
    # the expressions of the run-time compiled cases are refused by the parser, the usual ones are not
    for (es, kind), (et, expr, _) in G.JIT_EXPR.items():
        assert M.route(et, None, expr if kind == "compare" else None, expr if kind == "get_key" else None)[0] == "jit"
    assert M.route("float", get_key="-(x)")[0] == "jit" and M.route("double", get_key="-(x)")[0] == "jit"
    assert M.route("uint", get_key="((x) & 0x0fffffff)") == ("aot", 4, (0, 28, 4, 0, 0))
    assert M.route("ulong", "uint", get_key="(uint) ((x) >> 32)") == ("aot", 8, (32, 32, 4, 0, 0))
    assert M.route("uint", compare="((a) < (b))") == ("aot", 4, (0, 32, 4, 0, 1))
    assert M.route("float", get_key="(x) >> 1")[0] == "jit"                 # a float key is the whole key type
    assert M.route("ulong", get_key="(x) & 0xFF00")[0] == "jit"              # only contiguous low masks are built
