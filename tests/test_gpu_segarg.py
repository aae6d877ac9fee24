"""CloSegArg (include/clo_segarg.h) on the GPU against the numpy model of tests/segarg_model.py, bit for bit. Every array
is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); idx_out, val_out and num_out are pre-filled with the pattern, and after every call num_out is the
model's unclamped total, the m rows written equal the model's (val_out as bits), and the guards, every input and every row
at index >= m are unchanged. With T = clo_hip_segarg_tile, the merge steps (segment ends plus rows) of a tile: m + n around
the tile edges x count patterns x ops, ties, forms and count types; ties decided across a lane's, a wave's and a tile's
edge and across a whole tile; the extremum in the carried part and in the closing tile; runs of T + 5 and of 2^20 empty
segments; rows that hold the identity value; every value type at its extremes (floats: both zeros, infinities, NaNs of
both signs); totals above n and num_in below, at and above; cross-checks against CloSegReduce and CloSegSort; val_out
absent; element-aligned views, the host form, two queues; the thin ABI's status codes; a captured graph replayed on other
counts and values; a chain behind CloBucket's offsets; offsets that do not ascend (in bounds, contents not compared); a
segment of equal values carried through a whole trip of the carry scan; indices above 2^31 against a closed form."""
import numpy as np
import pytest

from segarg_model import FORMS, NONE, NP, OPS, TIES, none_value, segarg
from test_gpu_histogram import Region
from test_gpu_segreduce import PATTERNS, counts_of, source

pytestmark = pytest.mark.gpu

CDT = {"uint": np.uint32, "ulong": np.uint64}
TYPES = tuple(NP)


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def T(dev):
    clo = dev[0]
    t = clo.segarg_tile(4)
    assert t >= 1024 and t % 256 == 0 and clo.segarg_tile(8) == t
    return t


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def values_for(vt, n, seed=0):
    """Half of the values from five letters, so that ties abound in every segment; a quarter at the type's extremes and
    special values (the none values, both zeros, infinities, NaNs of both signs and two payloads); the rest any bits."""
    rng = np.random.default_rng(2000 + seed)
    dt = np.dtype(NP[vt])
    ut = np.dtype("u%d" % dt.itemsize)
    bits = rng.integers(0, np.iinfo(ut).max, n, dtype=ut, endpoint=True)
    if dt.kind == "f":
        inf, sign = np.array([np.inf], dt).view(ut)[0], ut.type(1 << (8 * dt.itemsize - 1))
        letters = np.array([1.5, -1.5, 0.0, 7.0, -7.0], dt).view(ut)
        special = np.array([0, sign, inf, inf | sign, inf + 1, (inf + 1) | sign, inf + 77, (inf + 77) | sign, np.iinfo(ut).max, np.iinfo(ut).max >> 1], ut)
    else:
        info = np.iinfo(dt)
        letters = np.array([0, 1, 5, info.max // 3, info.min // 3 if info.min else 9], dt).view(ut)
        special = np.array([info.min, info.max, info.min + 1, info.max - 1, -1 if info.min < 0 else info.max // 2 + 1], dt).view(ut)
    pick = rng.random(n)
    bits[pick < 0.5] = rng.choice(letters, int((pick < 0.5).sum()))
    ext = (pick >= 0.5) & (pick < 0.75)
    bits[ext] = rng.choice(special, int(ext.sum()))
    return bits.view(dt)


def run_arg(dev, op, tie, form, ct, vt, counts, n, what, num_in=None, base=0, offs=(0, 0, 0, 0), obj=None, q=None, src=None, compare=True, seed=0,
            vals=None, with_val=True, want=None):
    """One call on views at byte offsets offs = (counts_or_offsets, values_in, idx_out, val_out) with n rows of values;
    checks everything and returns (total, idx, val). src: the input as it is (broken preconditions); compare False: the
    rows' contents are not compared; vals: the n values, instead of values_for(vt, n, seed); want: (idx, val, total)
    instead of the model's."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = source(form, ct, counts, base)
    m_h = src.size - (1 if form == "offsets" else 0)
    if vals is None:
        vals = values_for(vt, n, seed)
    assert vals.dtype == NP[vt] and vals.size == n
    idx, val, total = (want or segarg(op, tie, form, src, vals, num_in)) if compare else (None, None, None)
    what = "%s %s %s %s %s n %d, %s" % (op, tie, form, ct, vt, n, what)
    vs = np.dtype(NP[vt]).itemsize
    sa = obj or clo.SegArg(op, tie, form, ctx, vt, ct)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0)
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if n else None
    i_r = Region(rdev, m_h * 4, offs[2], None, 2) if m_h else None
    o_r = Region(rdev, m_h * vs, offs[3], None, 0) if m_h and with_val else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert sa.with_device_data(q, s_r.view, view(n_r), view(v_r), view(i_r), view(o_r), num_r.view, m_h, n), what
        q.finish()
        got = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        if compare:
            assert got == total, "%s: num_out = %d, the model's total is %d" % (what, got, total)
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            if i_r:
                now = i_r.base.read(q, np.uint8, i_r.host.size)[i_r.at:i_r.at + idx.nbytes].copy().view(np.uint32)
                bad = np.flatnonzero(now != idx)
                assert bad.size == 0, "%s: idx_out of %d of %d segments differs, first %d: %d, the model has %d" % (
                    what, bad.size, idx.size, bad[0], now[bad[0]], idx[bad[0]])
                i_r.check(idx, what + ": idx_out")                          # ... and nothing behind the m rows written
            if o_r:
                now = bits_of(o_r.base.read(q, np.uint8, o_r.host.size)[o_r.at:o_r.at + val.nbytes].copy().view(val.dtype))
                bad = np.flatnonzero(now != bits_of(val))
                assert bad.size == 0, "%s: val_out of %d of %d segments differs, first %d: %x, the model has %x" % (
                    what, bad.size, val.size, bad[0], now[bad[0]], bits_of(val)[bad[0]])
                o_r.check(val, what + ": val_out")
        else:                                                              # in bounds: the guards
            for r, size in ((i_r, 4), (o_r, vs)):
                if r:
                    now = r.base.read(q, np.uint8, r.host.size)
                    r.check(now[r.at:r.at + m_h * size], what)
        s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return got, idx, val
    finally:
        for r in (s_r, n_r, v_r, i_r, o_r, num_r):
            if r:
                r.close()
        if obj is None:
            sa.close()


def rotate(case):
    """An op, a tie, a form, a count type and a value type for case number `case`: every one of them meets every pattern."""
    return OPS[case % 2], TIES[case // 2 % 2], FORMS[case // 4 % 2], ("uint", "ulong")[case // 8 % 2], TYPES[case % len(TYPES)]


def test_merge_lengths_around_the_tile_edges_and_count_patterns(dev, T):
    """m + n, the number of merge steps, at T - 1, T, T + 1, 2 T - 1, 2 T + 1 and 3 T + 5 x the count patterns; the
    offsets rebased."""
    case = 0
    for steps in (T - 1, T, T + 1, 2 * T - 1, 2 * T + 1, 3 * T + 5):
        for pattern in PATTERNS:
            # the pattern with `steps` rows, cut to the first segments whose rows and ends together take `steps` steps
            c = counts_of(pattern, steps, T, case)
            keep = int(np.searchsorted(np.cumsum(c + 1), steps, "left")) + 1
            c = c[:keep].copy()
            over = int((c + 1).sum()) - steps
            if over > 0:
                c[-1] -= min(over, int(c[-1]))
            while int((c + 1).sum()) > steps:                               # (only empty segments were left to cut)
                c = c[:-1]
            if int((c + 1).sum()) < steps:
                c[-1] += steps - int((c + 1).sum())
            n = int(c.sum())
            assert c.size + n == steps and (c >= 0).all(), (pattern, steps)
            op, tie, form, ct, vt = rotate(case)
            case += 1
            got, _, _ = run_arg(dev, op, tie, form, ct, vt, c, n, "%s, %d steps" % (pattern, steps), base=case * 1000, seed=case)
            assert got == n


@pytest.mark.parametrize("vt", ["uint", "double"])
def test_every_op_tie_form_and_count_type(dev, T, vt):
    counts = counts_of("geometric", 2 * T + 3, T, 5)
    counts[::7] = 0
    case = 0
    for op in OPS:
        for tie in TIES:
            for form in FORMS:
                for ct in ("uint", "ulong"):
                    case += 1
                    _, idx, _ = run_arg(dev, op, tie, form, ct, vt, counts, 2 * T + 3, "every combination", base=3 * case, seed=case)
                    assert (idx[::7] == NONE).all()


def test_ties_where_they_are_decided(dev, T):
    """All values equal in one segment of 3 T + 1 rows: `first` gives its first row and `last` its last. And the same
    extremum placed exactly twice in one segment (row i is merge step i), the two straddling a lane's edge (T / 256 steps
    per lane), a wave's edge, a tile's edge, and two tiles with a whole tile between them."""
    n = 3 * T + 1
    lane, wave = T // 256, T // 4
    for k, vt in enumerate(("uint", "float", "long")):
        dt = np.dtype(NP[vt])
        for op in OPS:
            for tie in TIES:
                equal = np.full(n, 7, dt)
                _, idx, _ = run_arg(dev, op, tie, FORMS[k % 2], "uint", vt, [n], n, "all equal", vals=equal)
                assert idx[0] == (0 if tie == "first" else n - 1)
                _, idx, _ = run_arg(dev, op, tie, "counts", "ulong", vt, [3, n - 3 - 5, 5], n, "all equal, between others", vals=equal)
                assert idx.tolist() == ([0, 3, n - 5] if tie == "first" else [2, n - 6, n - 1])
                for a, b in ((lane - 1, lane), (wave - 1, wave), (T - 1, T), (T - 1, 2 * T + 1), (5 * lane - 1, 5 * lane), (2 * T - 1, 2 * T)):
                    v = np.full(n, 50, dt)
                    v[[a, b]] = 10 if op == "argmin" else 90
                    _, idx, val = run_arg(dev, op, tie, "counts", "uint", vt, [n], n, "the extremum at rows %d and %d" % (a, b), vals=v)
                    assert idx[0] == (a if tie == "first" else b) and val[0] == v[a]


def test_the_extremum_in_the_carried_part_and_in_the_closing_tile(dev, T):
    """A segment of 2 T + 100 rows behind 50 short ones: it closes in the third tile. Its extremum lies in the first tile
    (it reaches the output through the carry scan and the fix-up alone), or in the tile that closes it."""
    counts = np.concatenate((np.full(50, 3), [2 * T + 100], np.full(40, 2)))
    n = int(counts.sum())
    start = 150
    for vt in ("int", "double"):
        for op in OPS:
            for tie, at in (("first", start + 5), ("last", start + T // 2), ("first", start + 2 * T + 90), ("last", start + 2 * T + 99),
                            ("last", start + T + 7)):
                v = values_for(vt, n, 3)
                v[start:start + 2 * T + 100] = 0                            # ties everywhere else in the long segment
                v[at] = -3 if op == "argmin" else 3
                _, idx, val = run_arg(dev, op, tie, "offsets", "uint", vt, counts, n, "the extremum at row %d" % at, vals=v, base=77)
                assert idx[50] == at and val[50] == v[at]


def test_empty_segments(dev, T):
    case = 0
    for m in (1, 5, T, 2 * T + 1):                                        # nothing but empty segments, without and with rows nobody owns
        for n in (0, 7, T + 3):
            op, tie, form, ct, vt = rotate(case)
            case += 1
            got, idx, val = run_arg(dev, op, tie, form, ct, vt, np.zeros(m, np.int64), n, "%d empty segments" % m, seed=case)
            assert got == 0 and (idx == NONE).all() and (bits_of(val) == bits_of(np.array([none_value(op, vt)]))[0]).all()
    # a tile that only closes segments: T + 5 empty segments between rows
    counts = np.concatenate((np.full(9, T // 4 + 1), np.zeros(T + 5, np.int64), np.full(9, T // 4 + 1)))
    for case, (form, ct) in enumerate((("counts", "ulong"), ("offsets", "uint"))):
        for op in OPS:
            run_arg(dev, op, TIES[case], form, ct, ("int", "float")[case], counts, int(counts.sum()), "T + 5 empty segments between rows", seed=3)


def test_a_million_empty_segments_take_bounded_work(dev, T):
    counts = np.concatenate((np.full(5, 700), np.zeros(1 << 20, np.int64), np.full(5, 900), np.zeros(3, np.int64)))
    for op, tie, form, vt in (("argmin", "first", "counts", "uint"), ("argmax", "last", "offsets", "double")):
        got, idx, _ = run_arg(dev, op, tie, form, "uint", vt, counts, 8000, "2^20 empty segments", seed=4)
        assert got == 8000 and (idx[5:5 + (1 << 20)] == NONE).all() and (idx[:5] != NONE).all()


def test_rows_that_hold_the_identity_value(dev, T):
    """The value an empty segment reports, as a row: in a segment of one row and as all rows of a segment, row 0 under
    `last` (whose packed aggregate is the all-ones word) and the last row under `first` included. An empty segment lies
    between them."""
    counts = np.array([1, 0, 4, 1, 0, 2 * T + 3, 0, 1], np.int64)
    n = int(counts.sum())
    for vt in TYPES:
        for op in OPS:
            ident = none_value(op, vt)
            other = none_value(OPS[1 - OPS.index(op)], vt)
            for tie in TIES:
                v = np.full(n, ident, NP[vt])
                _, idx, val = run_arg(dev, op, tie, "counts", "uint", vt, counts, n, "identity rows", vals=v)
                first = [0, NONE, 1, 5, NONE, 6, NONE, n - 1]
                last = [0, NONE, 4, 5, NONE, n - 2, NONE, n - 1]
                assert idx.tolist() == (first if tie == "first" else last)
                v = np.full(n, other, NP[vt])                                # ... and among better rows it loses
                v[[0, 3, n - 1]] = ident
                _, idx, _ = run_arg(dev, op, tie, "offsets", "ulong", vt, counts, n, "identity rows among others", vals=v, base=5)
                assert idx.tolist() == [0, NONE, 1 if tie == "first" else 4, 5, NONE, 6 if tie == "first" else n - 2, NONE, n - 1]


def test_every_value_type_at_its_extremes(dev, T):
    counts = counts_of("geometric", 2 * T + 9, T, 12)
    counts[::5] = 0
    n = int(counts.sum())
    for k, vt in enumerate(TYPES):
        for op in OPS:
            for tie in TIES:
                run_arg(dev, op, tie, FORMS[k % 2], ("uint", "ulong")[k % 2], vt, counts, n, "extremes", seed=k, base=k)
    for vt in ("float", "double"):                                       # -0.0 against +0.0 in either order; the infinities; NaNs by sign and payload
        dt = np.dtype(NP[vt])
        ut = np.dtype("u%d" % dt.itemsize)
        inf, sign = np.array([np.inf], dt).view(ut)[0], ut.type(1 << (8 * dt.itemsize - 1))
        rows = np.array([0, sign, sign, 0, inf, inf | sign, 5, inf + 1, inf + 2, (inf + 1) | sign, (inf + 2) | sign, 5], ut).view(dt)
        counts = [2, 2, 2, 2, 2, 2]
        for op, tie, want in (("argmin", "first", [1, 2, 5, 6, 9, 10]), ("argmin", "last", [1, 2, 5, 6, 9, 10]),
                              ("argmax", "first", [0, 3, 4, 7, 8, 11]), ("argmax", "last", [0, 3, 4, 7, 8, 11])):
            _, idx, val = run_arg(dev, op, tie, "counts", "uint", vt, counts, 12, "zeros, infinities and NaNs", vals=rows)
            assert idx.tolist() == want and (bits_of(val) == bits_of(rows)[want]).all()


def test_totals_above_the_rows_and_num_in(dev, T):
    """num_out always receives the unclamped total; a segment cut by n reports from the rows it has, the segments beyond
    report NONE. num_in below, at and above numel_seg."""
    case = 0
    for total in (T + 1, 3 * T + 11):
        for pattern in ("sevens", "geometric", "long between ones"):
            counts = counts_of(pattern, total, T, 7)
            for n in (0, 1, total // 2, total - 3, total - 1):
                op, tie, form, ct, vt = rotate(case)
                case += 1
                got, idx, _ = run_arg(dev, op, tie, form, ct, vt, counts, n, "%s, total %d" % (pattern, total), seed=case)
                starts = np.concatenate(([0], np.cumsum(counts)[:-1]))
                assert got == total and (idx[starts >= n] == NONE).all() and (idx[(starts < n) & (counts > 0)] != NONE).all()
    counts = counts_of("geometric", 3 * T + 9, T, 6)
    counts[::6] = 0
    m_h = counts.size
    for i, num_in in enumerate((0, 1, m_h // 2, m_h - 1, m_h, m_h + 1, 1 << 40)):
        for form in FORMS:
            op, tie, _, ct, vt = rotate(i)
            got, idx, _ = run_arg(dev, op, tie, form, ct, vt, counts, 3 * T + 9, "num_in %d of %d" % (num_in, m_h), num_in=num_in, base=5 * i, seed=i)
            assert got == int(counts[:min(num_in, m_h)].sum()) and idx.size == min(num_in, m_h)


def test_against_segreduce_and_segsort(dev, T):
    """For the four integer types val_out is CloSegReduce's min or max of the same call, and idx_out is the first row
    (argmin, first) or the last row (argmax, last) of every segment of CloSegSort's stable argsort."""
    clo, ctx, q = dev
    counts = counts_of("geometric", 3 * T + 50, T, 21)
    counts[::9] = 0
    m, n = counts.size, int(counts.sum())
    ends = np.cumsum(counts)
    full = counts > 0
    for vt in ("int", "uint", "long", "ulong"):
        vals = values_for(vt, n, 21)
        vs = vals.dtype.itemsize
        for op, tie, red in (("argmin", "first", "min"), ("argmax", "last", "max")):
            c_r, v_r = Region(dev, 4 * m, 0, counts.astype(np.uint32), 0), Region(dev, vals.nbytes, 0, vals, 1)
            i_r, o_r, a_r, p_r = Region(dev, 4 * m, 0, None, 2), Region(dev, vs * m, 0, None, 0), Region(dev, vs * m, 0, None, 1), Region(dev, 4 * n, 0, None, 2)
            nums = [Region(dev, 8, 0, None, k) for k in range(3)]
            sa, sr, ss = clo.SegArg(op, tie, "counts", ctx, vt, "uint"), clo.SegReduce(red, "counts", ctx, vt, vt, "uint"), clo.SegSort("counts", ctx, vt, 4, "uint")
            try:
                assert sa.with_device_data(q, c_r.view, None, v_r.view, i_r.view, o_r.view, nums[0].view, m, n)
                assert sr.with_device_data(q, c_r.view, None, v_r.view, a_r.view, nums[1].view, m, n)
                assert ss.with_device_data(q, c_r.view, None, v_r.view, None, None, p_r.view, nums[2].view, m, n)
                q.finish()
                aggr = a_r.base.read(q, np.uint8, a_r.host.size)[a_r.at:a_r.at + vs * m].copy().view(NP[vt])
                o_r.check(aggr, "%s %s: val_out against CloSegReduce" % (op, vt))
                perm = p_r.base.read(q, np.uint8, p_r.host.size)[p_r.at:p_r.at + 4 * n].copy().view(np.uint32)
                want = np.full(m, NONE, np.uint32)
                want[full] = perm[(ends - counts)[full]] if tie == "first" else perm[ends[full] - 1]
                i_r.check(want, "%s %s: idx_out against CloSegSort's argsort" % (op, vt))
                i_r.check(segarg(op, tie, "counts", counts, vals)[0], "the model")
            finally:
                for x in [c_r, v_r, i_r, o_r, a_r, p_r, sa, sr, ss] + nums:
                    x.close()


def test_without_val_out(dev, T):
    """val_out NULL: idx_out is the same, and nothing else is written (the canaries around every array, and the object's
    workspace is the size the getter gives: a smaller one is refused in test_thin_abi_status_codes)."""
    counts = counts_of("geometric", 3 * T + 17, T, 31)
    counts[::4] = 0
    n = int(counts.sum())
    for k, vt in enumerate(TYPES):
        op, tie = OPS[k % 2], TIES[k // 2 % 2]
        _, a, _ = run_arg(dev, op, tie, FORMS[k % 2], "uint", vt, counts, n, "with val_out", seed=k)
        _, b, _ = run_arg(dev, op, tie, FORMS[k % 2], "uint", vt, counts, n, "without val_out", seed=k, with_val=False)
        assert np.array_equal(a, b)


def test_element_aligned_views(dev, T):
    """Every array one (or three) elements past a 16-byte boundary: nothing may assume more than the element's
    alignment."""
    counts = counts_of("geometric", 2 * T + 37, T, 9)
    counts[5:9] = 0
    n = 2 * T + 37
    cases = (("counts", "uint", "int", (4, 4, 4, 4)), ("offsets", "uint", "float", (12, 12, 8, 12)), ("counts", "ulong", "long", (8, 8, 4, 8)),
             ("offsets", "ulong", "double", (8, 8, 12, 8)), ("counts", "uint", "uint", (12, 8, 12, 4)), ("offsets", "uint", "ulong", (4, 8, 4, 8)))
    for i, (form, ct, vt, offs) in enumerate(cases):
        run_arg(dev, OPS[i % 2], TIES[i // 2 % 2], form, ct, vt, counts, n, "views at %s" % (offs,), offs=offs, base=9, seed=i)


def test_two_objects_on_two_queues_and_one_object_moved(dev, T):
    clo, ctx, _ = dev
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("argmin", "last", "counts", "uint", "uint"), ("argmax", "first", "offsets", "ulong", "double"))
    objs = [clo.SegArg(op, tie, form, ctx, vt, ct) for op, tie, form, ct, vt in specs]
    try:
        for rnd in range(2):
            sent = []
            for i, (op, tie, form, ct, vt) in enumerate(specs):
                counts = counts_of("geometric", 40 * T + 9 + rnd, T, 10 * rnd + i)
                counts[::9] = 0
                n = int(counts.sum())
                src, vals = source(form, ct, counts, 7), values_for(vt, n, rnd)
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, src.nbytes, 0, src, 0), Region(rdev, vals.nbytes, 0, vals, 1), Region(rdev, counts.size * 4, 0, None, 2),
                        Region(rdev, counts.size * vals.dtype.itemsize, 0, None, 0), Region(rdev, 8, 0, None, 0)]
                sent.append((src, vals, counts.size, n, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (src, vals, m_h, n, regs) in enumerate(sent):
                assert objs[i].with_device_data(qs[i], regs[0].view, None, regs[1].view, regs[2].view, regs[3].view, regs[4].view, m_h, n)
            for i in range(2):
                qs[i].finish()
            for i, (src, vals, m_h, n, regs) in enumerate(sent):
                idx, val, t = segarg(specs[i][0], specs[i][1], specs[i][2], src, vals)
                what = "round %d, %s" % (rnd, specs[i][2])
                regs[4].check(np.array([t], np.uint64), what + ": num_out")
                regs[2].check(idx, what + ": idx_out")
                regs[3].check(val, what + ": val_out")
                for r in regs:
                    r.close()
        for j, qi in enumerate((0, 1, 0, 1)):
            total = (5, 60, 2, 30)[j] * T + j                               # small, large, small, large
            counts = counts_of("geometric", total, T, 40 + j)
            run_arg((clo, ctx, qs[qi]), "argmin", "last", "counts", "uint", "uint", counts, total, "moved, call %d" % j, obj=objs[0], q=qs[qi], seed=j)
    finally:
        for x in objs + qs:
            x.close()


def test_host_data_form(dev, T):
    clo, ctx, q = dev
    counts = counts_of("geometric", 2 * T + 9, T, 11)
    counts[::5] = 0
    total, qc = int(counts.sum()), clo.Queue(ctx)
    try:
        for form in FORMS:
            for op, tie, ct, vt in (("argmin", "first", "uint", "float"), ("argmax", "last", "ulong", "uint"), ("argmin", "last", "uint", "long")):
                src = source(form, ct, counts, 4321)
                sa = clo.SegArg(op, tie, form, ctx, vt, ct)
                for n in (0, total - 5, total, total + 7):
                    vals = values_for(vt, n, n)
                    for num_in, qe, qcomm, wv in ((None, q, qc, True), (counts.size // 2, None, None, False), (counts.size + 9, q, None, True)):
                        idx, val, t = segarg(op, tie, form, src, vals, num_in)
                        i, v, got = sa.with_host_data(src, vals, num_in=num_in, want_values=wv, q_exec=qe, q_comm=qcomm)
                        what = (form, op, tie, ct, vt, n, num_in)
                        assert got == t and i.dtype == np.uint32 and np.array_equal(i, idx), what
                        assert (v is None) if not wv else (v.dtype == val.dtype and np.array_equal(bits_of(v), bits_of(val))), what
                sa.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev, T):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    INT, UINT, LONG, DOUBLE = (clo.CLO_TYPES[t] for t in ("int", "uint", "long", "double"))
    m_h, n = 1000, 3 * T
    need = lib.clo_hip_segarg_workspace_bytes(m_h, n)
    assert need > 0 and need % 256 == 0
    counts = np.random.default_rng(5).integers(0, 9, 2 * m_h + 4, dtype=np.uint32)
    vals = values_for("uint", 2 * n + 4, 5)
    cn, vi, ni = Region(dev, counts.nbytes, 0, counts, 0), Region(dev, vals.nbytes, 0, vals, 1), Region(dev, 16, 0, np.array([m_h // 2, 0], np.uint64), 2)
    io, vo, num = Region(dev, 4 * m_h + 16, 0, None, 0), Region(dev, 8 * m_h + 16, 0, None, 2), Region(dev, 16, 0, None, 1)
    ws = Region(dev, need + 512, 0, None, 1)                                # the workspace between canaries: at a multiple of 256
    assert ws.ptr % 256 == 0
    s = q.stream

    def call(c_p, v_p, i_p, o_p, op=0, tie=0, form=0, cs=4, n_p=None, num_p=num.ptr, numel_seg=m_h, numel=n, vt=UINT, w=ws.ptr, wb=need):
        return lib.clo_hip_segarg(op, tie, form, c_p, cs, n_p, v_p, i_p, o_p, num_p, numel_seg, numel, vt, w, wb, s)

    try:
        full = (cn.ptr, vi.ptr, io.ptr, vo.ptr)
        for bad in (-1, 2, 100):
            assert call(*full, op=bad) == EARGS and call(*full, tie=bad) == EARGS and call(*full, form=bad) == EARGS
        for cs in (0, 1, 2, 3, 16):
            assert call(*full, cs=cs) == EUNSUPPORTED, cs
        for vt in ("char", "uchar", "short", "ushort", "half"):
            assert call(*full, vt=clo.CLO_TYPES[vt]) == EUNSUPPORTED, vt
        assert call(*full, vt=-1) == EUNSUPPORTED and call(*full, vt=11) == EUNSUPPORTED
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(*full, n_p=ni.ptr + 4) == EARGS                                                     # num_in misaligned
        assert call(*full, numel_seg=1 << 32) == EARGS and call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, io.ptr, vo.ptr) == EARGS and call(None, None, None, None, form=1, numel_seg=0, numel=0) == EARGS
        assert call(cn.ptr, None, io.ptr, vo.ptr) == EARGS and call(cn.ptr, vi.ptr, None, vo.ptr) == EARGS   # values_in, idx_out missing
        for i in range(4):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        for i, kw in ((0, dict(cs=8)), (1, dict(vt=LONG)), (3, dict(vt=DOUBLE))):                       # 4-aligned is not 8-aligned
            args = list(full)
            args[i] += 4
            assert call(*args, **kw) == EARGS, i
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: off by 64, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # one byte short
        q.finish()
        for r in (io, vo, num, ws):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size, which is not overrun, with val_out and without;
        # num_in; views at an odd element; numel_seg 0 needs no workspace, no input
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        rows = lambda r, dt, k: r.base.read(q, np.uint8, r.host.size)[r.at:r.at + k * np.dtype(dt).itemsize].copy().view(dt)
        guards = lambda: ws.check(ws.base.read(q, np.uint8, ws.host.size)[ws.at:ws.at + need], "the workspace's guards")
        assert call(*full) == 0
        q.finish()
        idx, val, t = segarg("argmin", "first", "counts", counts[:m_h], vals[:n])
        assert first() == t and np.array_equal(rows(io, np.uint32, m_h), idx) and np.array_equal(rows(vo, np.uint32, m_h), val)
        guards()
        assert call(cn.ptr, vi.ptr, io.ptr, None, op=1, tie=1, n_p=ni.ptr) == 0
        q.finish()
        idx, _, t = segarg("argmax", "last", "counts", counts[:m_h], vals[:n], m_h // 2)
        assert first() == t and np.array_equal(rows(io, np.uint32, m_h // 2), idx)
        guards()
        assert call(cn.ptr + 4, vi.ptr + 4, io.ptr + 4, vo.ptr + 4, op=1, vt=INT) == 0
        q.finish()
        idx, val, t = segarg("argmax", "first", "counts", counts[1:m_h + 1], vals[1:n + 1].view(np.int32))
        assert first() == t and np.array_equal(rows(io, np.uint32, m_h + 1)[1:], idx) and np.array_equal(rows(vo, np.int32, m_h + 1)[1:], val)
        assert call(None, vi.ptr, None, None, numel_seg=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        for r in (cn, vi, ni, io, vo, num, ws):
            r.close()


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, T, form):
    """clo_hip_segarg captured from one client stream (a linear graph) after one eager warm-up and replayed three times,
    the counts, num_in and the values rewritten and the outputs refilled with a canary before each replay (the protocol
    of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the rows."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, n = 900, 4 * T + 3
    need = lib.clo_hip_segarg_workspace_bytes(m_h, n)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, 4 * n, 4 * m_h, 4 * m_h, 8, need)]
    src_m, nin_m, vi, io, vo, num, ws = made
    means = [16, 3, 40, 9, 16]                                              # 900 segments of mean 40: above the rows
    totals = set()
    FLOAT = clo.CLO_TYPES["float"]

    def load(r):
        counts = np.random.default_rng(300 + r).geometric(1 / means[r], m_h) - (np.arange(m_h) % 4 == r % 4)
        src, num_in, vals = source(form, "uint", counts, 50 * r), m_h - 100 * (r % 3), values_for("float", n, r)
        for m in (io, vo, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (vi, vals)):
            mem_.put(arr)
        want = segarg("argmax", "last", form, src, vals, num_in)
        totals.add(want[2])
        return want, vals

    def enqueue():
        return lib.clo_hip_segarg(1, 1, FORMS.index(form), src_m.ptr, 4, nin_m.ptr, vi.ptr, io.ptr, vo.ptr, num.ptr, m_h, n, FLOAT, ws.ptr, need, q.stream)

    def verify(r, want):
        (idx, val, total), vals = want
        tag = "%s round %d" % (form, r)
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        GC.same(io.get(np.uint32, m_h), np.concatenate((idx, GC.canary(np.uint32, m_h - idx.size))), tag + ": idx_out")
        GC.same(vo.get(np.float32, m_h), np.concatenate((val, GC.canary(np.float32, m_h - val.size))), tag + ": val_out")
        GC.same(vi.get(np.float32, n), vals, "values_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(totals) >= 4 and max(totals) > n > min(totals), totals
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def test_chain_behind_bucket_offsets(dev, T):
    """CloBucket partitions rows by bin and writes the bins' CSR offsets; CloSegArg in the offsets form then finds, in
    every bin, the row with the smallest value — on one queue, with no host wait in between."""
    clo, ctx, q = dev
    from bucket_model import bucket
    n, num_bins = 5 * T + 5, 300
    rng = np.random.default_rng(41)
    keys = rng.integers(0, num_bins + 40, n).astype(np.uint32)              # some rows fall outside every bin
    keys[keys % 7 == 3] += 1                                                # ... and some bins stay empty
    vals = rng.integers(0, 50, n, dtype=np.uint32)
    k_r, v_r = Region(dev, 4 * n, 0, keys, 0), Region(dev, 4 * n, 0, vals, 1)
    ko_r, vo_r, of_r = Region(dev, 4 * n, 0, None, 2), Region(dev, 4 * n, 0, None, 2), Region(dev, 4 * (num_bins + 1), 0, None, 1)
    i_r, o_r, num_r = Region(dev, 4 * num_bins, 0, None, 0), Region(dev, 4 * num_bins, 0, None, 1), Region(dev, 8, 0, None, 2)
    bk, sa = clo.Bucket(ctx, "uint", 4, "uint"), clo.SegArg("argmin", "last", "offsets", ctx, "uint", "uint")
    try:
        assert bk.with_device_data(q, k_r.view, v_r.view, ko_r.view, vo_r.view, of_r.view, n, 0, 0, num_bins)
        assert sa.with_device_data(q, of_r.view, None, vo_r.view, i_r.view, o_r.view, num_r.view, num_bins, n)
        q.finish()
        _, wv, _, woff = bucket(keys, vals, 0, 0, num_bins, "uint")
        of_r.check(woff, "offsets_out")
        idx, val, total = segarg("argmin", "last", "offsets", woff, wv)
        assert 0 < total < n and (idx == NONE).any()
        num_r.check(np.array([total], np.uint64), "num_out")
        i_r.check(idx, "idx_out behind the bucket's offsets")
        o_r.check(val, "val_out behind the bucket's offsets")
    finally:
        for x in (k_r, v_r, ko_r, vo_r, of_r, i_r, o_r, num_r, bk, sa):
            x.close()


def test_broken_preconditions_stay_in_bounds(dev, T):
    """Offsets that descend or are unordered, counts whose sums wrap 2^64, a num_in above numel_seg: the call completes,
    the canaries and the inputs are intact. Contents are not compared: DESIGN.md section 25 gives the argument that this
    holds by construction, and this run shows it once."""
    rng = np.random.default_rng(90)
    m_h, n = 3 * T + 700, 3 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 2).astype(np.uint32)
    unordered = rng.integers(0, 2 * n, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for i, (form, ct, src) in enumerate((("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping))):
        for op, tie, vt in (("argmin", "first", "uint"), ("argmax", "last", "double")):
            run_arg(dev, op, tie, form, ct, vt, None, n, "broken preconditions", num_in=m_h + 1000, src=src, compare=False, seed=i)


@pytest.mark.parametrize("tie", TIES)
def test_equal_values_carried_through_a_whole_trip_of_the_carry_scan(dev, T, tie):
    """The one work-group of the carry scan takes segarg_carry_tiles tiles' states per trip. One segment of equal values
    of two trips' rows, behind T / 2 - 10 segments of one row and before 100 more: it begins in the first tile, passes through
    the whole second one, in which no segment closes, and closes in the third. Against the closed form."""
    clo = dev[0]
    trip = clo.segarg_carry_tiles()
    long = 2 * trip * T
    before, after = T // 2 - 10, 100
    counts = np.concatenate((np.ones(before, np.int64), [long], np.ones(after, np.int64)))
    n = int(counts.sum())
    assert 2 * before < T and 2 * before + long >= 2 * trip * T             # begins in the first tile, closes (at that step) in the third trip
    vals = np.full(n, 7, np.uint32)
    idx = np.arange(n, dtype=np.uint32)[np.concatenate((np.arange(before), [before if tie == "first" else before + long - 1], before + long + np.arange(after)))]
    for op in OPS:
        run_arg(dev, op, tie, "counts", "uint", "uint", counts, n, "two trips of equal values", vals=vals, want=(idx, np.full(idx.size, 7, np.uint32), n))


def test_indices_above_2p31(dev, T):
    """n = 2^31 + 2^20 + 5 uint values, made on the device in chunks: value i is 100 + (i & 0xff), except for 2000 rows
    of 50 laid across row 2^31 and two planted rows. Four segments: [0, 2^30), [2^30, 2^31 - 1000), the equal rows
    [2^31 - 1000, 2^31 + 1000) and the rest, whose unique minimum 3 lies at row n - 7 and whose unique maximum at row
    2^31 + 2^19. The expectation is closed-form."""
    import torch
    from test_gpu_above_2p31 import N, as_buffer, chunks
    clo, ctx, q = dev
    if torch.cuda.get_device_properties(0).total_memory < (96 << 30):
        pytest.skip("needs ~60 GiB of device memory")
    P = 1 << 31
    ends = [1 << 30, P - 1000, P + 1000, N]
    counts = torch.tensor(np.diff([0] + ends), dtype=torch.int64, device="cuda")
    vals = torch.empty(N, dtype=torch.int32, device="cuda")
    for lo, hi in chunks(N):
        vals[lo:hi] = (100 + (torch.arange(lo, hi, dtype=torch.int64, device="cuda") & 0xff)).to(torch.int32)
    vals[P - 1000:P + 1000] = 50
    vals[N - 7] = 3
    vals[P + (1 << 19)] = 0x7ffffff0
    io = torch.full((4 + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")                          # bytes A5 A5 A5 A5
    vo = torch.full((4 + 64,), -0x5A5A5A5B, dtype=torch.int32, device="cuda")
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    bufs = [as_buffer(clo, ctx, t) for t in (counts, vals, io, vo, cnt)]
    cases = (("argmin", "last", [(1 << 30) - 256, P - 1024, P + 999, N - 7], [100, 100, 50, 3]),
             ("argmax", "first", [255, (1 << 30) + 255, P - 1000, P + (1 << 19)], [355, 355, 50, 0x7ffffff0]),
             ("argmin", "first", [0, 1 << 30, P - 1000, N - 7], [100, 100, 50, 3]))
    try:
        for op, tie, want_i, want_v in cases:
            sa = clo.SegArg(op, tie, "counts", ctx, "uint", "ulong")
            try:
                assert sa.with_device_data(q, bufs[0], None, bufs[1], bufs[2], bufs[3], bufs[4], 4, N)
                q.finish()
            finally:
                sa.close()
            assert int(cnt[0]) == N
            assert (io[:4].to(torch.int64) & 0xffffffff).tolist() == want_i, (op, tie)
            assert vo[:4].tolist() == want_v, (op, tie)
            assert bool((io[4:] == -0x5A5A5A5B).all()) and bool((vo[4:] == -0x5A5A5A5B).all()), "rows >= m were written"
        # the inputs are what they were: checked in chunks on the device
        for lo, hi in chunks(N):
            want = (100 + (torch.arange(lo, hi, dtype=torch.int64, device="cuda") & 0xff)).to(torch.int32)
            for at, v in ((N - 7, 3), (P + (1 << 19), 0x7ffffff0)):
                if lo <= at < hi:
                    want[at - lo] = v
            a, b = max(lo, P - 1000), min(hi, P + 1000)
            if a < b:
                want[a - lo:b - lo] = 50
            assert bool((vals[lo:hi] == want).all()), "values_in changed in rows [%d, %d)" % (lo, hi)
    finally:
        for x in bufs:
            x.close()
        del counts, vals, io, vo
        torch.cuda.empty_cache()
