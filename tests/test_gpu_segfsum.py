"""CloSegFSum (include/clo_segfsum.h) on the GPU against the numpy model of its addition order (tests/segfsum_model.py),
bit for bit (fscan_model.same_bits: a NaN equals any NaN at its position). Every array is a view inside a larger
allocation with 256 guard bytes of a canary pattern on each side (the Region of test_gpu_histogram.py); sums_out and
num_out are pre-filled with the pattern, and after every call num_out is the model's unclamped total, the m rows written
equal the model's bits, and the guards, every input and every row at index >= m are unchanged. With T = 4352 merge steps
per tile: the row counts at which a lane (17), a wave (1088) and a tile end x ten layouts of segments; both forms x both
count types x the four pairs; rebased offsets; half values with subnormals and 65504; zeros of both signs, infinities and
NaNs; telescoping inputs (any order gives the same bits: a lost or doubled row shows) and rounding inputs (the order
shows in the low bits); a segment across two threads, two waves and the trips of the carry scan; the same bits from a
second call, from views at odd elements, from the other form and count type, from two queues, a moved object and the
host form; the thin ABI's status codes; a captured linear graph replayed on other counts and values; broken
preconditions (in bounds, contents not compared); cross-checks against CloExpand and CloSegReduce."""
import math

import numpy as np
import pytest

import segfsum_model as M
from segfsum_model import FORMS, NP, PAIRS, same_bits, segfsum
from test_gpu_histogram import Region

pytestmark = pytest.mark.gpu

CDT = {"uint": np.uint32, "ulong": np.uint64}
CTS = ("uint", "ulong")


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def T(dev):
    clo = dev[0]
    assert all(clo.segfsum_tile(np.dtype(NP[v]).itemsize, np.dtype(NP[s]).itemsize) == M.TILE for v, s in PAIRS)
    return M.TILE


def bits_of(a):
    a = np.ascontiguousarray(a)
    return a.view("u%d" % a.dtype.itemsize)


def run_fsum(dev, form, ct, vt, st, counts, vals, what, num_in=None, base=0, offs=(0, 0, 0), obj=None, q=None, src=None, compare=True, want=None):
    """One call on views at byte offsets offs = (counts_or_offsets, values_in, sums_out); checks everything and returns
    (total, the m sums as the GPU wrote them). src: the input as it is (broken preconditions); compare False: the rows'
    contents are not compared; want: (sums, total) instead of the model's."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    if src is None:
        src = M.source(form, np.asarray(counts, np.uint64), CDT[ct], base)
    m_h = src.size - (1 if form == "offsets" else 0)
    n = vals.size
    assert vals.dtype == NP[vt]
    sdt = np.dtype(NP[st])
    sums, total = (want or segfsum(form, src, vals, st, num_in)) if compare else (None, None)
    what = "%s %s %s -> %s n %d, %s" % (form, ct, vt, st, n, what)
    sf = obj or clo.SegFSum(form, ctx, vt, st, ct)
    s_r = Region(rdev, src.nbytes, offs[0], src, 0)
    n_r = Region(rdev, 8, 0, np.array([num_in], np.uint64), 1) if num_in is not None else None
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if n else None
    o_r = Region(rdev, m_h * sdt.itemsize, offs[2], None, 2) if m_h else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert sf.with_device_data(q, s_r.view, view(n_r), view(v_r), view(o_r), num_r.view, m_h, n), what
        q.finish()
        got = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        m = m_h if num_in is None else min(m_h, num_in)
        now = np.zeros(0, sdt)
        if o_r:
            now = o_r.base.read(q, np.uint8, o_r.host.size)[o_r.at:o_r.at + m * sdt.itemsize].copy().view(sdt)
            o_r.check(now, what + ": sums_out")                              # the guards, and nothing behind the m rows written
        if compare:
            assert got == total, "%s: num_out = %d, the model's total is %d" % (what, got, total)
            num_r.check(np.array([total], np.uint64), what + ": num_out")
            assert sums.size == m
            if not same_bits(now, sums):
                bad = np.flatnonzero((bits_of(now) != bits_of(sums)) & ~(np.isnan(now) & np.isnan(sums)))
                raise AssertionError("%s: sums_out of %d of %d segments differs, first %d: %r (%x), the model has %r (%x)" % (
                    what, bad.size, m, bad[0], now[bad[0]], bits_of(now)[bad[0]], sums[bad[0]], bits_of(sums)[bad[0]]))
        s_r.check(src, what + ": counts_or_offsets")
        if n_r:
            n_r.check(np.array([num_in], np.uint64), what + ": num_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        return got, now
    finally:
        for r in (s_r, n_r, v_r, o_r, num_r):
            if r:
                r.close()
        if obj is None:
            sf.close()


def rotate(case):
    """A form, a count type and a pair for case number `case`: every one of them meets every layout."""
    return (FORMS[case % 2], CTS[case // 2 % 2]) + PAIRS[case % len(PAIRS)]


@pytest.mark.parametrize("name", M.LAYOUTS)
def test_row_counts_and_layouts(dev, T, name):
    """0, 1, 16, 17, 18 rows (a lane's 17 steps), 1087, 1088, 1089 (a wave's), T - 1, T, T + 1 and 2 T + 5 x the layouts:
    one segment; length 1 throughout; length 17; geometric with mean 16; every second segment empty; 4 T + 5 empty
    segments between the rows; one segment across three tiles; an end on the last and on the first step of every tile;
    totals above the rows; num_in below numel_seg. Rounding values, so that the order shows; float -> float on counts
    throughout, and a rotation of form, count type and pair on top."""
    for k, n in enumerate(M.ROWS):
        counts, num_in = M.layout(name, n)
        if name == "tile_edges" and n >= T:                               # the layout is what it says
            c, _ = M.clipped_ends("counts", counts, n)
            assert T - 1 in c + np.arange(c.size) and T in c + np.arange(c.size)
        if name == "totals_above":
            assert int(counts.sum()) > n
        run_fsum(dev, "counts", "uint", "float", "float", counts, M.rounding("float", n), name, num_in=num_in)
        form, ct, vt, st = rotate(k + M.LAYOUTS.index(name))
        run_fsum(dev, form, ct, vt, st, counts, M.rows_for(vt, st, n, seed=k), name, num_in=num_in, base=1000 * k + 3)


@pytest.mark.parametrize("vt,st", PAIRS)
def test_forms_count_types_and_pairs(dev, T, vt, st):
    """Both forms x both count types x the pair, on rounding, telescoping and mixed-sign rows over three tiles; the
    telescoping sums are exact, so they also equal the differences they were made from."""
    n = 2 * T + 5
    counts, _ = M.layout("second_empty", n)
    tele = M.telescoping(vt, st, n)
    exact = np.concatenate((np.zeros(1), np.cumsum(tele.astype(np.float64))))
    ends = np.cumsum(counts).astype(np.int64)
    want_tele = (exact[ends] - exact[np.concatenate(([0], ends[:-1]))]).astype(NP[st])
    for form in FORMS:
        for ct in CTS:
            for kind, vals in (("rounding", M.rows_for(vt, st, n)), ("telescoping", tele), ("mixed", M.mixed(vt, n))):
                _, got = run_fsum(dev, form, ct, vt, st, counts, vals, kind, base=77)
                if kind == "telescoping":
                    assert same_bits(got, want_tele), "telescoping sums are not exact"


def test_offsets_with_a_base(dev, T):
    """Offsets rebased on offsets[0]: a slice of a CSR row pointer gives the bits of the counts it stands for."""
    n = T + 1
    counts, _ = M.layout("geometric", n)
    vals = M.rounding("float", n)
    _, ref = run_fsum(dev, "counts", "uint", "float", "float", counts, vals, "counts")
    for ct, base in (("uint", 1), ("uint", (1 << 32) - 1 - n), ("ulong", (1 << 40) + 3)):
        _, got = run_fsum(dev, "offsets", ct, "float", "float", counts, vals, "base %d" % base, base=base)
        assert same_bits(got, ref)


def test_half_values(dev, T):
    """Every finite half, subnormals included, several times over; rows of 65504 whose sums leave half's range."""
    n = 2 * T + 5
    rng = np.random.default_rng(8)
    bits = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    bits[(bits & 0x7c00) == 0x7c00] &= 0x83ff                             # infinities and NaNs become subnormals
    vals = bits.view(np.float16)
    assert (np.abs(vals[vals != 0]) < 6.2e-5).sum() > 100                   # subnormals
    for name in ("geometric", "one", "17"):
        counts, _ = M.layout(name, n)
        run_fsum(dev, "counts", "uint", "half", "float", counts, vals, "finite halves, " + name)
    big = np.full(n, 65504, np.float16)
    big[::3] = -65504
    big[1::7] = np.float16(6e-8)                                            # the smallest subnormal
    _, got = run_fsum(dev, "offsets", "ulong", "half", "float", [n], big, "65504")
    assert abs(float(got[0])) > 65504 * 1000


def test_zeros_infinities_and_nans(dev, T):
    """A segment without a row and a segment of -0.0 rows give +0; infinities and NaNs propagate; +inf with -inf in one
    segment is a NaN."""
    for vt, st in PAIRS:
        dt = NP[vt]
        rows = [[], [-0.0] * 40, [0.0, -0.0], [-0.0], [np.inf, 1.0], [-np.inf] * 3, [np.inf, 2.0, -np.inf], [np.nan, 1.0], [1.0, -1.0], [5.0],
                [-0.0] * (T + 9), [1.0] * 20 + [np.inf] + [1.0] * (T + 3), [3.0] * 18 + [np.nan] + [2.0] * 700, [np.inf] + [0.5] * T + [-np.inf], [], [-0.0]]
        counts = [len(r) for r in rows]
        vals = np.array([x for r in rows for x in r], dt)
        _, got = run_fsum(dev, "counts", "uint", vt, st, counts, vals, "special values")
        b = bits_of(got)
        for r in (0, 1, 2, 3, 8, 10, 14, 15):
            assert b[r] == 0, (vt, st, r, got[r])                           # +0, never -0
        assert got[4] == np.inf and got[5] == -np.inf and np.isnan(got[6]) and np.isnan(got[7]) and got[9] == 5
        assert got[11] == np.inf and np.isnan(got[12]) and np.isnan(got[13])


def long_segment_counts(rng, first, steps, total):
    """Geometric segments over the steps [0, first), one segment over the steps [first, first + steps), geometric ones
    up to `total` steps."""
    from test_gpu_segreduce import fill_steps
    return np.concatenate((fill_steps(rng, first), [steps - 1], fill_steps(rng, total - first - steps))).astype(np.uint64)


@pytest.mark.parametrize("tiles", [16 + 1, 1024 + 1])
def test_a_segment_across_the_threads_and_waves_of_the_carry_scan(dev, T, tiles):
    """One segment over 16 + 1 tiles (its open sums are combined by two threads of the carry scan) and over 1024 + 1
    (by two waves), between short segments; and the same as the only segment."""
    rng = np.random.default_rng(tiles)
    counts = long_segment_counts(rng, 5 * T // 2 + 3, tiles * T, (tiles + 6) * T + 11)
    n = int(counts.sum())
    for (vt, st), form in zip(PAIRS[1:3], FORMS):
        vals = M.rows_for(vt, st, n)
        run_fsum(dev, form, "uint", vt, st, counts, vals, "a segment across %d tiles" % tiles)
    run_fsum(dev, "counts", "ulong", "double", "double", [n], M.rounding("double", n), "one segment of %d tiles" % tiles)


@pytest.fixture(scope="module")
def trip_rows(T):
    from test_gpu_segreduce import CARRY_LAYOUTS, CARRY_TRIP, carry_layout
    assert CARRY_TRIP == M.CARRY_TRIP
    layouts = {name: carry_layout(T, name) for name in CARRY_LAYOUTS}
    rows = max(int(c.sum()) for c, _ in layouts.values())
    return layouts, {st: M.rows_for("float", st, rows, seed=M.TRIP_SEEDS[st]) for st in ("float", "double")}


@pytest.mark.parametrize("st", ["float", "double"])
@pytest.mark.parametrize("which", [0, 1])
def test_open_sums_cross_the_trips_of_the_carry_scan(dev, T, trip_rows, which, st):
    """m + n = (2 * 4096 + 108) T merge steps, the two layouts of test_gpu_segreduce.py's test of the same name: a
    segment across each trip edge, and one segment through the whole second trip. The running state of the trips before
    is added first: in the second layout the state that enters the third trip is ((r + w0) + w1) + w2) + w3, and the rows'
    seeds (segfsum_model.TRIP_SEEDS) are those at which r + (w0 + w1 + w2 + w3) gives other bits. The long segments' sums
    also lie within the bound of D(tiles) additions of the exact sum."""
    from test_gpu_segreduce import CARRY_LAYOUTS
    layouts, rows = trip_rows
    counts, longs = layouts[CARRY_LAYOUTS[which]]
    m, n = counts.size, int(counts.sum())
    assert m + n == (2 * M.CARRY_TRIP + 108) * T
    vals = rows[st][:n]
    _, got = run_fsum(dev, FORMS[which], CTS[which], "float", st, counts, vals, CARRY_LAYOUTS[which], base=5 * which)
    u = 2.0 ** (-24 if st == "float" else -53)
    D = M.depth((m + n) // T)
    for seg, row, length, _, _ in longs:
        x = vals[row:row + length].astype(np.float64)
        assert abs(float(got[seg]) - math.fsum(x)) <= D * u / (1 - D * u) * float(np.abs(x).sum()), (seg, got[seg])


def test_the_same_bits_whatever_the_call(dev, T):
    """The same segments and rows: twice on one object, on views at odd elements, in the other form, with the other count
    type, with num_in equal to and above numel_seg, on two queues at once, on one object moved between queues, and through
    the host form. All give the bits of the first call."""
    clo, ctx, q = dev
    n = 9 * T + 77
    counts, _ = M.layout("second_empty", n, seed=3)
    counts = np.concatenate((counts[:40], np.array([3 * T], np.uint64), counts[40:]))
    n = int(counts.sum())
    for vt, st in PAIRS:
        vals = M.rows_for(vt, st, n)
        vs, ss = vals.dtype.itemsize, np.dtype(NP[st]).itemsize
        obj = clo.SegFSum("counts", ctx, vt, st, "uint")
        qs = [clo.Queue(ctx), clo.Queue(ctx)]
        try:
            _, ref = run_fsum(dev, "counts", "uint", vt, st, counts, vals, "first", obj=obj)
            again = [run_fsum(dev, "counts", "uint", vt, st, counts, vals, "second", obj=obj)[1]]
            for offs in ((4, vs, ss), (12, 3 * vs, ss), (8, 5 * vs, 3 * ss)):
                again.append(run_fsum(dev, "counts", "uint", vt, st, counts, vals, "views at %s" % (offs,), offs=offs, obj=obj)[1])
            for form, ct in (("offsets", "uint"), ("counts", "ulong"), ("offsets", "ulong")):
                again.append(run_fsum(dev, form, ct, vt, st, counts, vals, "other form or count type", base=12345)[1])
            for num_in in (counts.size, counts.size + 5):
                again.append(run_fsum(dev, "counts", "uint", vt, st, counts, vals, "num_in", num_in=num_in, obj=obj)[1])
            for j, qi in enumerate((0, 1, 0)):                              # one object moved between queues
                again.append(run_fsum((clo, ctx, qs[qi]), "counts", "uint", vt, st, counts, vals, "moved, call %d" % j, obj=obj, q=qs[qi])[1])
            # two objects on two queues, nothing waits in between
            objs = [clo.SegFSum(FORMS[i], ctx, vt, st, CTS[i]) for i in range(2)]
            regs = []
            for i in range(2):
                src = M.source(FORMS[i], counts, CDT[CTS[i]], 9)
                rdev = (clo, ctx, qs[i])
                regs.append([Region(rdev, src.nbytes, 0, src, 0), Region(rdev, vals.nbytes, 0, vals, 1), Region(rdev, counts.size * ss, 0, None, 2),
                             Region(rdev, 8, 0, None, 0)])
            for i in range(2):
                qs[i].finish()
            for i in range(2):
                assert objs[i].with_device_data(qs[i], regs[i][0].view, None, regs[i][1].view, regs[i][2].view, regs[i][3].view, counts.size, n)
            for i in range(2):
                qs[i].finish()
                r = regs[i][2]
                again.append(r.base.read(qs[i], np.uint8, r.host.size)[r.at:r.at + counts.size * ss].copy().view(NP[st]))
                regs[i][3].check(np.array([n], np.uint64), "num_out on queue %d" % i)
                for x in regs[i]:
                    x.close()
                objs[i].close()
            host, total = obj.with_host_data(counts.astype(np.uint32), vals, q_exec=q)
            assert total == n
            again.append(host)
            for k, a in enumerate(again):
                assert same_bits(a, ref), (vt, st, k)
        finally:
            obj.close()
            for x in qs:
                x.close()


def test_host_data_form(dev, T):
    clo, ctx, q = dev
    counts, _ = M.layout("second_empty", 2 * T + 9)
    total = int(counts.sum())
    for form in FORMS:
        for (vt, st), ct in zip(PAIRS, CTS * 2):
            src = M.source(form, counts, CDT[ct], 4321)
            sf = clo.SegFSum(form, ctx, vt, st, ct)
            for n in (0, total - 5, total, total + 7):
                vals = M.rows_for(vt, st, n)
                for num_in, qe in ((None, q), (counts.size // 2, None), (counts.size + 9, q)):
                    sums, t = segfsum(form, src, vals, st, num_in)
                    a, got = sf.with_host_data(src, vals, num_in=num_in, q_exec=qe)
                    assert got == t and a.dtype == sums.dtype and same_bits(a, sums), (form, ct, vt, st, n, num_in)
            sf.close()


def test_thin_abi_status_codes(dev, T):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    HALF, FLOAT, DOUBLE, UINT = (clo.CLO_TYPES[t] for t in ("half", "float", "double", "uint"))
    m_h, n = 1000, 3 * T
    need = lib.clo_hip_segfsum_workspace_bytes(m_h, n)
    assert need > 0 and need % 256 == 0
    counts = np.random.default_rng(5).integers(0, 9, 2 * m_h + 4, dtype=np.uint32)
    vals = M.rounding("float", 2 * n + 4)
    cn, vi, ni = Region(dev, counts.nbytes, 0, counts, 0), Region(dev, vals.nbytes, 0, vals, 1), Region(dev, 16, 0, np.array([m_h // 2, 0], np.uint64), 2)
    so, num = Region(dev, 8 * m_h + 16, 0, None, 0), Region(dev, 16, 0, None, 1)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(c_p, v_p, a_p, form=0, cs=4, n_p=None, num_p=num.ptr, numel_seg=m_h, numel=n, vt=FLOAT, st=FLOAT, w=ws.ptr, wb=need):
        return lib.clo_hip_segfsum(form, c_p, cs, n_p, v_p, a_p, num_p, numel_seg, numel, vt, st, w, wb, s)

    try:
        full = (cn.ptr, vi.ptr, so.ptr)
        for form in (-1, 2, 100):
            assert call(*full, form=form) == EARGS
        for cs in (0, 1, 2, 3, 16):
            assert call(*full, cs=cs) == EUNSUPPORTED, cs
        for vt, st in ((UINT, UINT), (FLOAT, UINT), (UINT, FLOAT), (HALF, HALF), (FLOAT, HALF), (DOUBLE, FLOAT), (HALF, DOUBLE), (-1, FLOAT), (FLOAT, 11)):
            assert call(*full, vt=vt, st=st) == EUNSUPPORTED, (vt, st)
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(*full, n_p=ni.ptr + 4) == EARGS                                                     # num_in misaligned
        assert call(*full, numel_seg=1 << 32) == EARGS and call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, so.ptr) == EARGS and call(None, None, None, form=1, numel_seg=0, numel=0) == EARGS
        assert call(cn.ptr, None, so.ptr) == EARGS and call(cn.ptr, vi.ptr, None) == EARGS              # values_in, sums_out missing
        for i in range(3):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        assert call(cn.ptr, vi.ptr + 1, so.ptr, vt=HALF) == EARGS                                       # a half at an odd byte
        for i, kw in ((0, dict(cs=8)), (1, dict(vt=DOUBLE, st=DOUBLE)), (2, dict(st=DOUBLE))):          # 4-aligned is not 8-aligned
            args = list(full)
            args[i] += 4
            assert call(*args, **kw) == EARGS, i
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        q.finish()
        for r in (so, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; num_in; views at an odd element; numel_seg 0
        # needs no workspace, no input
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        rows = lambda dt, k: so.base.read(q, np.uint8, so.host.size)[so.at:so.at + k * np.dtype(dt).itemsize].copy().view(dt)
        assert call(*full) == 0
        q.finish()
        want, t = segfsum("counts", counts[:m_h], vals[:n], "float")
        assert first() == t and same_bits(rows(np.float32, m_h), want)
        assert call(*full, n_p=ni.ptr, st=DOUBLE) == 0
        q.finish()
        want, t = segfsum("counts", counts[:m_h], vals[:n], "double", m_h // 2)
        assert first() == t and same_bits(rows(np.float64, m_h // 2), want)
        assert call(cn.ptr + 4, vi.ptr + 2, so.ptr + 4, vt=HALF) == 0
        q.finish()
        halves = vals.view(np.float16)[1:n + 1]
        want, t = segfsum("counts", counts[1:m_h + 1], halves, "float")
        assert first() == t and same_bits(rows(np.float32, m_h + 1)[1:], want)
        assert call(None, vi.ptr, None, numel_seg=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (cn, vi, ni, so, num):
            r.close()


@pytest.mark.parametrize("form", FORMS)
def test_graph_capture_and_replay(dev, T, form):
    """clo_hip_segfsum captured from one client stream (a linear graph) after one eager warm-up and replayed three times,
    the counts, num_in and the values rewritten and sums_out and num_out refilled with a canary before each replay (the
    protocol of test_gpu_graph_capture.py): the same shapes, other totals, one of them above the rows."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    m_h, n = 900, 4 * T + 3
    need = lib.clo_hip_segfsum_workspace_bytes(m_h, n)
    made = [GC.Mem(gdev, x) for x in (4 * (m_h + 1), 8, 4 * n, 8 * m_h, 8, need)]
    src_m, nin_m, vi, so, num, ws = made
    means = [16, 3, 40, 9, 16]                                              # 900 segments of mean 40: above the rows
    totals = set()
    FLOAT, DOUBLE = clo.CLO_TYPES["float"], clo.CLO_TYPES["double"]

    def load(r):
        counts = (np.random.default_rng(300 + r).geometric(1 / means[r], m_h) - (np.arange(m_h) % 4 == r % 4)).astype(np.uint64)
        src, num_in, vals = M.source(form, counts, np.uint32, 50 * r), m_h - 100 * (r % 3), M.rows_for("float", "double", n, seed=r)
        for m in (so, num):
            m.fill()
        for mem_, arr in ((src_m, src), (nin_m, np.array([num_in], np.uint64)), (vi, vals)):
            mem_.put(arr)
        want = segfsum(form, src, vals, "double", num_in)
        totals.add(want[1])
        return want, vals

    def enqueue():
        return lib.clo_hip_segfsum(FORMS.index(form), src_m.ptr, 4, nin_m.ptr, vi.ptr, so.ptr, num.ptr, m_h, n, FLOAT, DOUBLE, ws.ptr, need, q.stream)

    def verify(r, want):
        (sums, total), vals = want
        tag = "%s round %d" % (form, r)
        assert int(num.get(np.uint64, 1)[0]) == total, tag + ": num_out"
        GC.same(so.get(np.float64, m_h), np.concatenate((sums, GC.canary(np.float64, m_h - sums.size))), tag + ": sums_out")
        GC.same(vi.get(np.float32, n), vals, "values_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(totals) >= 4 and max(totals) > n > min(totals), totals
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def test_broken_preconditions_stay_in_bounds(dev, T):
    """Offsets that descend or are unordered, counts whose sums wrap 2^64, a num_in above numel_seg: the call completes,
    the canaries and the inputs are intact. Contents are not compared: clo_hip_seg_device.h gives the argument that this
    holds by construction, and this run shows it once."""
    rng = np.random.default_rng(90)
    m_h, n = 3 * T + 700, 3 * T + 5
    descending = ((m_h - np.arange(m_h + 1)) * 2).astype(np.uint32)
    unordered = rng.integers(0, 2 * n, m_h + 1).astype(np.uint64)
    wrapping = (rng.integers(0, 1 << 62, m_h, dtype=np.uint64) << np.uint64(2)) | np.uint64(1)
    for i, (form, ct, src) in enumerate((("offsets", "uint", descending), ("offsets", "ulong", unordered), ("counts", "ulong", wrapping))):
        vt, st = PAIRS[i + 1]
        run_fsum(dev, form, ct, vt, st, None, M.rounding(vt, n), "broken preconditions", num_in=m_h + 1000, src=src, compare=False)


def test_round_trip_through_expand(dev, T):
    """segfsum(expand(v, counts), counts) == v * counts where the products and every partial sum are exact: small
    integers as floats, empty segments included."""
    clo, ctx, q = dev
    counts, _ = M.layout("geometric", 3 * T + 77, seed=22)
    counts[::4] = 0
    m, n = counts.size, int(counts.sum())
    for ct, vt, st, bits in (("uint", "float", "float", "uint"), ("ulong", "double", "double", "ulong"), ("uint", "float", "double", "uint")):
        vals = np.random.default_rng(22).integers(-1000, 1001, m).astype(NP[vt])
        vs, ss = vals.dtype.itemsize, np.dtype(NP[st]).itemsize
        c_r, v_r = Region(dev, counts.size * np.dtype(CDT[ct]).itemsize, 0, counts.astype(CDT[ct]), 0), Region(dev, vals.nbytes, 0, vals, 1)
        rows_r, n1_r, a_r, n2_r = Region(dev, vs * n, 0, None, 2), Region(dev, 8, 0, None, 0), Region(dev, ss * m, 0, None, 1), Region(dev, 8, 0, None, 2)
        ex, sf = clo.Expand("counts", ctx, bits, ct), clo.SegFSum("counts", ctx, vt, st, ct)
        try:
            assert ex.with_device_data(q, c_r.view, None, v_r.view, rows_r.view, None, None, n1_r.view, m, n)
            assert sf.with_device_data(q, c_r.view, None, rows_r.view, a_r.view, n2_r.view, m, n)
            q.finish()
            n2_r.check(np.array([n], np.uint64), "num_out")
            a_r.check((vals.astype(np.float64) * counts.astype(np.float64) + 0.0).astype(NP[st]), "values * counts")
        finally:
            for x in (c_r, v_r, rows_r, n1_r, a_r, n2_r, ex, sf):
                x.close()


def test_against_segreduce_on_small_integers(dev, T):
    """Small non-negative integers as floats: every sum is exact, and equals CloSegReduce's of the same values as uint."""
    clo, ctx, q = dev
    n = 3 * T + 5
    counts, num_in = M.layout("totals_above", n)
    ints = np.random.default_rng(31).integers(0, 1000, n).astype(np.uint32)
    sr = clo.SegReduce("sum", "counts", ctx, "uint", "uint", "uint")
    try:
        aggr, total = sr.with_host_data(counts.astype(np.uint32), ints, q_exec=q)
    finally:
        sr.close()
    for vt, st in PAIRS:
        t, got = run_fsum(dev, "counts", "uint", vt, st, counts, ints.astype(NP[vt]), "small integers")
        assert t == total and np.array_equal(got.astype(np.uint32), aggr) and np.array_equal(got, aggr.astype(NP[st]))
