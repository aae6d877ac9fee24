"""CloSegScan (include/clo_segscan.h) below the level of the tile: the constructed inputs of tests/segscan_lane_cases.py,
each through run_scan of test_gpu_segscan.py (num_out, the rows bit for bit against the numpy model, the rows beyond, the
guards and the inputs). What every input reaches in the kernels (lanes with 17 closes and with none, closes on a lane's
first and last step, waves of closes and of rows, short and empty lanes, tiles without rows and without rows to store;
every division of TAILS' stretch at every address residue; CARRY's two load paths at 1, 15, 16, 17, 31, 32 and 33 tiles)
is asserted on the CPU by tests/test_segscan_lane_reach_cpu.py. Every input meets sum, min and max, each with a 32-bit
and a 64-bit sum type (the inputs aimed at 8-byte values: 64-bit ones only), both kinds, both forms and both count types
in turn, and runs again in place wherever the widths match. The values are values_for's with the types' extremes planted
before the runs of closes and the edges a case is aimed at. Last, segment scan -> segment reduce on one queue without a
host wait, and the same chain with two objects each on two queues."""
import numpy as np
import pytest

from segreduce_model import segreduce
from segscan_lane_cases import all_cases, rotate, size
from segscan_lane_model import ITEMS, lanes
from segscan_model import FORMS, NP, OPS, segscan
from test_gpu_histogram import Region
from test_gpu_segreduce import values_for
from test_gpu_segscan import run_scan

pytestmark = pytest.mark.gpu

T_CPU = 17 * 256   # only to name the parametrised cases; the fixture asserts it is the library's tile
CASES = all_cases(T_CPU)


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def T(dev):
    t = dev[0].segscan_tile(4, 4)
    assert t == T_CPU
    return t


@pytest.fixture(scope="module")
def base_values(T):
    """One array of values per value type, shared by the cases and left unchanged."""
    vals = {vt: values_for(vt, 33 * T, 40 + i) for i, vt in enumerate(NP)}
    for v in vals.values():
        v.setflags(write=False)
    return vals


@pytest.mark.parametrize("number", range(len(CASES)), ids=lambda i: CASES[i].name.replace(" ", "_"))
def test_constructed_inputs(dev, T, base_values, number):
    case = CASES[number]
    ran = 0
    for k in range(6):
        op, incl, form, ct, (vt, st) = rotate(number, k, case.value_size)
        vals = case.values(vt, op, base_values[vt])
        offs = (0, case.align if case.value_size else 0, 0)
        for in_place in (False, True)[:2 if size(vt) == size(st) else 1]:
            got, data = run_scan(dev, op, incl, form, ct, vt, st, case.counts, case.n, case.name, base=number, offs=offs, vals=vals, in_place=in_place)
            assert got == int(case.counts.sum()) and data.size == min(got, case.n)
            ran += 1
    assert ran >= 8


@pytest.mark.parametrize("form", FORMS)
def test_lengths_16_17_and_18_in_turn(dev, T, base_values, form):
    """Segments of 16, 17 and 18 rows repeat: the closes drift through all 17 steps of the lanes within one tile, which the
    lane model says of this very input before it runs, every op and kind on it."""
    (case,) = [c for c in CASES if c.name.startswith("lengths 16")]
    src = case.counts if form == "counts" else np.concatenate(([0], np.cumsum(case.counts)))
    L = lanes(form, src, case.n, T)
    bits = (L.closes[0][:, None] >> np.arange(ITEMS)) & 1
    assert (bits.sum(axis=0) > 0).all()
    k = 0
    for op in OPS:
        for incl in (False, True):
            vt, st = (("int", "int"), ("uint", "ulong"), ("long", "long"))[k % 3]
            run_scan(dev, op, incl, form, ("uint", "ulong")[k % 2], vt, st, case.counts, case.n, case.name, vals=case.values(vt, op, base_values[vt]),
                     in_place=size(vt) == size(st) and k % 2 == 1)
            k += 1


def _chain(dev, queues, counts_list, vals_list):
    """SegScan (inclusive sum) -> SegReduce (max over the running sums) for every (counts, values) on its queue, nothing
    waiting for the device before everything is enqueued; then the checks."""
    clo, ctx, _ = dev
    made, sent = [], []
    try:
        for q, counts, vals in zip(queues, counts_list, vals_list):
            rdev = (clo, ctx, q)
            m, n = counts.size, vals.size
            regs = [Region(rdev, 4 * m, 0, counts.astype(np.uint32), 0), Region(rdev, 4 * n, 0, vals, 1), Region(rdev, 8 * n, 0, None, 2),
                    Region(rdev, 8, 0, None, 0), Region(rdev, 8 * m, 0, None, 1), Region(rdev, 8, 0, None, 2)]
            objs = [clo.SegScan("sum", "counts", ctx, "uint", "ulong", "uint", inclusive=True), clo.SegReduce("max", "counts", ctx, "ulong", "ulong", "uint"),
                    clo.SegReduce("sum", "counts", ctx, "uint", "ulong", "uint")]
            made += regs + objs
            extra = Region(rdev, 8 * m, 0, None, 0), Region(rdev, 8, 0, None, 1)
            made += list(extra)
            sent.append((q, counts, vals, regs, objs, extra))
        for q in queues:
            q.finish()                                                         # the uploads; from here on nothing waits
        for q, counts, vals, regs, (sc, mx, sm), extra in sent:
            m, n = counts.size, vals.size
            assert sc.with_device_data(q, regs[0].view, None, regs[1].view, regs[2].view, regs[3].view, m, n)
            assert mx.with_device_data(q, regs[0].view, None, regs[2].view, regs[4].view, regs[5].view, m, n)
            assert sm.with_device_data(q, regs[0].view, None, regs[1].view, extra[0].view, extra[1].view, m, n)
        for q in queues:
            q.finish()
        for i, (q, counts, vals, regs, objs, extra) in enumerate(sent):
            what = "chain %d" % i
            m, n = counts.size, vals.size
            running, total = segscan("sum", "counts", counts, vals, "ulong", True)
            assert total == n
            top, _ = segreduce("max", "counts", counts, running, "ulong")
            sums, _ = segreduce("sum", "counts", counts, vals, "ulong")
            assert np.array_equal(top[counts > 0], sums[counts > 0])             # non-negative values: the last running sum is the largest
            regs[2].check(running, what + ": the running sums")
            regs[4].check(top, what + ": the maximum of every segment's running sums")
            for r in (regs[3], regs[5], extra[1]):
                r.check(np.array([n], np.uint64), what + ": a total")
            got = regs[4].base.read(q, np.uint8, regs[4].host.size)[regs[4].at:regs[4].at + 8 * m].copy().view(np.uint64)
            reduced = extra[0].base.read(q, np.uint8, extra[0].host.size)[extra[0].at:extra[0].at + 8 * m].copy().view(np.uint64)
            assert np.array_equal(got[counts > 0], reduced[counts > 0]), what + ": differs from the segment reduce's sums"
            assert np.array_equal(reduced, sums), what
    finally:
        for x in made:
            x.close()


def _chain_input(T, seed, total):
    rng = np.random.default_rng(seed)
    counts = rng.geometric(1 / 16.0, total // 12).astype(np.int64)
    counts[rng.random(counts.size) < 0.2] = 0
    counts[counts.size // 3] = T + T // 2                                      # a segment across two tile edges
    counts = counts[:int(np.searchsorted(np.cumsum(counts), total))]
    return counts, rng.integers(0, 1 << 32, int(counts.sum()), dtype=np.uint64).astype(np.uint32)


def test_chain_into_segment_reduce_without_a_host_wait(dev, T):
    """Segment scan (inclusive sum, uint in ulong) -> segment reduce (max) of the running sums on one non-profiling queue
    with a single finish: for non-negative values the maximum of a segment's running sums is the segment's sum, which a
    segment reduce (sum) of the values gives on the same queue; all three against the numpy models. Then the same chain
    with two objects of each kind on two queues."""
    clo, ctx, _ = dev
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    try:
        a, b = _chain_input(T, 51, 3 * T + 9), _chain_input(T, 52, 5 * T + 1)
        _chain(dev, qs[:1], [a[0]], [a[1]])
        _chain(dev, qs, [a[0], b[0]], [a[1], b[1]])
    finally:
        for q in qs:
            q.close()
