"""A seeded stratified fuzz of CloSegScan (include/clo_segscan.h) on the GPU: the 216 strata of tests/segscan_strata.py
(form x count type x type pair x op x kind x length distribution x clip x num_in, each with n <= 4 T rows), every one
through the checks of test_gpu_segscan.py's run_scan: num_out, the rows below min(total, n) bit for bit against the
model, the rows beyond, the guards and the inputs untouched. What the strata reach (tiles without a close, closes on a
tile's first and last step, empty segments at a tile edge, totals above and below n) is asserted on the CPU by
tests/test_segscan_cpu.py. Then the 96 strata of strata_lanes(): lengths at the scale of a lane and a wave (runs of
empty segments, lengths around 17, blocks of 64 x 17 empties, lone rows), a third of them in place; what they reach is
asserted there too."""
import pytest

from segscan_strata import LANE_STRATA, STRATA, strata, strata_lanes
from test_gpu_segscan import run_scan

pytestmark = pytest.mark.gpu

GROUPS = 8
LANE_GROUPS = 4


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


@pytest.fixture(scope="module")
def cases(dev):
    return strata(dev[0].segscan_tile(4, 4))


@pytest.mark.parametrize("group", range(GROUPS))
def test_strata(dev, cases, group):
    assert len(cases) == STRATA
    for k in range(group, STRATA, GROUPS):
        s = cases[k]
        what = "stratum %d: %s, clip %s, num_in %s" % (k, s["dist"], s["clip"], s["num_mode"])
        got, data = run_scan(dev, s["op"], s["inclusive"], s["form"], s["count_type"], s["value_type"], s["sum_type"], None, s["n"], what,
                             num_in=s["num_in"], src=s["src"], vals=s["values"], offs=((0, 4, 8)[k % 3] if s["count_type"] == "uint" else (0, 8)[k % 2], 0, 0))
        assert data.size <= s["n"]


@pytest.fixture(scope="module")
def lane_cases(dev):
    return strata_lanes(dev[0].segscan_tile(4, 4))


@pytest.mark.parametrize("group", range(LANE_GROUPS))
def test_lane_strata(dev, lane_cases, group):
    assert len(lane_cases) == LANE_STRATA
    for k in range(group, LANE_STRATA, LANE_GROUPS):
        s = lane_cases[k]
        what = "lane stratum %d: %s, clip %s, num_in %s" % (k, s["dist"], s["clip"], s["num_mode"])
        vs = s["values"].dtype.itemsize
        got, data = run_scan(dev, s["op"], s["inclusive"], s["form"], s["count_type"], s["value_type"], s["sum_type"], None, s["n"], what,
                             num_in=s["num_in"], src=s["src"], vals=s["values"], in_place=s["in_place"],
                             offs=(0, vs * (k % (16 // vs)), 0))                  # the values at every element-aligned residue
        assert data.size <= s["n"]
