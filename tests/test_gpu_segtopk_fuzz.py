"""A seeded, stratified fuzz of CloSegTopK (include/clo_segtopk.h) on the GPU: 200 cases, every one against the numpy
model of tests/segtopk_model.py bit for bit, through the checked views of test_gpu_segtopk.run_topk (guards, inputs and
every unwritten slot unchanged). The strata: k over (1, 2, 5, 16, 63, 64, 65, 200, cap / 2, cap) x mean segment length
over (1, 16, T / 2, 4 T) x the share of empty segments over (0, 1 / 2) — 80 combinations, each met at least twice — while
the key type (eleven), the value mode (five), which, the form and the count type rotate with periods that are coprime to
one another, so that every pair of them meets. n <= 16 T, and fewer rows where short segments meet a large k, so that
the outputs stay below 2^22 slots; the row count is at, below or above the total, every seventh case has a num_in, a
third of the cases have few distinct keys. One object per configuration, so that workspaces are
reused between shapes. No case is skipped: every key and value size is built, which is asserted."""
import numpy as np
import pytest

from segtopk_model import FORMS, KEY_NP, WHICH
from test_gpu_segsort import MODES, VS
from test_gpu_segtopk import run_topk

pytestmark = pytest.mark.gpu

CASES, CHUNKS = 200, 8
MEANS = ("1", "16", "T/2", "4T")
EMPTY = (0.0, 0.5)


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def ks_of(cap):
    return (1, 2, 5, 16, 63, 64, 65, 200, cap // 2, cap)


def stratum(case, T, cap):
    """The case's parameters: the 80 combinations of (k, mean, empty share) in turn, the rest by coprime periods."""
    kk = ks_of(cap)
    k = kk[case % len(kk)]
    mean = MEANS[(case // len(kk)) % len(MEANS)]
    empty = EMPTY[(case // (len(kk) * len(MEANS))) % len(EMPTY)]
    kts = tuple(KEY_NP)
    return dict(k=k, mean=mean, empty=empty, kt=kts[case % len(kts)], mode=MODES[case % len(MODES)], which=WHICH[case % 2],
                form=FORMS[(case // 2) % 2], ct=("uint", "ulong")[(case // 3) % 2])


def counts_of(rng, s, T):
    mean = {"1": 1, "16": 16, "T/2": T // 2, "4T": 4 * T}[s["mean"]]
    n = int(rng.integers(1, 16 * T + 1))
    n = min(n, max((1 << 21) // s["k"], 8) * mean)                         # at most 2^21 slots of output (2^22 with the empty segments)
    c = rng.geometric(1 / mean, n // mean + 2) if mean > 1 else np.ones(n + 2, np.int64)
    c = c[:max(int(np.searchsorted(np.cumsum(c), n)), 1)]
    if s["empty"]:
        both = np.zeros(2 * c.size, np.int64)
        both[rng.permutation(2 * c.size)[:c.size]] = c                       # as many empty segments as others, anywhere
        c = both
    return c


@pytest.mark.parametrize("chunk", range(CHUNKS))
def test_strata(dev, chunk):
    clo, ctx, q = dev
    T, cap = clo.segtopk_tile(4, 0), clo.segtopk_k_max(4, 0)
    objs = {}
    try:
        for case in range(chunk, CASES, CHUNKS):
            s = stratum(case, T, cap)
            rng = np.random.default_rng(9000 + case)
            c = counts_of(rng, s, T)
            total = int(c.sum())
            assert total <= 16 * T + 4 * T                                    # (the last segment may pass the draw)
            n = (total, max(total - int(rng.integers(1, T)), 0), total + int(rng.integers(1, T)))[case // 5 % 3]
            key = (s["which"], s["form"], s["ct"], s["kt"], VS[s["mode"]])
            if key not in objs:
                objs[key] = clo.SegTopK(s["which"], s["form"], ctx, s["kt"], VS[s["mode"]], s["ct"])
            num_in = None if case % 7 else int(rng.integers(0, c.size + 3))
            run_topk(dev, s["which"], s["form"], s["ct"], s["kt"], s["mode"], c, n, s["k"], "fuzz case %d (mean %s, empty %s)" % (case, s["mean"], s["empty"]),
                     num_in=num_in, base=case, obj=objs[key], seed=case, distinct=7 if case % 3 == 0 else None)
    finally:
        for o in objs.values():
            o.close()


def test_the_strata_are_all_met_and_nothing_is_skipped(dev):
    clo = dev[0]
    T, cap = clo.segtopk_tile(4, 0), clo.segtopk_k_max(4, 0)
    for ks in (1, 2, 4, 8):
        for vs in (0, 4, 8):
            assert clo.segtopk_tile(ks, vs) > 0 and clo.segtopk_k_max(ks, vs) == cap
    met = {}
    for case in range(CASES):
        s = stratum(case, T, cap)
        met[(s["k"], s["mean"], s["empty"])] = met.get((s["k"], s["mean"], s["empty"]), 0) + 1
    assert len(met) == len(ks_of(cap)) * len(MEANS) * len(EMPTY) and min(met.values()) >= 2
    for a, b, count in (("kt", "mode", 55), ("kt", "which", 22), ("mode", "form", 10), ("which", "ct", 4), ("kt", "k", 110)):
        assert len({(stratum(c, T, cap)[a], stratum(c, T, cap)[b]) for c in range(CASES)}) == count, (a, b)
