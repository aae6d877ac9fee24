"""tests/fscan_model.py without a GPU: the model against truths that do not depend on it (exact integer prefix sums
on telescoping inputs, long-double sums on uniform ones, numpy_ops.scan_cast_expected for integer sum types, the IEEE
specials), and the inputs of tests/test_gpu_float_scan.py against six deliberately different models: a bit comparison
on these inputs cannot pass a scan that adds in another order, loses an element or counts one twice."""
import numpy as np
import pytest

import fscan_model as F
from numpy_ops import scan_cast_expected

BIG = [n for n in F.SIZES if n > F.TILE]            # every size of the GPU test with more than one tile


def differing(x, y):
    """The share of positions at which two results differ in bits."""
    u = "u%d" % x.dtype.itemsize
    return float(np.mean(x.view(u) != y.view(u)))


# ---------------------------------------------------------------------------------------------------------------------
# deliberately different models: (a) .. (d) add in another order, (e) and (f) add other things
# ---------------------------------------------------------------------------------------------------------------------

def variant_a(a, sdt):
    """Plain left-to-right sums in the sum type (numpy accumulates element by element, rounding each step to the
    type of the array: test_cumsum_rounds_every_step)."""
    v = F.convert(a, sdt)
    return np.concatenate((np.zeros(1, sdt), np.cumsum(v[:-1], dtype=sdt)))


def variant_b(monkeypatch):
    """Thread offset as `incl - mine`."""
    def block_parts(mine):
        incl = F.wave_scan(mine)
        base, _, total = model_block_parts(mine)
        return base, incl - mine.reshape(incl.shape), total
    model_block_parts = F.block_parts
    monkeypatch.setattr(F, "block_parts", block_parts)


def variant_c(monkeypatch):
    """Tile total as (w0 + w1) + (w2 + w3); the wave bases stay left to right."""
    def block_parts(mine):
        base, excl, _ = model_block_parts(mine)
        w = F.wave_scan(mine)[:, :, F.WAVE - 1]
        return base, excl, (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])
    model_block_parts = F.block_parts
    monkeypatch.setattr(F, "block_parts", block_parts)


def variant_d(monkeypatch):
    """Tile offset folded in as base + (excl + tile_excl)."""
    monkeypatch.setattr(F, "thread_offsets", lambda base, excl, tile_excl:
                        (base + (excl + tile_excl[:, None, None])).reshape(-1, F.THREADS))


def variant_e(a, sdt, k):
    """Element k is never loaded."""
    v = F.convert(a, sdt)
    v[k] = 0
    return F.scan_converted(v)


def variant_f(a, sdt, k):
    """Element k, the first of its tile, is added into the last slot of the tile before it as well."""
    assert k % F.TILE == 0 and k > 0
    v = F.convert(a, sdt)
    v[k - 1] = v[k - 1] + v[k]
    return F.scan_converted(v)


def run_variant(patch, a, sdt):
    with pytest.MonkeyPatch.context() as mp:
        patch(mp)
        return F.scan(a, sdt)


def test_cumsum_rounds_every_step():
    """What variant (a) relies on: numpy's cumsum in half and in float rounds after every addition."""
    for sdt in (np.float16, np.float32):
        a = F.uniform("half" if sdt is np.float16 else "float", 3000)
        run, want = sdt(0), np.empty(3000, sdt)
        for i in range(3000):
            run = sdt(np.float64(run) + np.float64(a[i]))          # (53 >= 2 * 24 + 2: one correct rounding)
            want[i] = run
        assert F.same_bits(np.cumsum(a, dtype=sdt), want)


# ---------------------------------------------------------------------------------------------------------------------
# the model against independent truths
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("st", F.SUM_TYPES)
@pytest.mark.parametrize("n", [1, 17, 4096, 4097, 1 << 24, (1 << 24) + 1])
def test_telescoping_input_gives_the_exact_integer_sums(st, n):
    d = F.telescoping_steps(st, n)
    got = F.scan(F.telescoping(st, n), F.NP[st])
    assert got.dtype == F.NP[st] and got.size == n
    assert np.array_equal(got.astype(np.float64).astype(np.int64), d[:-1] - d[0])       # (< 2^53: exact in a double)


@pytest.mark.parametrize("st", F.SUM_TYPES)
@pytest.mark.parametrize("n", [4097, (1 << 20) + 3])
def test_uniform_input_stays_within_the_tolerance_of_the_older_tests(st, n):
    """256 eps (cumsum|a| + 1) of the long-double sums, the bound of test_gpu_views.py::test_float_scan."""
    a = F.uniform(st, n)
    wide = a.astype(np.longdouble)
    exact = np.concatenate(([0.0], np.cumsum(wide)[:-1]))
    scale = np.concatenate(([0.0], np.cumsum(np.abs(wide))[:-1])) + 1.0
    err = np.abs(F.scan(a, F.NP[st]).astype(np.longdouble) - exact) / scale
    assert np.all(err <= 256 * np.finfo(F.NP[st]).eps), float(err.max() / np.finfo(F.NP[st]).eps)


@pytest.mark.parametrize("et,st", [("ulong", "uint"), ("long", "short"), ("uint", "uchar"), ("float", "int"), ("double", "long"),
                                   ("half", "uint"), ("double", "uchar"), ("float", "ulong")])
@pytest.mark.parametrize("n", [1, 4097, (1 << 20) + 3, (1 << 24) + 5])
def test_integer_sum_types_reduce_to_scan_cast_expected(et, st, n):
    """The pairs and inputs of test_gpu_round3.py::test_scan_into_narrower_or_integer_sums."""
    from cl_ops_amd.api import CLO_TYPE_NP
    edt, sdt = CLO_TYPE_NP[et], CLO_TYPE_NP[st]
    rng = np.random.default_rng(n % 991 + len(et) + len(st))
    if np.issubdtype(edt, np.floating):
        si = np.iinfo(sdt)
        hi = min(300.0, float(si.max))
        lo = -min(300.0, float(-si.min)) if si.min < 0 else 0.0
        a = (rng.random(n) * (hi - lo) * 0.999 + lo).astype(edt)
    else:
        info = np.iinfo(edt)
        a = rng.integers(info.min, info.max, n, dtype=edt, endpoint=True)
    got = F.scan(a, sdt)
    assert got.dtype == sdt and np.array_equal(got, scan_cast_expected(a, sdt))


def test_numpy_casts_round_to_nearest_even():
    """What fscan_model.convert relies on: `astype` is the correctly rounded C cast, also from 64-bit integers, from
    double to half in one step (not by way of float), and beyond the range of the target."""
    def cast(values, edt, sdt):
        return [float(x) for x in F.convert(np.array(values, dtype=edt), sdt)]
    assert cast([(1 << 24) + 1, (1 << 24) + 3, (1 << 63) + (1 << 39), (1 << 63) + (1 << 39) + 1], np.uint64, np.float32) \
        == [2.0 ** 24, 2.0 ** 24 + 4, 2.0 ** 63, 2.0 ** 63 + 2.0 ** 40]
    assert cast([(1 << 53) + 1, (1 << 53) + 3, -(1 << 53) - 1], np.int64, np.float64) == [2.0 ** 53, 2.0 ** 53 + 4, -2.0 ** 53]
    assert cast([1 + 2.0 ** -24, 1 + 3 * 2.0 ** -24, 1 + 2.0 ** -24 + 2.0 ** -50, 3.5e38], np.float64, np.float32) \
        == [1.0, 1 + 2.0 ** -22, 1 + 2.0 ** -23, np.inf]
    for edt in (np.float64, np.float32):
        assert cast([1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, 65519.996, 65520.0, -70000.0], edt, np.float16) \
            == [1.0, 1 + 2.0 ** -9, 65504.0, np.inf, -np.inf]
    assert cast([1 + 2.0 ** -11 + 2.0 ** -30], np.float64, np.float16) == [1 + 2.0 ** -10]
    assert cast([2049, 2051, 65519, 65520, -1000003], np.int32, np.float16) == [2048.0, 2052.0, 65504.0, np.inf, -np.inf]


# ---------------------------------------------------------------------------------------------------------------------
# the inputs discriminate
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("st", F.SUM_TYPES)
@pytest.mark.parametrize("n", BIG)
def test_rounding_input_tells_the_addition_orders_apart(st, n):
    """Shares of positions whose bits differ from the model's, measured (half / float / double):

        n                      (a) cumsum        (b) incl - mine   (c) (w0+w1)+(w2+w3)   (d) base+(excl+tile)
        4097                   .91 / .92 / .98   .62 / .51 / .55   one position each     none (see below)
        8193                   .94 / .93 / .94   .61 / .47 / .44   .26 / .12 / .30       .097 / .005 / .042
        64 * 4096 - 1          1.0 / .99 / 1.0   .56 / .59 / .62   .79 / .31 / .61       .12 / .12 / .11
        64 * 4096 + 1          .99 / 1.0 / 1.0   .47 / .47 / .60   .92 / .92 / .91       .084 / .084 / .12
        2^24                   1.0 / 1.0 / 1.0   .75 / .64 / .63   .95 / .98 / .94       .11 / .083 / .089
        2^24 + 1               1.0 / 1.0 / 1.0   .62 / .72 / .74   .95 / .98 / .98       .099 / .11 / .12
        2^24 + 64 * 4096 + 17  1.0 / 1.0 / 1.0   .63 / .74 / .59   .91 / .93 / 1.0       .084 / .12 / .085

    Required: (a) more than half, (b) more than a tenth, (c) and (d) at least one position. At n = 4097 the second
    tile holds one element and out[4096] = (+0 + +0) + total of tile 0 is the only place where either can show: (c)
    does (fscan_model.rounding chooses its first tile so), (d) cannot, whatever the input, because +0 + (+0 + total)
    has the same bits; it is held to equality there, and from 8193 on it shows."""
    sdt = F.NP[st]
    a = F.rounding(st, n)
    want = F.scan(a, sdt)
    shares = [differing(want, variant_a(a, sdt))] + [differing(want, run_variant(v, a, sdt)) for v in (variant_b, variant_c, variant_d)]
    print("shares %s %d: a %.4f b %.4f c %.2e d %.2e" % ((st, n) + tuple(shares)))
    assert shares[0] > 0.5 and shares[1] > 0.1 and shares[2] > 0
    d = shares[3]
    if n == 4097:
        assert d == 0
    else:
        assert d > 0


@pytest.mark.parametrize("st", F.SUM_TYPES)
@pytest.mark.parametrize("n", BIG)
def test_telescoping_input_shows_a_lost_and_a_doubled_element(st, n):
    """(e) and (f) differ from the model at EVERY position behind the fault (the sums stay exact: at most 2 B)."""
    sdt = F.NP[st]
    a = F.telescoping(st, n)
    want = F.scan(a, sdt)
    heads = np.arange(F.TILE, n, F.TILE)
    heads = heads[a[heads] != 0]                             # (a fault on a zero element is no fault)
    head = int(heads[heads.size // 2])                       # the first slot of a middle tile
    mid = int(np.flatnonzero(a[:n // 2 + 1])[-1])
    e = variant_e(a, sdt, mid)
    assert F.same_bits(e[:mid + 1], want[:mid + 1]) and np.all(e[mid + 1:] != want[mid + 1:]) and mid + 1 < n
    f = variant_f(a, sdt, head)
    assert F.same_bits(f[:head], want[:head]) and np.all(f[head:] != want[head:])


# ---------------------------------------------------------------------------------------------------------------------
# specials
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("st", F.SUM_TYPES)
@pytest.mark.parametrize("n", [1, 17, 4097, 3 * 4096 + 5])
def test_specials(st, n):
    sdt = F.NP[st]
    got = F.scan(np.full(n, -0.0, sdt), sdt)
    assert np.all(got == 0) and not np.signbit(got).any()                      # all -0.0 gives all +0.0
    for a in (F.rounding(st, n), -np.abs(F.rounding(st, n)), np.full(n, np.nan, sdt), np.full(n, -np.inf, sdt)):
        first = F.scan(a, sdt)[0]
        assert first == 0 and not np.signbit(first)                            # out[0] is +0.0 for any input
    if n < 17:
        return
    a = F.telescoping(st, n)
    exact = F.scan(a, sdt)
    for i, j in ((3, n - 2), (n // 2, n // 2 + 1), (0, n - 1)) + (((4095, 4096), (100, 2 * 4096 + 1)) if n > 2 * 4096 + 2 else ()):
        b = a.copy()
        b[i], b[j] = np.inf, -np.inf                                           # +inf, later -inf: NaN behind the second
        got = F.scan(b, sdt)
        assert F.same_bits(got[:i + 1], exact[:i + 1]) and np.all(got[i + 1:j + 1] == np.inf) and np.isnan(got[j + 1:]).all()
        b = a.copy()
        b[i] = np.nan                                                          # a NaN poisons exactly what lies behind it,
        got = F.scan(b, sdt)                                                   # the later tiles through the tile sums
        assert F.same_bits(got[:i + 1], exact[:i + 1]) and np.isnan(got[i + 1:]).all()
