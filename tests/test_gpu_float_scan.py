"""Scans with a half, float or double sum type (cl_ops_amd/csrc/hip/clo_hip_fscan.hip) against tests/fscan_model.py,
the order of the kernels' additions restated in numpy: every result equals the model BIT FOR BIT (fscan_model.same_bits:
the bytes, a NaN matching a NaN), never within a tolerance. tests/test_fscan_model_cpu.py holds the model to truths
of its own and shows that the two inputs used here tell it from a scan that adds in another order (`rounding`) or that
loses or repeats an element (`telescoping`).

Shapes: the smallest at which each branch and edge of fs_scan exists (fscan_model.SIZES): inside one tile, two levels
up to exactly one full upper tile (2^24), three levels from 2^24 + 1. Entries: the Scanner object with host data and
with device data, clo_hip_scan_exclusive_typed, clo_hip_scan_exclusive_fp; the thin entries also on a workspace of
exactly the bytes they ask for, between canaries. Conversions of the element to the sum type on rounding ties, beyond
the sum type's range and from subnormals; -0, infinities and NaNs."""
import functools

import numpy as np
import pytest

import fscan_model as F

pytestmark = pytest.mark.gpu

NP = dict(F.NP, uchar=np.uint8, int=np.int32, long=np.int64, ulong=np.uint64)
SMALL = [n for n in F.SIZES if n <= 64 * 4096 + 1]
CANARY = 0xC3


def clo_type(name):
    from cl_ops_amd.api import CLO_TYPES
    return CLO_TYPES[name]


@functools.lru_cache(maxsize=2)
def modelled(kind, st, n):
    """(input, the model's scan of it), computed once and never written to."""
    a = getattr(F, kind)(st, n)
    want = F.scan(a, NP[st])
    a.flags.writeable = want.flags.writeable = False
    return a, want


def assert_same(got, want, what):
    if not F.same_bits(got, want):
        assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape)
        u = "u%d" % got.dtype.itemsize
        bad = np.flatnonzero((got.view(u) != want.view(u)) & ~(np.isnan(got) & np.isnan(want)))
        raise AssertionError("%s: %d of %d positions differ from the model, the first at %d: got %r, model %r"
                             % (what, bad.size, got.size, bad[0], got[bad[0]], want[bad[0]]))


def scanner_both_ways(gpu, a, et, st):
    """Scanner.with_host_data and Scanner.with_device_data on the same input."""
    import cl_ops_amd as clo
    ctx, q = gpu
    sdt = np.dtype(NP[st])
    sc = clo.Scanner("blelloch", ctx, et, st)
    src, dst = clo.Buffer(ctx, max(a.nbytes, 16)), clo.Buffer(ctx, max(a.size * sdt.itemsize, 16))
    try:
        host = sc.with_host_data(a, q)
        src.write(q, a)
        dst.write(q, np.full(a.size * sdt.itemsize, CANARY, np.uint8))
        sc.with_device_data(q, src, dst, a.size)
        q.finish()
        return host, dst.read(q, sdt, a.size)
    finally:
        for x in (src, dst, sc):
            x.close()


def thin(gpu, entry, a, et, st, exact_workspace=False):
    """clo_hip_scan_exclusive_typed (entry "typed") or clo_hip_scan_exclusive_fp ("fp") on device copies of `a`.
    exact_workspace: the workspace is exactly the bytes the entry asks for, in the middle of an allocation filled
    with a canary that has to be intact afterwards."""
    import cl_ops_amd as clo
    from cl_ops_amd import _hip
    ctx, q = gpu
    lib, sdt, n = _hip.lib, np.dtype(NP[st]), a.size
    if entry == "typed":
        call, sarg, wsb = lib.clo_hip_scan_exclusive_typed, clo_type(st), lib.clo_hip_scan_typed_workspace_bytes(n, clo_type(st))
    else:
        call, sarg, wsb = lib.clo_hip_scan_exclusive_fp, sdt.itemsize, lib.clo_hip_scan_fp_workspace_bytes(n, sdt.itemsize)
    assert wsb >= (-(-n // 4096) + 8) * sdt.itemsize
    margin = 4096                                                   # (a multiple of the workspace alignment)
    src, dst, ws = clo.Buffer(ctx, max(a.nbytes, 16)), clo.Buffer(ctx, max(n * sdt.itemsize, 16)), clo.Buffer(ctx, wsb + 2 * margin)
    try:
        src.write(q, a)
        dst.write(q, np.full(n * sdt.itemsize, CANARY, np.uint8))
        ws.write(q, np.full(wsb + 2 * margin, CANARY, np.uint8))
        _hip.check(call(src.ptr, dst.ptr, n, clo_type(et), sarg, ws.ptr + margin, wsb, q.stream), "clo_hip_scan_exclusive_" + entry)
        q.finish()
        if exact_workspace:
            around = ws.read(q, np.uint8, wsb + 2 * margin)
            assert np.all(around[:margin] == CANARY), "bytes below the workspace overwritten"
            assert np.all(around[margin + wsb:] == CANARY), "bytes above the workspace overwritten"
        assert np.array_equal(src.read(q, a.dtype, n).view(np.uint8), a.view(np.uint8)), "input changed"
        return dst.read(q, sdt, n)
    finally:
        for x in (src, dst, ws):
            x.close()


# ---------------------------------------------------------------------------------------------------------------------
# every shape, both inputs, the three sum types
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ["rounding", "telescoping"])
@pytest.mark.parametrize("n", F.SIZES)
@pytest.mark.parametrize("st", F.SUM_TYPES)
def test_scanner_equals_the_model(gpu, st, n, kind):
    a, want = modelled(kind, st, n)
    host, device = scanner_both_ways(gpu, a, st, st)
    assert_same(host, want, "%s %d %s, host data" % (st, n, kind))
    assert_same(device, want, "%s %d %s, device data" % (st, n, kind))


@pytest.mark.parametrize("kind", ["rounding", "telescoping"])
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("st", F.SUM_TYPES)
def test_typed_entry_equals_the_model(gpu, st, n, kind):
    a, want = modelled(kind, st, n)
    assert_same(thin(gpu, "typed", a, st, st), want, "%s %d %s" % (st, n, kind))


def fp_input(et, n):
    if et == "long":
        return np.random.default_rng([6, n]).integers(-(1 << 40), 1 << 40, n)
    return F.rounding(et, n)


@pytest.mark.parametrize("n", [4097, 64 * 4096 + 1])
@pytest.mark.parametrize("st", ["float", "double"])
@pytest.mark.parametrize("et", ["half", "float", "long"])
def test_fp_entry_equals_the_model_and_the_typed_entry(gpu, et, st, n):
    """clo_hip_scan_exclusive_fp, sum sizes 4 and 8: the numbers it computes."""
    a = fp_input(et, n)
    got = thin(gpu, "fp", a, et, st)
    assert_same(got, F.scan(a, NP[st]), "%s -> %s %d" % (et, st, n))
    assert_same(got, thin(gpu, "typed", a, et, st), "%s -> %s %d against the typed entry" % (et, st, n))


@pytest.mark.parametrize("n", [4097, (1 << 24) + 1])
@pytest.mark.parametrize("entry,st", [("typed", "half"), ("typed", "float"), ("fp", "float"), ("typed", "double"), ("fp", "double")])
def test_workspace_of_exactly_the_bytes_asked_for(gpu, entry, st, n):
    """Two and three levels of sums in a workspace of clo_hip_scan_typed_workspace_bytes (clo_hip_scan_fp_workspace_bytes)
    and not one byte more: the canary on both sides is intact and the result is the model's."""
    a, want = modelled("rounding", st, n)
    assert_same(thin(gpu, entry, a, st, st, exact_workspace=True), want, "%s %s %d" % (entry, st, n))


# ---------------------------------------------------------------------------------------------------------------------
# the conversion is the C cast, rounded to nearest, ties to even
# ---------------------------------------------------------------------------------------------------------------------

def pairs(x, n, tail=()):
    """+x[0], -x[0], +x[1], -x[1], ...: every pair cancels exactly, so every sum of the tree is +0 or one converted
    element and out[2 i + 1] is the conversion of x[i] alone. `tail`: the last elements (they need not cancel)."""
    a = np.zeros(n, x.dtype)
    m = (n - len(tail)) // 2
    a[0:2 * m:2], a[1:2 * m:2] = x[:m], -x[:m]
    if len(tail):
        a[n - len(tail):] = tail
    return a


def conversion_input(et, st, n):
    rng = np.random.default_rng([5, len(et), len(st), n])
    m = n // 2 + 1
    if (et, st) == ("ulong", "float"):            # no negatives to cancel with: out[1] and out[2] pin a tie each way
        a = rng.integers(1 << 24, 1 << 26, n, dtype=np.uint64)                 # (odd values below 2^25 are ties)
        a[:2] = (1 << 24) + 3, (1 << 24) + 1                                   # -> 2^24 + 4 (up to even), 2^24 (down to even)
        a[n - n // 8::11] |= np.uint64(1 << 63)                                # values a signed conversion would get wrong
        return a
    if (et, st) == ("long", "double"):
        x = rng.integers(1 << 53, 1 << 56, m)                                  # (odd values below 2^54 are ties)
        x[:2] = (1 << 53) + 3, (1 << 53) + 1
        return pairs(x, n)
    if (et, st) == ("double", "float"):
        x = rng.random(m) + 0.5                                                # 53 bits to round to 24
        x[::3] = 1.0 + (2 * rng.integers(0, 1 << 22, x[::3].size) + 1) * 2.0 ** -24      # ties
        x[1::3] = x[::3][:x[1::3].size] + 2.0 ** -50                           # just above a tie: up, never to even
        return pairs(x, n, tail=(3.4e38, 3.5e38, -1e39, 1.0))                  # FLT_MAX is 3.4028e38: finite, inf, -inf
    if st == "half" and et in ("double", "float"):
        x = rng.random(m) + 0.5
        x[::3] = 1.0 + (2 * rng.integers(0, 1 << 9, x[::3].size) + 1) * 2.0 ** -11       # ties
        if et == "double":                                                     # just above a tie; a conversion by way
            x[1::3] = x[::3][:x[1::3].size] + 2.0 ** -30                       # of float would see a tie here
        return pairs(x.astype(NP[et]), n, tail=(65519.996, 65520.0, -70000.0, 1.0))      # 65504, inf, -inf
    if (et, st) == ("int", "half"):
        x = rng.integers(0, 4096, m)                                           # (odd values from 2048 on are ties)
        x[:3] = 2049, 2051, 4095
        return pairs(x.astype(np.int32), n, tail=(65519, 65520, -1000003, 3))  # 65504, inf, -inf
    if (et, st) == ("uchar", "half"):
        keep = rng.random(n) < min(1.0, 30000 / (128.0 * n))                   # (the sums stay below 65504)
        return rng.integers(0, 256, n, dtype=np.uint8) * keep.astype(np.uint8)           # exact; the sums round from 2048 on
    if (et, st) == ("half", "float"):                                          # any finite half, subnormals included
        bits = rng.integers(0, 0x7c00, n, dtype=np.uint16) | (rng.integers(0, 2, n, dtype=np.uint16) << np.uint16(15))
        bits[::9] &= np.uint16(0x83ff)                                         # (exponent 0: subnormal halves)
        return bits.view(np.float16)
    raise KeyError((et, st))


@pytest.mark.parametrize("n", [4097, 64 * 4096 + 1])
@pytest.mark.parametrize("et,st", [("ulong", "float"), ("long", "double"), ("double", "float"), ("double", "half"), ("float", "half"),
                                   ("int", "half"), ("uchar", "half"), ("half", "float")])
def test_conversion_to_the_sum_type(gpu, et, st, n):
    a = conversion_input(et, st, n)
    want = F.scan(a, NP[st])
    host, device = scanner_both_ways(gpu, a, et, st)
    assert_same(host, want, "%s -> %s %d, host data" % (et, st, n))
    assert_same(device, want, "%s -> %s %d, device data" % (et, st, n))
    assert_same(thin(gpu, "typed", a, et, st), want, "%s -> %s %d, typed entry" % (et, st, n))


@pytest.mark.parametrize("st", F.SUM_TYPES)
def test_subnormal_elements_and_sums_are_kept(gpu, st):
    """The telescoping input times the smallest subnormal of the type: every element and every sum is an integer
    multiple of it below 2^11 (2^24, 2^53) of them, exact, subnormal or just above; a device that flushed
    subnormals would return zeros."""
    n = 4097
    tiny = np.nextafter(NP[st](0), NP[st](1))
    a = (F.telescoping(st, n) * tiny).astype(NP[st])
    d = F.telescoping_steps(st, n)
    want = F.scan(a, NP[st])
    assert np.array_equal(want.astype(np.longdouble), (d[:-1] - d[0]).astype(np.longdouble) * np.longdouble(tiny))
    assert np.count_nonzero(np.abs(a) < np.finfo(NP[st]).tiny) > n // 2
    host, device = scanner_both_ways(gpu, a, st, st)
    assert_same(host, want, st + ", host data")
    assert_same(device, want, st + ", device data")


# ---------------------------------------------------------------------------------------------------------------------
# -0, infinities, NaNs
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("st", ["float", "half"])
def test_specials(gpu, st):
    n, sdt = 4097, NP[st]
    run = lambda a: thin(gpu, "typed", np.ascontiguousarray(a, sdt), st, st)
    got = run(np.full(n, -0.0, sdt))
    assert not got.view(np.uint8).any(), "all -0.0 gives all +0.0"
    base = F.telescoping(st, n)
    for first in (-0.0, -3.0, np.nan, -np.inf):
        a = base.copy()
        a[0] = first
        got = run(a)
        assert got[0] == 0 and not np.signbit(got[0]), "out[0] is +0.0 whatever the first element is"
        assert_same(got, F.scan(a, sdt), "%s, first element %r" % (st, first))
    exact = F.scan(base, sdt)
    for i, j in ((3, n - 2), (100, 4095), (4095, 4096), (0, 2000)):
        a = base.copy()
        a[i], a[j] = np.inf, -np.inf
        got = run(a)
        assert_same(got, F.scan(a, sdt), "%s, +inf at %d and -inf at %d" % (st, i, j))
        assert_same(got[:i + 1], exact[:i + 1], "in front of the +inf")
        assert np.all(got[i + 1:j + 1] == np.inf) and np.isnan(got[j + 1:]).all(), (i, j)
        a = base.copy()
        a[i] = np.nan
        got = run(a)
        assert_same(got, F.scan(a, sdt), "%s, NaN at %d" % (st, i))
        assert_same(got[:i + 1], exact[:i + 1], "in front of the NaN")
        assert np.isnan(got[i + 1:]).all(), "a NaN at %d poisons everything behind it, the next tile through the tile sums" % i
