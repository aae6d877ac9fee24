"""Pins the restatements of upstream (oracle/clo_oracle.c, tests/rng_model.py, the cast of the narrower-sums GPU
test) to upstream's own kernels, executed: oracle/ref_build.py compiles the reference tree's OpenCL C for the host
and tests/ref_exec.py drives it with upstream's launch loops. CPU only. Every comparison is bit for bit unless it
says otherwise; every case is seeded.

Skips when neither oracle/_ref/ nor the reference tree exists (a checkout without the upstream tree); with the tree
present a missing library is a failure."""
import os
import re

import numpy as np
import pytest

import oracle_lib as O
import ref_exec as R
import rng_model as M
from numpy_ops import scan_cast_expected

pytestmark = pytest.mark.skipif(not R.available(), reason="no oracle/_ref and no reference tree (CLO_REFERENCE_DIR)")

U32, U64 = np.uint32, np.uint64
KIND = {"uint": O.KEY_UNSIGNED, "ulong": O.KEY_UNSIGNED, "ushort": O.KEY_UNSIGNED, "uchar": O.KEY_UNSIGNED,
        "int": O.KEY_SIGNED, "long": O.KEY_SIGNED, "float": O.KEY_FLOAT, "double": O.KEY_FLOAT}


def bits_of(a):
    return np.ascontiguousarray(a).view("u%d" % a.dtype.itemsize)


def same_bits(a, b):
    return a.dtype == b.dtype and np.array_equal(bits_of(a), bits_of(b))


def keys_of(tname, n, seed, distinct=None):
    """Seeded keys of a type over its whole range (both signs; floats with both zeros and infinities, no NaN: its
    order under upstream's `>` is undefined)."""
    rng = np.random.default_rng(seed)
    dt = np.dtype(R.NP_TYPES[tname])
    if dt.kind == "f":
        a = (rng.standard_normal(n) * 1000).astype(dt)
        special = np.array([0.0, -0.0, np.inf, -np.inf, 0.0, -0.0, 1.5, -1.5], dt)
        k = min(n, special.size)
        # among the first `distinct` values when those are all that is drawn from, anywhere otherwise
        a[rng.permutation(min(distinct, n) if distinct else n)[:k]] = special[:k]
    else:
        info = np.iinfo(dt)
        a = rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if distinct:
        a = a[rng.integers(0, min(distinct, n), n)]
    return a


def pairs_of(n, seed, key="uint", distinct=50):
    """ulong (key, index) pairs, key in the high word, at most `distinct` different keys."""
    k = keys_of(key, n, seed, distinct)
    return (bits_of(k).astype(U64) << U64(32)) | np.arange(n, dtype=U64)


PAIR_KW = {"uint": dict(key_size=4, key_shift=32), "float": dict(key_size=4, key_shift=32, key_kind=O.KEY_FLOAT)}


# ---------------------------------------------------------------------------------------------------------
# the build
# ---------------------------------------------------------------------------------------------------------

def test_every_configuration_has_a_library():
    """With the reference tree present a missing library is a failure, never a skip."""
    if R.reference_present():
        names = sorted(R._ref_build().configs())
    else:
        names = [f[len("libclo_ref_"):-3] for f in os.listdir(R.REF_DIR) if f.startswith("libclo_ref_")]
    assert len(names) >= 160
    for c in names:
        assert R.Lib.get(c).names, c


# ---------------------------------------------------------------------------------------------------------
# scan
# ---------------------------------------------------------------------------------------------------------

INT_PAIRS = [("uint", "uint"), ("uint", "ulong"), ("uchar", "uint"), ("int", "long"), ("ushort", "ushort"), ("ulong", "ulong"),
             ("uchar", "ushort"), ("ushort", "ulong"), ("ulong", "uint"), ("uint", "uchar"), ("long", "short"), ("int", "ushort"),
             ("ulong", "int")]
# (numel, lws_max, dev_max_lws, needs slack past data_out): multiples of 2*lws with one block and several blocks per
# group (numel > 2*lws^2); odd multiples of lws, whose last lws elements are the tail the first kernel skips and the
# third still adds to; one launch only; and sizes that are no multiple of lws, where upstream's third kernel runs
# gws3 - numel work-items past the end of data_out.
SCAN_SHAPES = [(128, 0, 64, False), (1024, 0, 64, False), (4096, 0, 256, False), (1 << 14, 0, 64, False), (1 << 13, 16, 256, False),
               (96, 32, 32, False), (224, 32, 32, False), (480, 32, 256, False), (64, 0, 256, False), (2, 0, 256, False),
               (100, 32, 32, True), (1000, 0, 64, True), (50, 0, 256, True)]


@pytest.mark.parametrize("types", INT_PAIRS)
def test_scan_integer_pairs_equal_the_oracle(types):
    et, st = types
    for i, (n, lws_max, dev, slack) in enumerate(SCAN_SHAPES):
        a = keys_of(et, n, 100 + i)
        got = R.scan(a, R.NP_TYPES[st], lws_max, dev, overrun_slack=slack)
        assert same_bits(got, O.blelloch(a, R.NP_TYPES[st], lws_max, dev)), (types, n, lws_max, dev)


def test_scan_skips_the_tail_like_the_oracle_says():
    """test_oracle.py's tail case, on the executed kernels: 96 elements in blocks of 64."""
    b = O.scan_bench_rand(2, U32, 96)
    got = R.scan(b, U32, 32, 32)
    assert np.array_equal(got, O.blelloch(b, U32, lws_max=32, dev_max_lws=32))
    assert np.array_equal(got[:64], O.serial_scan(b, U32)[:64]) and not np.array_equal(got[64:], O.serial_scan(b, U32)[64:])
    big = O.scan_bench_rand(1, U32, 1 << 14)                       # several blocks per group: serialised, complete
    assert np.array_equal(R.scan(big, U64, 0, 16), O.serial_scan(big, U64))


def test_scan_refuses_what_upstream_cannot_run():
    with pytest.raises(R.RefusedShape):
        R.scan(np.zeros(1, U32), U32)                               # numel / 2 = 0 work-items
    with pytest.raises(R.RefusedShape):
        R.scan(np.zeros(1000, U32), U32, 0, 64)                     # 24 elements past data_out
    with pytest.raises(R.RefusedShape):
        R.scan(np.zeros(6 * 64, U32), U32, 0, 64)                   # three work-group sums under a tree of two


@pytest.mark.parametrize("types", [("float", "uint"), ("double", "long"), ("float", "int"), ("double", "uchar"), ("float", "ulong")])
def test_scan_casts_floats_like_the_numpy_expression(types):
    """The executed kernel's float -> integer conversion against the expression the GPU test of narrower and integer
    sums uses. Values the sum type can hold after truncation (anything else is undefined in C): fractions of both
    signs everywhere, whole negative values into the signed sums."""
    et, st = types
    edt, sdt = np.dtype(R.NP_TYPES[et]), np.dtype(R.NP_TYPES[st])
    si = np.iinfo(sdt)
    hi = min(300.0, float(si.max))
    lo = -min(300.0, float(-si.min)) if si.min < 0 else -0.999
    for i, (n, dev) in enumerate([(128, 64), (1024, 64), (4096, 256), (1 << 14, 64)]):
        rng = np.random.default_rng(7 + i)
        a = (rng.random(n) * (hi - lo) * 0.999 + lo).astype(edt)
        a[:8] = np.array([0.5, -0.5, 0.999, -0.999, 1.5, 2.999, -0.0, 0.0], edt)
        if si.min < 0:
            a[8:12] = np.array([-1.5, -2.999, -1.0, -127.5], edt)
        assert a.min() < 0 and np.any(a != np.trunc(a))
        got = R.scan(a, sdt, 0, dev)
        assert same_bits(got, scan_cast_expected(a, sdt)), (types, n)
        assert same_bits(got, O.serial_scan(np.trunc(a.astype(np.float64)).astype(np.int64).astype(sdt), sdt))


@pytest.mark.parametrize("types", [("uint", "float"), ("float", "float"), ("double", "double")])
def test_scan_float_sums_within_the_bound_of_the_gpu_test(types):
    """Float sums are compared with the long double prefix sums under the bound of
    test_float_scan_matches_a_float64_reference (256 eps of the running sum of magnitudes), not bit for bit with
    HIP: the order of the additions differs by design."""
    et, st = types
    edt, sdt = np.dtype(R.NP_TYPES[et]), np.dtype(R.NP_TYPES[st])
    for i, (n, dev) in enumerate([(128, 64), (4096, 64), (1 << 14, 64)]):
        rng = np.random.default_rng(40 + i)
        a = (rng.random(n) - 0.25).astype(edt) if edt.kind == "f" else rng.integers(0, 128, n).astype(edt)
        got = R.scan(a, sdt, 0, dev)
        wide = a.astype(np.longdouble)
        exact = np.concatenate(([0.0], np.cumsum(wide)[:-1]))
        scale = np.concatenate(([0.0], np.cumsum(np.abs(wide))[:-1])) + 1.0
        err = np.abs(got.astype(np.longdouble) - exact) / scale
        assert np.all(err <= 256 * np.finfo(sdt).eps), (types, n, float(err.max() / np.finfo(sdt).eps))


# ---------------------------------------------------------------------------------------------------------
# sbitonic / abitonic
# ---------------------------------------------------------------------------------------------------------

def test_bitonic_sorts_equal_the_oracle_at_every_power_of_two():
    for t in range(1, 17):
        a = keys_of("uint", 1 << t, t)
        exp = O.sbitonic(a)
        assert same_bits(R.sbitonic(a), exp), t
        got, launches = R.abitonic(a)
        oexp, n_launches = O.abitonic(a)
        assert same_bits(got, oexp) and same_bits(got, exp) and len(launches) == n_launches, t


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("tname", ["uint", "ulong", "int", "long", "ushort", "uchar", "float", "double"])
def test_bitonic_sorts_of_every_key_type(tname, descending):
    """Whole-element keys: signed and IEEE keys compare as typed values, both directions. Bit for bit, so where +0 and
    -0 land is pinned too."""
    for t in (1, 3, 6, 10, 12):
        a = keys_of(tname, 1 << t, 50 + t)
        kw = dict(key_kind=KIND[tname], descending=descending)
        exp = O.sbitonic(a, **kw)
        assert same_bits(R.sbitonic(a, descending=descending), exp), (tname, t)
        got, launches = R.abitonic(a, descending=descending)
        oexp, n_launches = O.abitonic(a, **kw)
        assert same_bits(got, oexp) and len(launches) == n_launches, (tname, t)
        if not descending and t == 10:
            assert np.array_equal(got[1:] >= got[:-1], np.ones(got.size - 1, bool))


@pytest.mark.parametrize("descending", [False, True])
@pytest.mark.parametrize("key", ["uint", "float"])
def test_bitonic_tie_order_on_pairs(key, descending):
    """(key, index) pairs with at most 50 distinct keys (the float keys hold both zeros, which tie under `>`): the
    order of equal keys is the network's, and the oracle's is upstream's."""
    for t in (4, 8, 11, 13):
        p = pairs_of(1 << t, 70 + t, key)
        kw = dict(PAIR_KW[key], descending=descending)
        exp = O.sbitonic(p, **kw)
        assert np.unique(p >> U64(32)).size <= 50
        if key == "float" and t > 4:
            hi = p >> U64(32)
            assert np.any(hi == U64(0)) and np.any(hi == U64(0x80000000))      # both zeros are among the keys
        if t > 4:
            assert not np.array_equal(exp, O.stable_sort(p, **kw))      # the network is not stable: the order is its own
        assert np.array_equal(R.sbitonic(p, key, descending), exp), (key, t)
        got, launches = R.abitonic(p, key, descending)
        oexp, n_launches = O.abitonic(p, **kw)
        assert np.array_equal(got, oexp) and len(launches) == n_launches, (key, t)


def _kernel_names_upstream():
    """The 26 names of sort/clo_sort_abitonic.in.h where the tree is present, else those of the compiled unit."""
    if R.reference_present():
        with open(os.path.join(R._ref_build().reference_dir(), "src", "cl_ops", "sort", "clo_sort_abitonic.in.h")) as f:
            return sorted(set(re.findall(r'#define\s+CLO_SORT_ABITONIC_KNAME_\w+\s+"(abit_\w+)"', f.read())))
    return sorted(R.Lib.get("abitonic_uint_asc").names)


def test_each_abitonic_kernel_alone_against_its_oracle_family():
    """Every kernel named in upstream's header is launched once by itself, at a stage it finishes and at a later one
    (so both directions occur), on random data and on pairs, and must equal the oracle's function of the same family.
    Fails if a name of the header was never launched."""
    names = _kernel_names_upstream()
    assert len(names) == 26 and sorted(R.ABIT_KERNELS) == names
    assert sorted(R.Lib.get("abitonic_uint_asc").names) == names
    fam_no = {"any": 0, "local": 1, "priv": 2, "hyb": 3}
    del R.LAUNCHES[:]
    for name in names:
        fam, K, S, V = R.abit_parse(name)
        for data, key, kw in ((None, None, {}), ("pairs", "uint", PAIR_KW["uint"])):
            if fam in ("any", "priv"):
                n, lws, first = 1 << 10, 64, 7                      # the step these start from
            else:
                lws = max(1 << (K - S), 4)
                n, first = lws * V * 4, K
            gws = n // V
            for stage in (first, first + 1):
                a = pairs_of(n, K + S, "uint") if data else keys_of("uint", n, K + S)
                buf = R.Buf(a)
                R.abit_kernel(R.Lib.get(R.sort_config("abitonic", a, key)), name, buf, stage, first, gws, lws)
                exp = O.abit_kernel(a, fam_no[fam], stage, first, S, lws, **kw)
                assert np.array_equal(buf.a, exp), (name, stage, data)
                assert not np.array_equal(exp, a)
    launched = {k for c, k, _, _ in R.LAUNCHES}
    assert launched == set(names), set(names) - launched


ABIT_OPTS = [dict(), dict(maxps=1), dict(maxps=2), dict(maxps=3), dict(minps=2), dict(minps=3, maxps=3), dict(minps=4),
             dict(maxsfs=0), dict(maxsfs=5), dict(maxsfs=1, maxps=3), dict(lws_max=16), dict(lws_max=8, maxps=2),
             dict(dev_max_lws=1024), dict(dev_max_lws=1024, minps=2, maxps=2), dict(dev_max_lws=1024, maxps=1),
             dict(dev_max_lws=2048, maxps=1), dict(dev_max_lws=1024, maxps=3, minps=3)]


@pytest.mark.parametrize("opts", ABIT_OPTS)
def test_abitonic_strategy_and_launch_list(opts):
    """Which kernel does which steps: the driver's strategy table launches the same number of kernels as the oracle's
    and, kernel by kernel executed, gives the oracle's bits on pairs (a wrong step split would change the tie order)."""
    used = set()
    for t in (3, 9, 13):
        p = pairs_of(1 << t, 90 + t, "uint")
        got, launches = R.abitonic(p, "uint", **opts)
        oexp, n_launches = O.abitonic(p, key_size=4, key_shift=32, **opts)
        assert len(launches) == n_launches and np.array_equal(got, oexp), (opts, t)
        assert np.array_equal(got, O.sbitonic(p, key_size=4, key_shift=32))
        used |= {k for k, _, _ in launches}
    assert "abit_any" in used


def test_abitonic_strategies_reach_every_kernel_family_member():
    """Over the option sets above every one of the 26 kernels takes part in a whole sort too."""
    used = set()
    for opts in ABIT_OPTS:
        used |= {s["kernel"] for s in R.abitonic_strategy(1 << 13, **opts)}
    assert used == set(R.ABIT_KERNELS), set(R.ABIT_KERNELS) - used


def test_bitonic_refuses_other_than_powers_of_two():
    for f in (R.sbitonic, R.abitonic):
        with pytest.raises(R.RefusedShape):
            f(np.zeros(1000, U32))


# ---------------------------------------------------------------------------------------------------------
# gselect
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("descending", [False, True])
def test_gselect_equals_the_oracle(descending):
    for n in (1, 17, 256, 1000):
        for tname in ("uint", "int", "long", "float", "double", "uchar", "ushort", "ulong"):
            a = keys_of(tname, n, n + len(tname), distinct=40 if n > 100 else None)
            exp = O.gselect(a, key_kind=KIND[tname], descending=descending)
            assert same_bits(R.gselect(a, descending=descending), exp), (tname, n)
        for key in ("uint", "float"):
            p = pairs_of(n, n, key, distinct=9)
            exp = O.gselect(p, descending=descending, **PAIR_KW[key])
            assert np.array_equal(R.gselect(p, key, descending), exp), (key, n)
            assert np.array_equal(exp, O.stable_sort(p, descending=descending, **PAIR_KW[key]))     # +0 and -0 tie: by index


# ---------------------------------------------------------------------------------------------------------
# satradix
# ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("radix", [2, 4, 8, 16, 32, 64, 128, 256])
def test_satradix_of_uint_keys_every_radix(radix):
    """Radix 8 / 32 / 64 / 128 leave the top 32 % bits of a 32-bit key unsorted (total_digits rounds down): executed
    upstream says so too. That is test_satradix_radix_8_is_partial_upstream's premise."""
    bits = R.tzc(radix)
    for n, dev in ((256, 64), (1024, 256)):
        a = keys_of("uint", n, radix + n)
        got = R.satradix(a, radix=radix, dev_max_lws=dev)
        assert np.array_equal(got, O.satradix(a, radix=radix, dev_max_lws=dev)), (radix, n)
        sorted_bits = (32 // bits) * bits
        mask = U32((1 << sorted_bits) - 1)
        assert np.array_equal(got, a[np.argsort(a & mask, kind="stable")])
        assert (sorted_bits == 32) == np.array_equal(got, np.sort(a)), radix


@pytest.mark.parametrize("tname", ["int", "long", "ushort", "uchar", "ulong"])
def test_satradix_of_other_key_types(tname):
    """Signed keys: the digits are those of the raw bits, so the negative keys stay after the positive ones
    (SURVEY §8a-6 iii). 64-bit keys take twice the passes."""
    for radix, n, dev in ((16, 512, 64), (256, 512, 256), (8, 256, 64)):
        a = keys_of(tname, n, radix + len(tname))
        got = R.satradix(a, radix=radix, dev_max_lws=dev)
        assert same_bits(got, O.satradix(a, radix=radix, dev_max_lws=dev, key_kind=KIND[tname])), (tname, radix)
        if radix != 8:
            assert np.array_equal(bits_of(got), np.sort(bits_of(a)))
            if KIND[tname] == O.KEY_SIGNED:
                neg = np.flatnonzero(got < 0)
                assert 0 < neg.size < n and neg[0] == n - neg.size and np.all(got[:neg[0]] >= 0)
    pos = np.abs(keys_of(tname, 256, 5) >> 1) if KIND[tname] == O.KEY_SIGNED else keys_of(tname, 256, 5)
    assert np.array_equal(R.satradix(pos, dev_max_lws=64), np.sort(pos))


def test_satradix_pairs_with_the_key_in_the_high_word():
    """Upstream counts the digits of the element, not of the key: on (uint key, index) pairs it makes 64 / bits passes,
    and the passes past bit 31 see the same digits again (OpenCL C reduces the shift count modulo 32). Harmless
    while 32 % bits == 0; refused otherwise (see ref_exec.satradix)."""
    for radix, n in ((16, 512), (4, 256), (256, 1024), (2, 256)):
        for distinct in (50, None):
            p = pairs_of(n, radix, "uint", distinct=distinct)
            got = R.satradix(p, "uint", radix=radix, dev_max_lws=64)
            assert np.array_equal(got, O.satradix(p, radix=radix, dev_max_lws=64, key_size=4, key_shift=32)), radix
            assert np.array_equal(got, O.stable_sort(p, key_size=4, key_shift=32))
    for radix in (8, 32, 64, 128):
        with pytest.raises(R.RefusedShape):
            R.satradix(pairs_of(256, 1), "uint", radix=radix, dev_max_lws=64)


@pytest.mark.parametrize("radix,n,lws", [(16, 1024, 64), (4, 256, 16), (256, 1024, 256), (8, 512, 32)])
def test_satradix_aux_arrays_of_one_pass(radix, n, lws):
    """offsets (with the back-filled gaps), counters (digit-major) and their scan, after the first digit pass."""
    for a in (keys_of("uint", n, radix), np.where(np.arange(n) % 3 == 0, 0x11111111, 0xEEEEEEEE).astype(U32),
              np.full(n, 0x33333333, U32), (keys_of("uint", n, 3) | U32(radix - 1))):
        got = R.satradix(a, radix=radix, lws_max=lws, dev_max_lws=lws, debug=True)
        exp = O.satradix(a, radix=radix, lws_max=lws, dev_max_lws=lws, debug=True)
        for g, e, what in zip(got, exp, ("sorted", "offsets", "counters", "counters_sum")):
            assert np.array_equal(g, e), (what, radix)


def test_satradix_refuses_what_upstream_cannot_run():
    with pytest.raises(R.RefusedShape):
        R.satradix(np.zeros(1000, U32))
    with pytest.raises(R.RefusedShape):
        R.satradix(np.zeros(8, U32), radix=16)


# ---------------------------------------------------------------------------------------------------------
# RNG
# ---------------------------------------------------------------------------------------------------------

MAIN_SEEDS = [0, 1, 12345, (1 << 32) + 7, (1 << 63) + 11, (1 << 64) - 1]


def state_bytes(st):
    return np.ascontiguousarray(st).view(np.uint8).reshape(-1)


@pytest.mark.parametrize("name", M.NAMES)
def test_rng_seeding_kernels(name):
    """clo_rng_init for every hash and main seed == dev_gid_states; without a hash it is clo_ulong2statetype of
    gid + main_seed, which pins ulong2state."""
    for ms in MAIN_SEEDS:
        for h in (None, "KNUTH(x)", "XS1(x)"):
            got = R.rng_dev_gid_seeds(name, 96, ms, h)
            assert np.array_equal(got, state_bytes(M.dev_gid_states(name, 96, ms, h))), (name, ms, h)
        with np.errstate(over="ignore"):
            seeds = np.arange(96, dtype=U64) + U64(ms)
        assert np.array_equal(R.rng_dev_gid_seeds(name, 96, ms), state_bytes(M.ulong2state(name, seeds)))


@pytest.mark.parametrize("name", M.NAMES)
def test_rng_streams(name):
    """64 states x 256 draws from kernel-made seeds of several main seeds and every hash, and from arbitrary state
    bytes (zero and negative states among them): outputs and final states == fill; one launch == step."""
    S = 64
    starts = [R.rng_dev_gid_seeds(name, S, ms, h) for ms, h in zip(MAIN_SEEDS, [None, "KNUTH(x)", "XS1(x)", None, "KNUTH(x)", "XS1(x)"])]
    raw = np.random.default_rng(11).integers(0, 256, S * M.SEED_SIZE[name], dtype=np.uint8)
    raw[:M.SEED_SIZE[name]] = 0
    raw[M.SEED_SIZE[name]:2 * M.SEED_SIZE[name]] = 0xFF
    starts.append(raw)
    for i, sb in enumerate(starts):
        st = M.state_from_bytes(name, sb, S)
        out, fin = R.rng_bench(name, sb, 256)
        exp, efin = M.fill(name, st, S * 256)
        assert np.array_equal(out.reshape(-1), exp) and np.array_equal(fin, state_bytes(efin)), (name, i)
        one, fin1 = R.rng_bench(name, sb, 1)
        ns, x = M.step(name, st)
        assert np.array_equal(one[0], x) and np.array_equal(fin1, state_bytes(ns)), (name, i)


@pytest.mark.parametrize("name", M.NAMES)
def test_rng_bits_and_maxint(name):
    sb = R.rng_dev_gid_seeds(name, 64, 99, "KNUTH(x)")
    st = M.state_from_bytes(name, sb, 64)
    for bits in (1, 8, 31, 32):
        out, fin = R.rng_bench(name, sb, 64, bits=bits)
        exp, efin = M.fill(name, st, 64 * 64, bits)
        assert np.array_equal(out.reshape(-1), exp) and np.array_equal(fin, state_bytes(efin)), (name, bits)
        assert bits == 32 or int(out.max()) < (1 << bits)
    for maxint in (1 << 10, 1000, 1, (1 << 31) + 1):
        out, fin = R.rng_bench(name, sb, 64, maxint=maxint)
        exp, efin = M.fill(name, st, 64 * 64, 32, maxint)
        assert np.array_equal(out.reshape(-1), exp) and np.array_equal(fin, state_bytes(efin)), (name, maxint)
        assert int(out.max()) < maxint


# ---------------------------------------------------------------------------------------------------------
# the harness itself
# ---------------------------------------------------------------------------------------------------------

def test_canaries_are_checked_and_would_notice():
    a = keys_of("uint", 256, 1)
    for run in (lambda: R.sbitonic(a), lambda: R.abitonic(a), lambda: R.gselect(a), lambda: R.satradix(a, dev_max_lws=64),
                lambda: R.scan(a, U64, 0, 64), lambda: R.rng_bench("lcg", R.rng_dev_gid_seeds("lcg", 64), 2)):
        checks, launches = R.CANARY_CHECKS[0], len(R.LAUNCHES)
        run()
        # both margins of at least one buffer after every launch
        assert len(R.LAUNCHES) > launches and R.CANARY_CHECKS[0] - checks >= 2 * (len(R.LAUNCHES) - launches)
    b = R.Buf(a)
    b.check()
    b.raw[R.MARGIN + b.nbytes] ^= 1                                  # the first byte past the end
    with pytest.raises(R.CanaryError):
        b.check()
    b = R.Buf(a)
    b.raw[R.MARGIN - 1] = 0                                          # the last byte before the start
    with pytest.raises(R.CanaryError):
        b.check()


def test_a_rerun_gives_identical_bytes():
    a, p = keys_of("uint", 1024, 2), pairs_of(1024, 2)
    f = keys_of("float", 1024, 3)
    runs = [lambda: R.sbitonic(p, "uint"), lambda: R.abitonic(p, "uint")[0], lambda: R.gselect(p, "uint"),
            lambda: R.satradix(p, "uint", dev_max_lws=64), lambda: R.satradix(a, radix=8, dev_max_lws=64),
            lambda: R.scan(a, U64, 0, 64), lambda: R.scan(f, np.float32, 0, 64), lambda: R.scan(a[:1000], U32, 0, 64, overrun_slack=True),
            lambda: R.rng_bench("tauslcg", R.rng_dev_gid_seeds("tauslcg", 64, 5, "XS1(x)"), 16)[0]]
    for i, run in enumerate(runs):
        assert same_bits(run(), run()), i


# ---------------------------------------------------------------------------------------------------------
# the committed vectors of tests/golden/sortscan_golden.npz
# ---------------------------------------------------------------------------------------------------------

def test_sortscan_golden_equals_executed_upstream():
    """Every expected output of sortscan_golden.npz that upstream can compute (powers of two for the bitonic and
    radix sorts, numel >= radix) equals what upstream's kernels give. Not compared: the radix sort of the typed
    vectors (upstream's digits order raw bits; DESIGN §1 keeps numeric order) and satradix on 1, 17 and 1000 pairs."""
    G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sortscan_golden.npz"))
    checked = 0
    for name in G.files:
        tag = name[:-3]
        if name.startswith("sort_") and name.endswith("_in"):
            a, exp = G[name], G[tag + "_out"]
            assert np.array_equal(R.sbitonic(a), exp) and np.array_equal(R.abitonic(a)[0], exp), name
            assert np.array_equal(R.satradix(a, dev_max_lws=64), exp), name
            checked += 3
            if a.size <= 1024:
                assert np.array_equal(R.gselect(a), exp), name
                checked += 1
        elif name.startswith("pairs_") and name.endswith("_in"):
            a = G[name]
            assert np.array_equal(R.satradix(a, "uint", dev_max_lws=64), G[tag + "_out"]), name
            assert np.array_equal(R.sbitonic(a, "uint"), G[tag + "_bitonic_out"]), name
            assert np.array_equal(R.abitonic(a, "uint")[0], G[tag + "_bitonic_out"]), name
            checked += 3
        elif name.startswith("gselect_pairs_") and name.endswith("_in"):
            assert np.array_equal(R.gselect(G[name], "uint"), G[tag + "_out"]), name
            checked += 1
        elif name.startswith("typed_") and name.endswith("_in"):
            a, exp = G[name], G[tag + "_out"]
            for got in (R.sbitonic(a), R.abitonic(a)[0], R.gselect(a)):
                assert np.array_equal(got, exp), name                # as values: the vectors hold both zeros
                checked += 1
        elif name.startswith("scan_") and name.endswith("_in"):
            a = G[name]
            if tag.startswith("scan_wrap"):
                assert np.array_equal(R.scan(a, U32, 0, 64), G[tag + "_out"]), name
                checked += 1
            else:
                n = tag.split("_")[1]
                for sdt, t in ((U32, "u32"), (U64, "u64")):
                    assert np.array_equal(R.scan(a, sdt, 0, min(64, max(a.size // 2, 1))), G["scan_%s_%s_out" % (t, n)]), name
                    checked += 1
    srt, offs, cnt, cs = R.satradix(G["structural_in"], radix=16, lws_max=64, dev_max_lws=64, debug=True)
    for got, what in ((srt, "out"), (offs, "offsets"), (cnt, "counters"), (cs, "counters_sum")):
        assert np.array_equal(got, G["structural_" + what]), what
    assert checked >= 140
