"""The public sorts, scans and RNG fill on device views that are aligned only to their element size (what a torch
slice such as t[3:] hands over): every input and output lies at a byte offset inside a larger allocation with 256
guard bytes of a canary pattern on each side. After every call the output equals a plain reference bit for bit, no
guard byte has changed, and an out-of-place call has left its input as it was. Offsets of es and 16 - es bytes (and 7
/ 9 elements of 1 byte, 6 / 10 bytes of 2) on the input alone, the output alone, both at different offsets, and in
place; sizes on every path of the radix sort (one launch, single sweep, chain-free passes on small and on big tiles,
the digit stream on and off, radix 2 .. 256, odd pass counts in place, key fields, a run-time compiled get_key), the
by-key sort (pack / unpack and fused first and last passes, argsort, no keys_out, in place), both tile shapes of the
integer scan, the floating-point scans, clo_hip_reduce_sum, the bitonic sorts and gselect, the six RNGs into torch
slices, and clo_hip_radix_sort_fed with its first digits at every byte offset. Also: every C-ABI entry that takes a
workspace or a device uint64 word refuses a misaligned one with CLO_HIP_EARGS."""
import ctypes as C

import numpy as np
import pytest

import rng_model as M

pytestmark = pytest.mark.gpu

G = 256                                   # guard bytes on each side of a view
_PAT = [((np.arange(251 * 16) * 167 + 41 * k) % 251).astype(np.uint8) ^ np.uint8(0xA5) for k in range(3)]
_NP = {"uchar": np.uint8, "char": np.int8, "ushort": np.uint16, "short": np.int16, "uint": np.uint32, "int": np.int32,
       "ulong": np.uint64, "long": np.int64, "half": np.float16, "float": np.float32, "double": np.float64}
_INT = {2: np.int16, 4: np.int32, 8: np.int64}


def offsets(es):
    """Byte offsets of a view: es and 16 - es; for 1- and 2-byte elements also two odd multiples around 8 bytes."""
    return {1: [1, 15, 7, 9], 2: [2, 14, 6, 10], 4: [4, 12], 8: [8]}[es]


def configs(es, full=True):
    """(input offset, output offset or None for in place): input alone, output alone, both, in place."""
    o = offsets(es)
    if not full:
        return [(o[-1], 0), (0, o[0]), (o[0], None)]
    c = [(x, 0) for x in o] + [(0, x) for x in o] + [(x, None) for x in o]
    return c + ([(o[0], o[1])] if len(o) > 1 else [(o[0], 16 - o[0] if o[0] != 8 else 24)])


@pytest.fixture(scope="module")
def dev():
    import cl_ops_amd as clo
    ctx = clo.Context(0)
    q = clo.Queue(ctx)
    yield clo, ctx, q
    q.close()
    ctx.close()


class Region:
    """An owned allocation of nbytes + 2 G bytes filled with a canary pattern (and `data` at the view), and a view
    of nbytes at byte G + off of it."""

    def __init__(self, dev, nbytes, off, data=None, salt=0):
        clo, ctx, self.q = dev
        self.n, self.at = nbytes, G + off
        self.host = np.resize(_PAT[salt], nbytes + 2 * G)
        if data is not None:
            self.host[self.at:self.at + nbytes] = np.ascontiguousarray(data).view(np.uint8)
        self.base = clo.Buffer(ctx, nbytes + 2 * G)
        self.base.write(self.q, self.host)
        self.view = clo.Buffer(ctx, nbytes, device_ptr=self.base.ptr + self.at)

    @property
    def ptr(self):
        return self.base.ptr + self.at

    def check(self, want=None, what=""):
        """The guards are intact and the view holds `want` (bytes of an array; None: what it held at the start)."""
        got = self.base.read(self.q, np.uint8, self.n + 2 * G)
        lo, hi = got[:self.at], got[self.at + self.n:]
        assert np.array_equal(lo, self.host[:self.at]), "guard below the view overwritten " + what
        assert np.array_equal(hi, self.host[self.at + self.n:]), "guard above the view overwritten " + what
        exp = self.host[self.at:self.at + self.n] if want is None else np.ascontiguousarray(want).view(np.uint8)
        view = got[self.at:self.at + self.n]
        if not np.array_equal(view, exp):
            bad = np.flatnonzero(view != exp)
            raise AssertionError("view differs at %d of %d bytes, first at byte %d %s" % (bad.size, self.n, bad[0], what))
        return view

    def close(self):
        self.view.close()     # (the wrapper before the memory it wraps)
        self.base.close()


def random_bits(dt, n, seed, specials=True):
    dt = np.dtype(dt)
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 63, n, dtype=np.uint64) ^ (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    a = a.astype({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize]).view(dt)
    if specials and dt.kind == "f" and n:      # -0, +0, infinities and NaNs of both signs with payloads
        sp = {2: [0, 0x8000, 0x7c00, 0xfc00, 0x7e01, 0xfe02],
              4: [0, 0x80000000, 0x7f800000, 0xff800000, 0x7fc00001, 0xffc00002],
              8: [0, 1 << 63, 0x7ff0 << 48, 0xfff0 << 48, (0x7ff8 << 48) | 1, (0xfff8 << 48) | 2]}[dt.itemsize]
        bits = np.array(sp, dtype=np.uint64).astype({2: np.uint16, 4: np.uint32, 8: np.uint64}[dt.itemsize])
        a[::13] = np.resize(bits.view(dt), a[::13].shape)
    return a


def sort_order(a, key=None):
    """The radix sort's stable order: unsigned by bits, signed numerically, floating point in IEEE total order
    (-NaN < -inf < ... < -0 < +0 < ... < +inf < +NaN)."""
    if key is not None:
        return np.argsort(key, kind="stable")
    if a.dtype.kind == "f":
        x = a.view(_INT[a.itemsize]).astype(np.int64)
        mx = (1 << (8 * a.itemsize - 1)) - 1
        return np.argsort(np.where(x < 0, ~(x & mx), x), kind="stable")
    return np.argsort(a, kind="stable")


def run_sort(dev, s, a, want, cfgs, what=""):
    """Sorter.with_device_data under every (input offset, output offset / None = in place) of cfgs."""
    clo, ctx, q = dev
    for io, oo in cfgs:
        tag = "%s in@%s out@%s" % (what, io, "in place" if oo is None else oo)
        src = Region(dev, a.nbytes, io, a, salt=1)
        if oo is None:
            s.with_device_data(q, src.view, None, a.size)
            q.finish()
            src.check(want, tag)
        else:
            dst = Region(dev, a.nbytes, oo, salt=2)
            s.with_device_data(q, src.view, dst.view, a.size)
            q.finish()
            dst.check(want, tag)
            src.check(None, tag + " (input)")
            dst.close()
        src.close()


# ---------------------------------------------------------------------------------------------------------------------
# satradix: plain sorts
# ---------------------------------------------------------------------------------------------------------------------

# (element type, n, CLO_RADIX_SWEEP or None, radix, all offset configurations?): one launch, the single sweep (the
# library's choice and forced), chain-free small tiles (above the sweep range and forced)
_SORT = [(t, n, None, 16, True) for t in ("uchar", "ushort") for n in (5000, 70001)]
_SORT += [(t, n, None, 16, True) for t in ("int", "uint", "float") for n in (12345, 70001, (1 << 21) + 3)]
_SORT += [(t, n, None, 16, True) for t in ("ulong", "double") for n in (8191, 70001, (1 << 20) + 3)]
_SORT += [("uint", (1 << 21) + 3, "1", 16, False), ("uint", 70001, "0", 16, False), ("ulong", 70001, "0", 16, False),
          ("ulong", (1 << 20) + 3, "1", 16, False)]
_SORT += [("uint", n, None, r, False) for n in (5000, 70001) for r in (2, 64, 256)]
_SORT += [("ulong", 70001, None, 256, False), ("double", (1 << 20) + 3, None, 256, False)]


@pytest.mark.parametrize("etype,n,sweep,radix,full", _SORT)
def test_sort(dev, monkeypatch, etype, n, sweep, radix, full):
    clo, ctx, q = dev
    if sweep is not None:
        monkeypatch.setenv("CLO_RADIX_SWEEP", sweep)      # (read when the sorter is made)
    a = random_bits(_NP[etype], n, n + radix)
    want = a[sort_order(a)]
    s = clo.Sorter("satradix", ctx, etype, options="radix=%d" % radix)
    run_sort(dev, s, a, want, configs(a.itemsize, full), etype)
    s.close()


@pytest.mark.parametrize("etype,radix,n", [("uint", 128, 70001), ("uint", 128, (1 << 21) + 3), ("uchar", 256, 70001),
                                           ("ushort", 8, 70001), ("ushort", 8, 3000)])
def test_sort_odd_pass_count_in_place(dev, etype, radix, n):
    """An odd number of passes in place ends in tmp and is copied back (uint radix 128: 5 passes of 7 bits; uchar
    radix 256: one; ushort radix 8: 3 passes of 6 bits)."""
    clo, ctx, q = dev
    a = random_bits(_NP[etype], n, 3)
    s = clo.Sorter("satradix", ctx, etype, options="radix=%d" % radix)
    run_sort(dev, s, a, a[sort_order(a)], [(x, None) for x in offsets(a.itemsize)] + [(offsets(a.itemsize)[0], 0)])
    s.close()


@pytest.mark.parametrize("etype,key_type,get_key,n", [
    ("uint", None, "((x) >> 8) & 0xfff", 70001), ("uint", None, "((x) >> 8) & 0xfff", 5000),
    ("ulong", "uint", "(uint) ((x) >> 32)", (1 << 20) + 3), ("ushort", None, "((x) >> 4) & 0xff", 30000)])
def test_sort_key_field(dev, etype, key_type, get_key, n):
    clo, ctx, q = dev
    a = random_bits(_NP[etype], n, 5)
    dt = a.dtype.type
    if etype == "ulong":
        a &= dt((1 << 42) - 1)                          # (equal keys with other low words: stability shows)
        key = a >> dt(32)
    else:
        sh, mask = (8, 0xfff) if etype == "uint" else (4, 0xff)
        key = (a >> dt(sh)) & dt(mask)
    s = clo.Sorter("satradix", ctx, etype, key_type=key_type, get_key=get_key)
    run_sort(dev, s, a, a[sort_order(a, key)], configs(a.itemsize), get_key)
    s.close()


def test_sort_run_time_compiled_get_key(dev):
    """A get_key outside the parsed family: the key extract and gather kernels, compiled with hiprtc, read and
    write the views."""
    clo, ctx, q = dev
    a = random_bits(np.uint32, 70001, 9)
    s = clo.Sorter("satradix", ctx, "uint", get_key="((x) / 65536)")
    run_sort(dev, s, a, a[sort_order(a, a // 65536)], configs(4), "jit")
    s.close()


@pytest.mark.parametrize("etype,n,no_digits", [("uint", (1 << 26) + 4099, None), ("ulong", (1 << 22) + 77, None),
                                               ("ulong", (1 << 22) + 77, "1")])
def test_sort_big_tiles(dev, monkeypatch, etype, n, no_digits):
    """Big tiles, with the digit stream between the passes and (CLO_RADIX_NO_DIGITS=1) without; against
    torch.sort on the device."""
    import torch
    clo, ctx, q = dev
    if no_digits:
        monkeypatch.setenv("CLO_RADIX_NO_DIGITS", no_digits)
    a = random_bits(_NP[etype], n, 11)
    t = torch.from_numpy(a.view(np.int64) if etype == "ulong" else a.astype(np.int64)).cuda()
    if etype == "ulong":                                # (unsigned order: flip the sign bit, sort as int64)
        t = t ^ torch.tensor(-(1 << 63), dtype=torch.int64, device="cuda")
    want = torch.sort(t, stable=True).values
    if etype == "ulong":
        want = want ^ torch.tensor(-(1 << 63), dtype=torch.int64, device="cuda")
    want = want.cpu().numpy().view(np.uint64) if etype == "ulong" else want.cpu().numpy().astype(np.uint32)
    del t
    s = clo.Sorter("satradix", ctx, etype)
    es = a.itemsize
    run_sort(dev, s, a, want, [(es, 16 - es if es == 4 else 24), (es, None)], etype)
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# satradix: by key
# ---------------------------------------------------------------------------------------------------------------------

_KV_REF = {}


def _kv_data(etype, n):
    if (etype, n) not in _KV_REF:
        keys = random_bits(_NP[etype], n, 17 + n)
        values = np.random.default_rng(n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        _KV_REF[(etype, n)] = (keys, values, sort_order(keys))
    return _KV_REF[(etype, n)]


def run_by_key(dev, s, data, ki_off, vi_off, ko, vo, with_values=True, keys_out=True, inplace=False, what=""):
    """One by-key sort with keys_in, values_in, keys_out, values_out at the given byte offsets."""
    clo, ctx, q = dev
    keys, values, order = data
    n = keys.size
    tag = "%s keys_in@%s values_in@%s keys_out@%s values_out@%s%s" % (what, ki_off, vi_off, ko, vo, " in place" if inplace else "")
    kin = Region(dev, keys.nbytes, ki_off, keys, salt=1)
    vin = Region(dev, 4 * n, vi_off, values, salt=2) if with_values else None
    want_v = values[order] if with_values else order.astype(np.uint32)
    if inplace:
        s.by_key_with_device_data(q, kin.view, vin.view, kin.view, vin.view, n)
        q.finish()
        kin.check(keys[order], tag)
        vin.check(want_v, tag)
        kin.close()
        vin.close()
        return
    kout = Region(dev, keys.nbytes, ko, salt=0) if keys_out else None
    vout = Region(dev, 4 * n, vo, salt=0)
    s.by_key_with_device_data(q, kin.view, vin.view if vin else None, kout.view if kout else None, vout.view, n)
    q.finish()
    vout.check(want_v, tag)
    if kout:
        kout.check(keys[order], tag)
    kin.check(None, tag + " (keys in)")
    if vin:
        vin.check(None, tag + " (values in)")
    for r in (kin, vin, kout, vout):
        if r:
            r.close()


# pack / unpack around the pair sort (one launch, the sweep range, radix 4 and 32 on the chain-free passes) and the
# fused first and last passes (chain-free small tiles above 2^20 pairs, big tiles from 2^22)
_KV = [(t, n, 16) for t in ("uchar", "short", "uint", "float") for n in (5000, 70001, (1 << 20) + 3)]
_KV += [("uint", (1 << 20) + 3, 4), ("short", (1 << 20) + 3, 32), ("uint", (1 << 22) + 1, 16), ("float", (1 << 22) + 1, 256)]


@pytest.mark.parametrize("etype,n,radix", _KV)
def test_by_key(dev, etype, n, radix):
    clo, ctx, q = dev
    data = _kv_data(etype, n)
    s = clo.Sorter("satradix", ctx, etype, options="radix=%d" % radix)
    o, o4 = offsets(data[0].itemsize), offsets(4)
    run_by_key(dev, s, data, o[0], 0, 0, 0, what=etype)            # each array offset on its own
    run_by_key(dev, s, data, 0, o4[-1], 0, 0, what=etype)
    run_by_key(dev, s, data, 0, 0, o[-1], 0, what=etype)
    run_by_key(dev, s, data, 0, 0, 0, o4[0], what=etype)
    run_by_key(dev, s, data, o[0], o4[-1], o[-1], o4[0], what=etype)   # all four
    run_by_key(dev, s, data, o[-1], 0, o[0], o4[-1], with_values=False, what=etype + " argsort")
    run_by_key(dev, s, data, o[-1], o4[-1], None, o4[0], keys_out=False, what=etype + " no keys_out")
    run_by_key(dev, s, data, o[-1], o4[0], None, None, inplace=True, what=etype)
    s.close()


def test_by_key_one_pass_in_place_above_2_20(dev):
    """uchar keys, radix 256: one pass; in place it writes the pairs and the unpack kernel splits them."""
    clo, ctx, q = dev
    data = _kv_data("uchar", (1 << 20) + 3)
    s = clo.Sorter("satradix", ctx, "uchar", options="radix=256")
    for ki, vi in ((1, 4), (15, 12), (7, 8)):
        run_by_key(dev, s, data, ki, vi, None, None, inplace=True, what="uchar radix 256")
    run_by_key(dev, s, data, 7, 4, 9, 12, what="uchar radix 256")
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# scans
# ---------------------------------------------------------------------------------------------------------------------

def scan_input(et, n, seed):
    dt = np.dtype(_NP[et])
    rng = np.random.default_rng(seed)
    if dt.kind == "f":
        return (rng.random(n) - 0.25).astype(dt)
    info = np.iinfo(dt)                                  # full range: the 64-bit sums carry into their high half
    return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)


def run_scan(dev, sc, a, sdt, cfgs, want):
    """want: the expected output, or a function that asserts on it (called with the output and a tag)."""
    clo, ctx, q = dev
    n = a.size
    for io, oo in cfgs:
        tag = "in@%s out@%s" % (io, oo)
        src = Region(dev, a.nbytes, io, a, salt=1)
        dst = Region(dev, n * sdt.itemsize, oo, salt=2)
        sc.with_device_data(q, src.view, dst.view, n)
        q.finish()
        if callable(want):
            got = dst.base.read(q, np.uint8, dst.n, offset=dst.at)
            want(got.view(sdt), tag)
            dst.check(got, tag)
        else:
            dst.check(want, tag)
        src.check(None, tag + " (input)")
        src.close()
        dst.close()


def scan_configs(es_in, es_out, full):
    oi, oo = offsets(es_in), offsets(es_out)
    if not full:
        return [(oi[-1], 0), (0, oo[0]), (oi[0], oo[-1])]
    return [(x, 0) for x in oi] + [(0, x) for x in oo] + [(oi[0], oo[-1]), (oi[-1], oo[0])]


@pytest.mark.parametrize("et,st", [("uint", "uint"), ("uint", "ulong"), ("uchar", "uint"), ("int", "long"), ("ushort", "ulong")])
@pytest.mark.parametrize("n", [100003, (1 << 21) + 5])
def test_scan(dev, et, st, n):
    """Both tile shapes of the look-back scan (below 2^21 elements and from there on) against int64 prefix sums
    that wrap in the sum type."""
    clo, ctx, q = dev
    a = scan_input(et, n, n + len(et))
    sdt = np.dtype(_NP[st])
    wide = a.astype(np.int64).view(np.uint64)
    want = np.concatenate((np.zeros(1, np.uint64), np.cumsum(wide[:-1], dtype=np.uint64))).astype(sdt.str.replace("i", "u")).view(sdt)
    sc = clo.Scanner("blelloch", ctx, et, st)
    run_scan(dev, sc, a, sdt, scan_configs(a.itemsize, sdt.itemsize, True), want)
    sc.close()


@pytest.mark.parametrize("et,st", [("float", "float"), ("half", "float"), ("double", "double")])
@pytest.mark.parametrize("n", [100003, (1 << 21) + 5])
def test_float_scan(dev, et, st, n):
    """Floating-point sums: equal to the exact prefix sums to rounding (closeness to upstream), bit-identical to the
    same scan on 256-byte aligned arrays, and that one bit-identical to tests/fscan_model.py (the order of the
    additions depends on the layout of the tiles alone, and is the one the kernel file states)."""
    import fscan_model
    clo, ctx, q = dev
    a = scan_input(et, n, 7)
    sdt = np.dtype(_NP[st])
    sc = clo.Scanner("blelloch", ctx, et, st)
    aligned = None
    wide = a.astype(np.longdouble)
    exact = np.concatenate(([0.0], np.cumsum(wide)[:-1]))
    scale = np.concatenate(([0.0], np.cumsum(np.abs(wide))[:-1])) + 1.0
    eps = np.finfo(sdt).eps

    def check(got, tag):
        nonlocal aligned
        err = np.abs(got.astype(np.longdouble) - exact) / scale
        assert np.all(err <= 256 * eps), (tag, float(err.max() / eps))
        if aligned is None:
            aligned = got.copy()
            assert np.array_equal(got.view(np.uint8), fscan_model.scan(a, sdt).view(np.uint8)), tag + ": differs from the model"
        assert np.array_equal(got.view(np.uint8), aligned.view(np.uint8)), tag + ": differs from the aligned scan"

    run_scan(dev, sc, a, sdt, [(0, 0)] + scan_configs(a.itemsize, sdt.itemsize, n < (1 << 21)), check)
    sc.close()


@pytest.mark.parametrize("et", ["uchar", "short", "uint", "ulong"])
def test_reduce_sum(dev, et):
    from cl_ops_amd import _hip
    clo, ctx, q = dev
    n = 300001
    a = scan_input(et, n, 5)
    want = int(a.astype(np.int64).view(np.uint64).sum(dtype=np.uint64))
    total = clo.Buffer(ctx, 8)
    for off in [0] + offsets(a.itemsize):
        src = Region(dev, a.nbytes, off, a, salt=1)
        _hip.check(_hip.lib.clo_hip_reduce_sum(src.ptr, n, a.itemsize, int(a.dtype.kind == "i"), total.ptr, q.stream))
        q.finish()
        assert int(total.read(q, np.uint64, 1)[0]) == want, off
        src.check(None, "reduce_sum @%d" % off)
        src.close()
    total.close()


# ---------------------------------------------------------------------------------------------------------------------
# bitonic sorts and gselect
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("alg,n", [("sbitonic", 3000), ("sbitonic", 100003), ("abitonic", 3000), ("abitonic", 100003),
                                   ("gselect", 3000)])
@pytest.mark.parametrize("etype", ["uint", "ushort", "uchar", "double"])
def test_bitonic_and_gselect(dev, alg, n, etype):
    """Ascending by value; doubles without NaNs and zeros, so that equal keys are equal bits."""
    clo, ctx, q = dev
    if etype == "double":
        a = np.random.default_rng(n).standard_normal(n) * 1e3
    else:
        a = random_bits(_NP[etype], n, n + 1)
    s = clo.Sorter(alg, ctx, etype)
    run_sort(dev, s, a, np.sort(a, kind="stable"), configs(a.itemsize, n < 10000), alg)
    s.close()


# ---------------------------------------------------------------------------------------------------------------------
# RNG fill into t[k:]
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.NAMES)
def test_rng_fill_into_a_torch_slice(dev, name):
    """clo_rng_fill into a slice of an int32 tensor at byte offsets 4, 8 and 12 past a 256-byte guard, numel a
    multiple of 4 and not, 1000 states: values and final states as the model has them, guard words unchanged."""
    import torch
    clo, ctx, q = dev
    S = 1000
    r = clo.Rng(name, ctx, q, "dev_gid", None, S, 5)
    st = M.dev_gid_states(name, S, 5)
    for numel in (4000, 4001, 4003):
        for k in (1, 2, 3):
            total = numel + 2 * (G // 4) + 4
            canary = np.resize(_PAT[0], 4 * total).view(np.int32)
            base = torch.from_numpy(canary.copy()).cuda()
            torch.cuda.synchronize()
            lo = G // 4 + k
            r.fill(q, base[lo:lo + numel], numel)
            q.finish()
            exp, st = M.fill(name, st, numel)
            got = base.cpu().numpy()
            want = canary.copy()
            want[lo:lo + numel] = exp.view(np.int32)
            assert np.array_equal(got[:lo], want[:lo]) and np.array_equal(got[lo + numel:], want[lo + numel:]), \
                (name, numel, k, "guard words")
            assert np.array_equal(got[lo:lo + numel], want[lo:lo + numel]), (name, numel, k)
            assert np.array_equal(r.states(q), st), (name, numel, k, "states")
    r.close()


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_radix_sort_fed: first digits at any byte
# ---------------------------------------------------------------------------------------------------------------------

def test_radix_sort_fed_first_digits_at_any_byte(dev):
    """The first histogram reads the caller's digit bytes; they may start at any byte of `tmp`."""
    from cl_ops_amd import _hip
    from cl_ops_amd._hip import lib
    clo, ctx, q = dev
    n, es = (1 << 22) + 77, 8
    a = random_bits(np.uint64, n, 13)
    lib.clo_hip_env_refresh()
    assert lib.clo_hip_radix_takes_first_digits(n, es, 0, 4) == 1
    want = np.sort(a)
    digits = (a & np.uint64(0xff)).astype(np.uint8)
    wsb = lib.clo_hip_radix_workspace_bytes(n, es, 64, 4)
    src, tmp, ws = clo.Buffer(ctx, n * es), clo.Buffer(ctx, n * es), clo.Buffer(ctx, wsb)
    src.write(q, a)
    ws.write(q, np.zeros(128, np.uint32))
    for k in range(17):
        dst = Region(dev, n * es, 8 * (k % 3), salt=2)
        tmp.write(q, digits, offset=k)
        _hip.check(lib.clo_hip_radix_sort_fed(src.ptr, dst.ptr, tmp.ptr, n, es, 0, 64, 0, 4, tmp.ptr + k, ws.ptr, wsb,
                                              q.stream), "clo_hip_radix_sort_fed")
        q.finish()
        dst.check(want, "first digits at tmp + %d" % k)
        dst.close()
    for b in (src, tmp, ws):
        b.close()


# ---------------------------------------------------------------------------------------------------------------------
# misaligned scratch and atomic targets are refused
# ---------------------------------------------------------------------------------------------------------------------

_SZ = C.c_size_t


def _refusals(lib, d, ws, w8, n):
    """(entry, call) pairs of the workspace and of the uint64 word under test (`ws`, `w8`); d[0..3]: the data
    arrays, d[4]: a workspace that is aligned and initialised."""
    a, b, c, e = d[:4]
    sort_kv = lib["clo_hip_radix_sort_kv"]        # (a function object of its own: _hip.py does not declare this one)
    sort_kv.restype = C.c_int
    sort_kv.argtypes = [C.c_void_p] * 6 + [_SZ] + [C.c_int] * 5 + [C.c_void_p, _SZ, C.c_void_p]
    seg = (_SZ * 1)(n)
    rib = C.c_int(0)
    big = 1 << 20
    return [
        ("radix_sort", lambda: lib.clo_hip_radix_sort(a, b, c, n, 4, 0, 32, 0, 4, ws, big, None)),
        ("radix_sort_fed", lambda: lib.clo_hip_radix_sort_fed(a, b, c, n, 4, 0, 32, 0, 4, None, ws, big, None)),
        ("radix_sort_kv", lambda: sort_kv(a, None, None, b, c, e, n, 4, 0, 32, 0, 4, ws, big, None)),
        ("radix_sort_segmented", lambda: lib.clo_hip_radix_sort_segmented(a, b, c, n, seg, 1, None, None, None, 0, 4, 0, 32, 4,
                                                                          ws, big, None, C.byref(rib))),
        ("radix_sort_segmented2", lambda: lib.clo_hip_radix_sort_segmented2(a, None, b, c, n, seg, 1, None, None, None, None, 0,
                                                                            4, 0, 32, 4, ws, big, None, C.byref(rib))),
        ("msd_partition", lambda: lib.clo_hip_msd_partition(a, b, n, 4, 0, 32, 4, None, ws, big, None)),
        ("scan_workspace_init", lambda: lib.clo_hip_scan_workspace_init(ws, big, None)),
        ("scan_exclusive", lambda: lib.clo_hip_scan_exclusive(a, b, n, 4, 0, 8, ws, big, None)),
        ("scan_exclusive_carry", lambda: lib.clo_hip_scan_exclusive_carry(a, b, n, 4, 0, 8, None, None, ws, big, None)),
        ("scan_exclusive_typed", lambda: lib.clo_hip_scan_exclusive_typed(a, b, n, 9, 8, ws, big, None)),
        ("scan_exclusive_fp", lambda: lib.clo_hip_scan_exclusive_fp(a, b, n, 9, 4, ws, big, None)),
    ], [
        ("scan_exclusive_carry in", lambda: lib.clo_hip_scan_exclusive_carry(a, b, n, 4, 0, 8, w8, None, d[4], big, None)),
        ("scan_exclusive_carry out", lambda: lib.clo_hip_scan_exclusive_carry(a, b, n, 4, 0, 8, None, w8, d[4], big, None)),
        ("reduce_sum", lambda: lib.clo_hip_reduce_sum(a, n, 4, 0, w8, None)),
        ("msd_histogram", lambda: lib.clo_hip_msd_histogram(a, n, 4, 0, 32, 2, w8, None)),
        ("msd_partition counts", lambda: lib.clo_hip_msd_partition(a, b, n, 4, 0, 32, 4, w8, d[4], big, None)),
    ]


@pytest.mark.parametrize("ws_off,w8_off", [(8, 4), (128, 12), (64, 1)])
def test_misaligned_workspace_and_words_are_refused(dev, ws_off, w8_off):
    """Each clo_hip_* entry that takes a workspace (CLO_HIP_WORKSPACE_ALIGN = 256 bytes) or a device uint64 word
    (8 bytes) returns CLO_HIP_EARGS when it is misaligned, before anything is enqueued: the arrays and the
    scratch are left as they were."""
    from cl_ops_amd import _hip
    clo, ctx, q = dev
    lib = _hip.lib
    n = 5000
    arr = [Region(dev, 8 * n, 0, salt=i % 3) for i in range(4)] + [Region(dev, 1 << 20, 0)]
    scratch = Region(dev, (1 << 20) + 512, 0, salt=1)
    d = [r.ptr for r in arr]
    # the word and workspace under test lie inside `scratch` at the offsets: valid memory, only misaligned
    ws_calls, w8_calls = _refusals(lib, d, scratch.ptr + ws_off, scratch.ptr + w8_off, n)
    _hip.check(lib.clo_hip_scan_workspace_init(d[4], 1 << 20, q.stream))
    for what, call in ws_calls + w8_calls:
        st = call()
        assert st == _hip.CLO_HIP_EARGS, (what, st)
    q.finish()
    _hip.check(lib.clo_hip_scan_workspace_forget(d[4]))
    scratch.check(None, "scratch")
    for r in arr[:4]:
        r.check(None, "arrays")
    for r in arr + [scratch]:
        r.close()
