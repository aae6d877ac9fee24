"""The scatter of clo_radix4_pair_kernel under run-structured keys (tests/radix_pass_model.py): every case calls the
thin C ABI (clo_hip_radix_sort, clo_hip_radix_sort_kv), so digit width, key field, key kind and element size are set
freely, and is compared bit for bit with a plain stable sort by the order key. tests/test_radix_pass_reach_cpu.py
imports CASES and proves without a GPU which path, which template instantiation and which branch of the scatter every
case reaches.

Around every result: 256 canary bytes below and above the output view, in half of the cases every view one element
past a 16-byte boundary, the source unchanged after an out-of-place sort, and a second call on the same workspace
with the input reversed."""
import ctypes as C
import functools

import numpy as np
import pytest

import radix_pass_model as M

pytestmark = pytest.mark.gpu

CANARY = 0xC3
GUARD = 256
N_BIG8 = (1 << 22) + 77          # 8-byte elements and key-value pairs on 1024-thread tiles (from 32 MiB)
N_BIG4 = (1 << 26) + 5           # the smallest size class of 4-byte elements on 1024-thread tiles (from 256 MiB)


def small_sizes(elem_size):
    tile = 512 * M.items_of(elem_size)
    return (2 * tile + 1, 9 * tile + 3, 17 * tile - 1)


def _passes(bits, db):
    pb = sum(M.PAIRS[db])
    return (bits + pb - 1) // pb, bits // pb


def _case(op, es, n, db, field, kind, family, pstar, k, **kw):
    c = dict(op=op, es=es, n=n, db=db, shift=field[0], bits=field[1], kind=kind, family=family, pstar=pstar, upper="random",
             seed=1000 + k, misaligned=k % 2 == 1, sweep0=n < N_BIG8, values=True, keys_out=True, inplace=False)
    c.update(kw)
    c["id"] = "%s%d-n%d-db%d-s%db%d-k%d-%s-p%d%s%s" % (
        op, es, n, db, c["shift"], c["bits"], kind, family, pstar, "-odd" if c["misaligned"] else "",
        "" if op == "keys" else ("-val" if c["values"] else "-arg") + ("" if c["keys_out"] else "-nokeys") + ("-inplace" if c["inplace"] else ""))
    return c


_FIELDS = {1: [(0, 8), (3, 5), (1, 7)], 2: [(0, 16), (3, 13), (5, 11)], 4: [(0, 32), (3, 29), (5, 12), (0, 20)],
           8: [(5, 12), (0, 20), (3, 29), (0, 64)]}


def _pstar(family, db, bits):
    passes, fullp = _passes(bits, db)
    if family == "single_mixed":
        return 0 if (db % 2 == 0 or fullp == 0) else fullp - 1
    if family == "short_runs":
        return passes - 1 if db % 2 == 0 else 0
    return passes - 1 if db % 2 == 1 else min(1, passes - 1)


def _small_cases():
    out = []
    for es in (1, 2, 4, 8):
        sizes = small_sizes(es)
        for db in range(1, 9):
            for fi, family in enumerate(("single_mixed", "short_runs", "two_runs")):
                fields = _FIELDS[es] if not (es == 8 and db <= 3) else _FIELDS[es][:3]
                field = fields[(db + fi) % len(fields)]
                n = sizes[2] if family == "two_runs" else sizes[(db + fi) % 2]
                out.append(_case("keys", es, n, db, field, 0, family, _pstar(family, db, field[1]), len(out)))
    # the other families, and signed (1) and IEEE (2) keys at every element size that has them
    extra = [(1, 0, "one_digit_per_tile", 8, (0, 8), 0), (2, 0, "one_digit_per_tile", 2, (3, 13), 3), (4, 0, "one_digit_per_tile", 5, (3, 29), 0),
             (8, 0, "one_digit_per_tile", 6, (0, 20), 1), (4, 0, "sorted", 4, (3, 29), 0), (8, 0, "reversed", 8, (5, 12), 0),
             (2, 0, "skew90", 1, (5, 11), 0), (4, 0, "short_runs", 3, (0, 20), 3), (4, 0, "two_runs", 5, (5, 12), 2),
             (1, 1, "sorted", 3, (0, 8), 0), (1, 1, "skew90", 8, (0, 8), 0), (2, 1, "reversed", 5, (0, 16), 0),
             (2, 2, "skew90", 4, (0, 16), 0), (2, 2, "sorted", 7, (0, 16), 0), (4, 1, "skew90", 6, (0, 32), 0),
             (4, 1, "one_digit_per_tile", 4, (0, 32), 3), (4, 1, "two_runs", 4, (3, 29), 3), (4, 2, "reversed", 8, (0, 32), 0),
             (4, 2, "sorted", 2, (0, 32), 0), (8, 1, "reversed", 4, (0, 64), 0), (8, 2, "skew90", 8, (0, 64), 0),
             (8, 2, "sorted", 7, (0, 64), 0), (8, 1, "short_runs", 5, (0, 64), 12)]
    for i, (es, kind, family, db, field, pstar) in enumerate(extra):
        out.append(_case("keys", es, small_sizes(es)[i % 3], db, field, kind, family, pstar, len(out)))
    return out


def _big8_cases():
    out = []
    # (digit_bits, field): all six (LB, HB); radix 16 with the digit stream (p* before the last pass), radix 256 on a
    # field of whole passes (p* = the last pass, which writes none)
    for db, field in ((1, (5, 12)), (2, (0, 16)), (3, (3, 18)), (5, (5, 20)), (7, (3, 21)), (4, (7, 20)), (8, (0, 24))):
        passes, fullp = _passes(field[1], db)
        for fi, family in enumerate(("single_mixed", "short_runs", "two_runs")):
            if db == 4:
                pstar = (0, 1, 0)[fi]
            elif db == 8:
                pstar = passes - 1
            else:
                pstar = (0, fullp - 1, passes - 1)[fi]
            out.append(_case("keys", 8, N_BIG8, db, field, 0, family, pstar, len(out)))
    return out


def _big4_cases():
    return [_case("keys", 4, N_BIG4, 4, (3, 29), 0, "short_runs", 0, 1),            # digit stream by shifts and masks, a last pass of 5 bits
            _case("keys", 4, N_BIG4, 8, (5, 20), 0, "two_runs", 2, 2),              # a last pass with no high digit
            _case("keys", 4, N_BIG4, 4, (0, 32), 0, "single_mixed", 2, 4, upper="grouped")]   # digit stream by byte permutes


def _kv_cases():
    out = []
    fields = {1: [(0, 8), (3, 5)], 2: [(0, 16), (3, 13)], 4: [(0, 32), (3, 29), (5, 12)]}
    for ks in (1, 2, 4):
        for n in (2 * 4096 + 1, 9 * 4096 + 3, N_BIG8):
            for family in ("short_runs", "two_runs", "single_mixed"):
                k = len(out)
                field = fields[ks][k % len(fields[ks])]
                db = 4 if k % 2 else 8
                passes = _passes(field[1], db)[0]
                out.append(_case("kv", ks, n, db, field, 0, family, (0, passes - 1)[(k + k // 3) % 2], k, values=k % 2 == 0, keys_out=k % 3 != 0))
    out.append(_case("kv", 1, 9 * 4096 + 3, 8, (0, 8), 0, "short_runs", 0, len(out), inplace=True))     # one pass in place: the unpack after it
    out.append(_case("kv", 1, 2 * 4096 + 1, 4, (0, 8), 1, "skew90", 0, len(out)))
    out.append(_case("kv", 2, 9 * 4096 + 3, 8, (0, 16), 2, "sorted", 0, len(out), values=False))
    out.append(_case("kv", 4, 2 * 4096 + 1, 4, (0, 32), 2, "skew90", 0, len(out), keys_out=False))
    out.append(_case("kv", 4, 9 * 4096 + 3, 8, (0, 32), 1, "reversed", 0, len(out)))
    return out


CASES = _small_cases() + _big8_cases() + _big4_cases() + _kv_cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def sim_geometry(case):
    """(element size, key shift) as the pair passes see the case: a key-value sort moves 8-byte pairs key << 32 | value."""
    return (8, 32 + case["shift"]) if case["op"] == "kv" else (case["es"], case["shift"])


@functools.lru_cache(maxsize=4)
def case_keys(op, es, n, db, shift, bits, kind, family, pstar, upper, seed):
    _, items, tile, _ = M.shape(n, 8 if op == "kv" else es)
    return M.make_keys(family, n, es, shift, bits, db, pstar, seed, kind, tile, items, upper)


def keys_of(case):
    return case_keys(*(case[k] for k in ("op", "es", "n", "db", "shift", "bits", "kind", "family", "pstar", "upper", "seed")))


def values_of(case):
    if case["values"]:
        return np.random.default_rng(case["seed"] + 1).integers(0, 1 << 32, case["n"], dtype=np.uint64).astype(np.uint32)
    return np.arange(case["n"], dtype=np.uint32)


# ----------------------------------------------------------------------------------------------------------------------

def _lib():
    from cl_ops_amd._hip import lib
    return lib


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, _ = gpu
    q = clo.Queue(ctx)
    lib = _lib()
    f = lib["clo_hip_radix_sort_kv"]
    f.restype = C.c_int
    f.argtypes = [C.c_void_p] * 6 + [C.c_size_t] + [C.c_int] * 5 + [C.c_void_p, C.c_size_t, C.c_void_p]
    g = lib["clo_hip_radix_kv_workspace_bytes"]
    g.restype = C.c_size_t
    g.argtypes = [C.c_size_t, C.c_int, C.c_int, C.c_int]
    yield clo, ctx, q, f, g
    q.close()


@pytest.fixture(autouse=True)
def library_switches(monkeypatch):
    """Every test starts and ends on the library's own choice of path; the function handed out turns the single-sweep
    passes off."""
    lib = _lib()
    monkeypatch.delenv("CLO_RADIX_SWEEP", raising=False)
    monkeypatch.delenv("CLO_RADIX_NO_DIGITS", raising=False)
    lib.clo_hip_env_refresh()

    def no_sweep():
        monkeypatch.setenv("CLO_RADIX_SWEEP", "0")
        lib.clo_hip_env_refresh()

    yield no_sweep
    monkeypatch.undo()
    lib.clo_hip_env_refresh()


class View:
    """n elements of `es` bytes inside a buffer of their own, GUARD canary bytes on both sides; odd: the view starts
    one element past a 16-byte boundary."""

    def __init__(self, dev, n, es, odd):
        clo, ctx, self.q = dev[0], dev[1], dev[2]
        self.n, self.es = n, es
        self.off = GUARD + (es if odd else 0)
        self.total = (self.off + n * es + GUARD + 15) & ~15
        self.b = clo.Buffer(ctx, self.total)
        assert self.b.ptr % 16 == 0
        self.ptr = self.b.ptr + self.off

    def fill(self):
        from cl_ops_amd import _hip
        _hip.check(_lib().clo_hip_memset_async(self.b.ptr, CANARY, self.total, self.q.stream), "clo_hip_memset_async")

    def put(self, a):
        assert a.nbytes == self.n * self.es
        self.b.write(self.q, a, self.off)

    def check(self, want, what):
        raw = self.b.read(self.q, np.uint8, self.total)
        body = raw[self.off:self.off + self.n * self.es]
        assert (raw[:self.off] == CANARY).all(), what + ": bytes below the view were written"
        assert (raw[self.off + self.n * self.es:] == CANARY).all(), what + ": bytes above the view were written"
        w = np.ascontiguousarray(want).view(np.uint8)
        if not np.array_equal(body, w):
            bad = np.flatnonzero(body != w)
            raise AssertionError("%s: %d of %d bytes differ, the first in element %d" % (what, bad.size, w.size, bad[0] // self.es))

    def close(self):
        self.b.close()


def reference(a, case):
    """(order, sorted elements): a plain stable sort by the order key; at 2^26 the order comes from torch's stable
    sort on the device."""
    if a.size < N_BIG4:
        order = M.stable_order(a, case["shift"], case["bits"], case["kind"])
        return order, a[order]
    import torch
    k = torch.from_numpy(M.order_key(a, case["shift"], case["bits"], case["kind"]).astype(np.int64)).cuda()
    order = torch.sort(k, stable=True).indices
    del k
    out = torch.from_numpy(a.view(np.int32)).cuda()[order].cpu().numpy().view(a.dtype)
    order = order.cpu().numpy()
    torch.cuda.empty_cache()
    return order, out


def run_keys(dev, case):
    clo, ctx, q = dev[0], dev[1], dev[2]
    lib = _lib()
    n, es, odd = case["n"], case["es"], case["misaligned"]
    a = keys_of(case)
    assert lib.clo_hip_radix_polls(n, es, case["db"]) == 0
    wsb = lib.clo_hip_radix_workspace_bytes(n, es, case["bits"], case["db"])
    src, dst, tmp = View(dev, n, es, odd), View(dev, n, es, odd), View(dev, n, es, odd)
    ws = clo.Buffer(ctx, wsb)
    try:
        ws.write(q, np.zeros(128, np.uint32))
        for rnd, inp in enumerate((a, a[::-1].copy())):
            want = reference(inp, case)[1]
            for v in (src, dst, tmp):
                v.fill()
            src.put(inp)
            st = lib.clo_hip_radix_sort(src.ptr, dst.ptr, tmp.ptr, n, es, case["shift"], case["bits"], case["kind"], case["db"],
                                        ws.ptr, wsb, q.stream)
            assert st == 0, (case["id"], rnd, st)
            q.finish()
            dst.check(want, "%s call %d: output" % (case["id"], rnd))
            src.check(inp, "%s call %d: source" % (case["id"], rnd))
            tmp_raw = tmp.b.read(q, np.uint8, tmp.total)
            assert (tmp_raw[:tmp.off] == CANARY).all() and (tmp_raw[tmp.off + n * es:] == CANARY).all(), case["id"] + ": around tmp"
            assert lib.clo_hip_check_status(ws.ptr, q.stream) == 0
    finally:
        q.finish()
        for b in (src, dst, tmp, ws):
            b.close()


def run_kv(dev, case):
    clo, ctx, q, sort_kv, kv_ws = dev
    n, ks, odd = case["n"], case["es"], case["misaligned"]
    keys = keys_of(case)
    vals = values_of(case)
    assert _lib().clo_hip_radix_polls(n, 8, case["db"]) == 0
    wsb = kv_ws(n, ks, case["bits"], case["db"])
    kin, vin = View(dev, n, ks, odd), View(dev, n, 4, odd)
    kout = kin if case["inplace"] else View(dev, n, ks, odd)
    vout = vin if case["inplace"] else View(dev, n, 4, odd)
    pa, pb = clo.Buffer(ctx, 8 * n), clo.Buffer(ctx, 8 * n)
    ws = clo.Buffer(ctx, wsb)
    try:
        ws.write(q, np.zeros(128, np.uint32))
        for rnd, (k, v) in enumerate(((keys, vals), (keys[::-1].copy(), vals if not case["values"] else vals[::-1].copy()))):
            order = reference(k, case)[0]
            for w in {kin, vin, kout, vout}:
                w.fill()
            kin.put(k)
            if case["values"]:
                vin.put(v)
            st = sort_kv(kin.ptr, vin.ptr if case["values"] else None, kout.ptr if case["keys_out"] else None, vout.ptr, pa.ptr, pb.ptr,
                         n, ks, case["shift"], case["bits"], case["kind"], case["db"], ws.ptr, wsb, q.stream)
            assert st == 0, (case["id"], rnd, st)
            q.finish()
            tag = "%s call %d: " % (case["id"], rnd)
            vout.check(v[order] if case["values"] else order.astype(np.uint32), tag + "values")
            if case["keys_out"]:
                kout.check(k[order], tag + "keys")
            elif not case["inplace"]:
                kout.check(np.full(n * ks, CANARY, np.uint8), tag + "keys_out is NULL, the view")
            if not case["inplace"]:
                kin.check(k, tag + "keys_in")
                if case["values"]:
                    vin.check(v, tag + "values_in")
    finally:
        q.finish()
        for b in {kin, vin, kout, vout, pa, pb, ws}:
            b.close()


def _group(pred):
    return [pytest.param(c, id=c["id"]) for c in CASES if pred(c)]


def _run(dev, library_switches, case):
    if case["sweep0"]:
        library_switches()
    (run_kv if case["op"] == "kv" else run_keys)(dev, case)


@pytest.mark.parametrize("case", _group(lambda c: c["op"] == "keys" and c["n"] < N_BIG8))
def test_small_tiles(dev, library_switches, case):
    """512-thread tiles, 2, 9 and 17 of them with a partial last one: every element size, digit width and family."""
    _run(dev, library_switches, case)


@pytest.mark.parametrize("case", _group(lambda c: c["op"] == "keys" and c["n"] == N_BIG8))
def test_big_tiles_8_bytes(dev, library_switches, case):
    """1024-thread tiles of 8-byte elements: all six (LB, HB), with the digit stream and without."""
    _run(dev, library_switches, case)


@pytest.mark.parametrize("case", _group(lambda c: c["op"] == "keys" and c["n"] == N_BIG4))
def test_big_tiles_4_bytes(dev, library_switches, case):
    """1024-thread tiles of 4-byte elements: four next digits per dword, gathered by shifts and masks (a key field at an
    odd bit) and by byte permutes; the order comes from torch's stable sort on the device."""
    _run(dev, library_switches, case)


@pytest.mark.parametrize("case", _group(lambda c: c["op"] == "kv"))
def test_key_value_passes(dev, library_switches, case):
    """The first and last pass of a key-value sort: keys of 1, 2 and 4 bytes, values or argsort, keys_out or none, and
    one pass in place (the unpack after it)."""
    _run(dev, library_switches, case)
