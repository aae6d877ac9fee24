"""The bitonic sorts, one sort per distinct launch schedule (tests/bitonic_schedule_model.py): every kernel family at
every step count, element size and key mode ends a sort once — in the LAST stage, whose comparators nothing after
them can heal — at the smallest size that has it. tests/test_bitonic_reach_cpu.py walks ROWS, JIT_ROWS and
SORTER_ROWS through the model without a GPU and proves that.

Every case: the `launches` out-parameter against the model's count; for the ahead-of-time kernels the per-label counts
of clo_hip_timing_read against the model's (the device ran the kernels the case is named for); the result bit for bit —
whole-element keys against np.sort of the order image in both directions, partial keys and every run-time compiled
case against the oracle's network (oracle_lib.sbitonic), tie order included: few distinct keys, the element's index in
the bits outside the key field. Key layouts rotate over the table (random, sorted, reversed, organ pipe, two values;
whole-element keys sort descending in the layout after their row's: two values alone let a skipped step through);
every buffer sits between canaries, half of the views start one element past a 16-byte boundary, one size per element
size is no power of two."""
import ctypes as C

import numpy as np
import pytest

import bitonic_schedule_model as M
import oracle_lib as O

pytestmark = pytest.mark.gpu

CANARY = 0xC3
GUARD = 256
LAYOUTS = ("random", "sorted", "reversed", "organ_pipe", "two_values")
UNSIGNED = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}
# partial keys (mode 0) the oracle can express: (key_shift, key_bits, key_size) with the key's bytes whole or ending at
# the element's top bit; the last 8-byte one is wider than 32 bits (the 64-bit ordered keys of reg_network_general)
FIELDS = {1: [(4, 4, 1)], 2: [(8, 8, 1), (0, 8, 1)], 4: [(16, 16, 2), (0, 16, 2), (24, 8, 1)],
          8: [(32, 32, 4), (0, 32, 4), (48, 16, 2), (16, 48, 8)]}

# ---- the table ----------------------------------------------------------------------------------------------------------
# Ahead of time: (element size, mode, log2 of the padded size, CLO_BITONIC_MERGE2). Per element size and mode every
# log2 from the first tile-kernel size to the last size that brings a new last-stage pass (and 2 elements: the
# one-launch-per-step branch below 2^Q) ...
_LOG2 = {1: [1] + list(range(5, 23)), 2: [1] + list(range(5, 24)), 4: [1] + list(range(5, 25)), 8: [1] + list(range(4, 22))}
MODES = {1: (0, 1, 2), 2: (0, 1, 2, 3), 4: (0, 1, 2, 3), 8: (0, 1, 2, 3)}
ROWS = [(es, mode, T, 0 if (es == 4 and mode and T == 24) else 1)     # (4-byte whole keys at 2^24: the 10-step pass runs without the two-tile merge)
        for es in (1, 2, 4, 8) for mode in MODES[es] for T in _LOG2[es]]
# ... the two-tile merge at its smallest size, two tiles, where only CLO_BITONIC_MERGE2=2 takes it ...
ROWS += [(es, mode, M.klf_of(es) + 1, 2) for es in (1, 2, 4, 8) for mode in MODES[es] if mode]
# ... and the rows that are there for a decision of the host code, not for a kernel
# (general keys alone keep the two-tile merge away at (4, 0, 24, 1), the element size alone at (1, 1, 22, 1) and others)
ROWS += [(4, 1, 24, 1),      # use_m2 taken because it saves a pass (stage 24: 9 steps and the two-tile merge)
         (2, 1, 24, 1)]      # a 10-step pass on 32-byte rows, costed 250: the cut is 3 + 7
# one size per element size that is no power of two (whole-element keys: the tail is padded): elements short of 2^T
NOT_POW2 = {(1, 1, 17, 1): 1001, (2, 2, 16, 1): 4097, (4, 3, 17, 1): 12345, (8, 1, 15, 1): 1}

# Run-time compiled: (element type, "get_key" | "compare", expression, (key_shift, key_size) as the oracle sees it)
JIT_EXPR = {(1, "get_key"): ("uchar", "(x) / 16", (4, 1)), (1, "compare"): ("uchar", "((a) & 0xF0) > ((b) & 0xF0)", (4, 1)),
            (2, "get_key"): ("ushort", "(x) / 256", (8, 1)), (2, "compare"): ("ushort", "((a) & 0xFF) > ((b) & 0xFF)", (0, 1)),
            (4, "get_key"): ("uint", "(x) / 65536", (16, 2)), (4, "compare"): ("uint", "((a) & 0xFF) > ((b) & 0xFF)", (0, 1)),
            (8, "get_key"): ("ulong", "(x) / 4294967296", (32, 4)), (8, "compare"): ("ulong", "((a) & 0xFF) > ((b) & 0xFF)", (0, 1))}
_JIT_LOG2 = {1: [1] + list(range(5, 22)), 2: [1] + list(range(5, 22)), 4: [1] + list(range(5, 22)), 8: [1] + list(range(4, 21))}
JIT_ROWS = [(es, kind, T) for es in (1, 2, 4, 8) for kind in ("get_key", "compare") for T in _JIT_LOG2[es]]
# `-(x)` on floating-point elements (no shift and mask says that): (element type, log2 numel)
JIT_FLOAT_ROWS = [("float", 20), ("double", 17)]

# Through Sorter(...): (algorithm, element type, key type, compare, get_key, numel, what clo_sort_new makes of it)
SORTER_ROWS = [("abitonic", "uint", None, None, None, 1 << 16, "aot"),
               ("sbitonic", "ulong", "uint", None, "(uint) ((x) >> 32)", 1 << 15, "aot"),
               ("abitonic", "uint", None, None, "(x) / 65536", 1 << 15, "jit"),
               ("sbitonic", "uint", None, "((a) & 0xFF) > ((b) & 0xFF)", None, 1 << 14, "jit"),
               ("abitonic", "float", None, "((a) < (b))", None, 1 << 15, "aot"),
               ("abitonic", "float", None, None, "-(x)", 1 << 14, "jit"),
               ("sbitonic", "int", None, None, "((x))", (1 << 16) - 333, "aot")]


def row_numel(row):
    return (1 << row[2]) - NOT_POW2.get(row, 0)


def row_field(k, es):
    """(key_shift, key_bits, key_size, key_kind) of the k-th general-key row: the fields rotate, signed keys where the
    key's bytes are whole."""
    shift, bits, size = FIELDS[es][k % len(FIELDS[es])]
    return shift, bits, size, 1 if (k // len(FIELDS[es])) % 2 and bits == 8 * size else 0


BOTH_DIRECTIONS_LOG2 = 21


def general_direction(k):
    """The one direction of a general-key row above 2^21."""
    return k % 2


def _aot_id(row):
    es, mode, T, m2 = row
    return "e%d-m%d-2p%d%s-merge2_%d" % (es, mode, T, "-%d" % NOT_POW2[row] if row in NOT_POW2 else "", m2)


assert len(set(ROWS)) == len(ROWS) and all(r in ROWS for r in NOT_POW2)


# ---- data ---------------------------------------------------------------------------------------------------------------

def image(a, kind):
    """The unsigned integer with the order of the typed key (whole elements)."""
    ut = UNSIGNED[a.dtype.itemsize]
    u = a.view(ut)
    sign = ut(1) << ut(8 * a.dtype.itemsize - 1)
    if kind == 0:
        return u.copy()
    if kind == 1:
        return u ^ sign
    return np.where(u & sign, ~u, u | sign)


def unimage(img, kind):
    ut = img.dtype.type
    sign = ut(1) << ut(8 * img.dtype.itemsize - 1)
    if kind == 0:
        return img.copy()
    if kind == 1:
        return img ^ sign
    return np.where(img & sign, img ^ sign, ~img)


def arrange(img, layout):
    """Keys (any unsigned order image) in the case's layout."""
    if layout == "random" or layout == "two_values":
        return img
    s = np.sort(img)
    if layout == "sorted":
        return s
    if layout == "reversed":
        return s[::-1].copy()
    return np.concatenate((s[0::2], s[1::2][::-1]))


def whole_keys(es, kind, n, layout, seed):
    """n whole-element keys as their unsigned bits; floating point without -0.0 and NaN: equal keys are equal bits."""
    rng = np.random.default_rng(seed)
    ut = UNSIGNED[es]
    if kind == 2:
        ft = {2: np.float16, 4: np.float32, 8: np.float64}[es]
        if layout == "two_values":
            a = np.array([-1.5, 2.0], ft)[rng.integers(0, 2, n)]
        else:
            a = (rng.standard_normal(n) * (10.0 ** rng.integers(-3, 4, n))).astype(ft)
            a[a == 0] = ft(1.0)
        assert np.isfinite(a).all()
        u = a.view(ut)
    elif layout == "two_values":
        u = np.array([1, (1 << (8 * es)) - 2], ut)[rng.integers(0, 2, n)]          # (signed: 1 and -2)
    else:
        u = rng.integers(0, 1 << (8 * es), n, dtype=np.uint64).astype(ut)
    return unimage(arrange(image(u, kind), layout), kind)


def partial_keys(es, shift, bits, kind, n, layout, seed):
    """n elements whose key field holds one of 2 (layout two_values) or 50 distinct keys, arranged by the layout in the
    key's typed order, and whose other bits hold the element's index (as much of it as fits)."""
    rng = np.random.default_rng(seed)
    ut = UNSIGNED[es]
    distinct = min(2 if layout == "two_values" else 50, 1 << bits)
    vals = rng.choice(1 << bits, distinct, replace=False).astype(np.uint64)
    rank = rng.integers(0, distinct, n)
    order = np.argsort(vals ^ np.uint64((1 << (bits - 1)) if kind == 1 else 0), kind="stable")      # typed order of the distinct keys
    rank = arrange(rank.astype(np.uint64), layout).astype(np.int64)
    keys = vals[order][rank]
    idx = np.arange(n, dtype=np.uint64)
    low = idx & np.uint64((1 << shift) - 1)
    hb = 8 * es - shift - bits
    high = (idx >> np.uint64(shift)) & np.uint64((1 << hb) - 1) if hb else np.zeros(n, np.uint64)
    e = low | (keys << np.uint64(shift))
    if hb:
        e |= high << np.uint64(shift + bits)
    return e.astype(ut)


# ---- device -------------------------------------------------------------------------------------------------------------

def _lib():
    from cl_ops_amd._hip import lib
    return lib


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, _ = gpu
    q = clo.Queue(ctx)
    handles = {}
    yield clo, ctx, q, handles
    q.finish()
    for h in handles.values():
        _lib().clo_hip_bitonic_jit_destroy(h)
    q.close()


@pytest.fixture(autouse=True)
def switches(monkeypatch):
    """Every test starts and ends on the library's own CLO_BITONIC_MERGE2 and with the launch timing off; the function
    handed out sets the mode of a case."""
    lib = _lib()
    monkeypatch.delenv("CLO_BITONIC_MERGE2", raising=False)
    lib.clo_hip_env_refresh()

    def merge2(mode):
        monkeypatch.setenv("CLO_BITONIC_MERGE2", str(mode))
        lib.clo_hip_env_refresh()

    yield merge2
    lib.clo_hip_timing_enable(0)
    lib.clo_hip_timing_reset()
    monkeypatch.undo()
    lib.clo_hip_env_refresh()


class View:
    """`cap` elements of `es` bytes inside a buffer of their own, GUARD canary bytes on both sides; odd: the view
    starts one element past a 16-byte boundary."""

    def __init__(self, dev, cap, es, odd):
        clo, ctx, self.q = dev[0], dev[1], dev[2]
        self.cap, self.es = cap, es
        self.off = GUARD + (es if odd else 0)
        self.total = (self.off + cap * es + GUARD + 15) & ~15
        self.b = clo.Buffer(ctx, self.total)
        assert self.b.ptr % 16 == 0
        self.ptr = self.b.ptr + self.off

    def put(self, a):
        from cl_ops_amd import _hip
        _hip.check(_lib().clo_hip_memset_async(self.b.ptr, CANARY, self.total, self.q.stream), "clo_hip_memset_async")
        self.b.write(self.q, a, self.off)

    def check(self, want, what):
        """The first want.size elements are `want`, bit for bit; nothing outside the view was written."""
        raw = self.b.read(self.q, np.uint8, self.total)
        end = self.off + self.cap * self.es
        assert (raw[:self.off] == CANARY).all(), what + ": bytes below the view were written"
        assert (raw[end:] == CANARY).all(), what + ": bytes above the view were written"
        w = np.ascontiguousarray(want).view(np.uint8)
        body = raw[self.off:self.off + w.size]
        if not np.array_equal(body, w):
            bad = np.flatnonzero(body != w)
            raise AssertionError("%s: %d of %d bytes differ, the first in element %d" % (what, bad.size, w.size, bad[0] // self.es))

    def close(self):
        self.b.close()


def timed(fn):
    """fn() with the launch timing on: {label: launches recorded}."""
    from cl_ops_amd import _hip
    lib = _lib()
    lib.clo_hip_timing_reset()
    lib.clo_hip_timing_enable(1)
    try:
        fn()
        return {l: _hip.timing_read(l)[0] for l in M.LABELS}
    finally:
        lib.clo_hip_timing_enable(0)
        lib.clo_hip_timing_reset()


def run_aot(dev, switches, row, k):
    es, mode, T, m2 = row
    lib, q = _lib(), dev[2]
    n = row_numel(row)
    cap = lib.clo_hip_bitonic_padded_numel(n)
    assert cap == 1 << T
    layout = LAYOUTS[k % len(LAYOUTS)]
    model = M.aot_schedule(es, mode, n, m2)
    switches(m2)
    if mode:
        # ascending in the row's layout, descending in the next one: two values alone let most wrong networks through
        shift, bits, size, kind = 0, 8 * es, es, mode - 1
        jobs = []
        for desc in (0, 1):
            a = whole_keys(es, kind, n, LAYOUTS[(k + desc) % len(LAYOUTS)], 7000 + k)
            s = np.sort(image(a, kind))
            pad = np.zeros(cap - n, s.dtype) if desc else np.full(cap - n, s.dtype.type(~s.dtype.type(0)))
            jobs.append((desc, a, unimage(np.concatenate((s[::-1] if desc else s, pad)), kind)))
    else:
        shift, bits, size, kind = row_field(k, es)
        assert M.mode_of(es, shift, bits, size, kind) == 0
        a = partial_keys(es, shift, bits, kind, n, layout, 7000 + k)
        # (both directions up to 2^21; above, where the oracle's network takes seconds, one per case, alternating)
        jobs = [(desc, a, O.sbitonic(a, threads=0, key_size=size, key_shift=shift, key_kind=kind, descending=bool(desc)))
                for desc in ((0, 1) if T <= BOTH_DIRECTIONS_LOG2 else (general_direction(k),))]
    v = View(dev, cap, es, k % 2 == 1)
    try:
        for desc, a, want in jobs:
            v.put(a)
            launches = C.c_int(-1)

            def call():
                st = lib.clo_hip_bitonic_tiled(v.ptr, n, es, shift, bits, size, kind, desc, C.byref(launches), q.stream)
                assert st == 0, (_aot_id(row), st)
                q.finish()

            counts = timed(call)
            what = "%s %s %s" % (_aot_id(row), LAYOUTS[(k + desc * (mode != 0)) % len(LAYOUTS)], "descending" if desc else "ascending")
            assert launches.value == len(model), what
            assert counts == M.label_counts(model), what
            v.check(want, what)
    finally:
        q.finish()
        v.close()


def jit_handle(dev, elem_type, compare, get_key):
    handles = dev[3]
    key = (elem_type, compare, get_key)
    if key not in handles:
        h, log = C.c_void_p(), C.c_char_p()
        t = M.TYPES[elem_type][0]
        st = _lib().clo_hip_bitonic_jit_create(t, t, compare.encode() if compare else None, get_key.encode() if get_key else None, None,
                                               C.byref(h), C.byref(log))
        assert st == 0 and h.value, (key, st, log.value)
        handles[key] = h
    return handles[key]


def run_jit(dev, elem_type, compare, get_key, a, want, what):
    lib, q = _lib(), dev[2]
    es = a.dtype.itemsize
    h = jit_handle(dev, elem_type, compare, get_key)
    model = M.jit_schedule(es, a.size)
    v = View(dev, a.size, es, M.log2u(a.size) % 2 == 1)
    try:
        v.put(a)
        launches = C.c_int(-1)

        def call():
            st = lib.clo_hip_bitonic_jit_sort(h, v.ptr, a.size, 1, C.byref(launches), q.stream)
            assert st == 0, (what, st)
            q.finish()

        counts = timed(call)
        assert launches.value == len(model), what
        assert not any(counts.values()), what + ": ahead-of-time kernels ran"
        v.check(want, what)
    finally:
        q.finish()
        v.close()


# ---- tests --------------------------------------------------------------------------------------------------------------

def _params(rows, ids):
    return [pytest.param(r, k, id=ids(r)) for k, r in enumerate(rows)]


@pytest.mark.parametrize("row,k", _params(ROWS, _aot_id))
def test_ahead_of_time_schedule(dev, switches, row, k):
    run_aot(dev, switches, row, k)


@pytest.mark.parametrize("row,k", _params(JIT_ROWS, lambda r: "e%d-%s-2p%d" % r))
def test_run_time_compiled_schedule(dev, row, k):
    es, kind, T = row
    elem_type, expr, (shift, size) = JIT_EXPR[(es, kind)]
    layout = LAYOUTS[k % len(LAYOUTS)]
    bits = min(8 * size, 8 * es - shift)
    a = partial_keys(es, shift, bits, 0, 1 << T, layout, 9000 + k)
    want = O.sbitonic(a, threads=0, key_size=size, key_shift=shift)
    run_jit(dev, elem_type, expr if kind == "compare" else None, expr if kind == "get_key" else None, a, want,
            "%s %s 2^%d %s" % (elem_type, expr, T, layout))


@pytest.mark.parametrize("elem_type,T", JIT_FLOAT_ROWS)
def test_run_time_compiled_negated_float_key(dev, elem_type, T):
    """get_key `-(x)` with the default compare sorts descending by value: the oracle's network with `<`."""
    es = M.TYPES[elem_type][1]
    a = whole_keys(es, 2, 1 << T, "random", T).view({4: np.float32, 8: np.float64}[es])
    want = O.sbitonic(a, threads=0, key_kind=O.KEY_FLOAT, descending=True)
    run_jit(dev, elem_type, None, "-(x)", a, want, "%s -(x) 2^%d" % (elem_type, T))


@pytest.mark.parametrize("elem_type", ["half", "float", "double"])
def test_float_zeros_and_nans(dev, elem_type):
    """Both zeros, infinities and NaNs of both signs with two payloads among ordinary keys, one merge stage above the
    tile: the IEEE total order (-NaN < -inf < -0 < +0 < +inf < +NaN), which is the oracle's network run on the order
    image — upstream's own `>` leaves NaNs where they are and ties the zeros."""
    lib, q = _lib(), dev[2]
    es = M.TYPES[elem_type][1]
    ut = UNSIGNED[es]
    n = 1 << (M.klf_of(es) + 1)
    a = whole_keys(es, 2, n, "random", 31)
    rng = np.random.default_rng(32)
    ft = {2: np.float16, 4: np.float32, 8: np.float64}[es]
    sign = ut(1) << ut(8 * es - 1)
    nan, inf = np.array([np.nan, np.inf], ft).view(ut)
    special = np.array([0, sign, inf, inf | sign, nan, nan | ut(1), nan | sign, nan | sign | ut(2)], ut)
    a[rng.integers(0, n, n // 4)] = special[rng.integers(0, special.size, n // 4)]
    model = M.aot_schedule(es, 3, n, 1)
    v = View(dev, n, es, True)
    try:
        for desc in (0, 1):
            want = unimage(O.sbitonic(image(a, 2), threads=0, descending=bool(desc)), 2)
            assert np.array_equal(image(want, 2), np.sort(image(a, 2))[::-1 if desc else 1])
            v.put(a)
            launches = C.c_int(-1)
            assert lib.clo_hip_bitonic_tiled(v.ptr, n, es, 0, 8 * es, es, 2, desc, C.byref(launches), q.stream) == 0
            q.finish()
            assert launches.value == len(model)
            v.check(want, "%s zeros and NaNs, descending %d" % (elem_type, desc))
    finally:
        q.finish()
        v.close()


@pytest.mark.parametrize("row", SORTER_ROWS, ids=lambda r: "-".join(str(x) for x in r[:2]) + "-" + r[6] + "-%d" % r[5])
def test_sorter_routing(dev, row):
    """Sorter("sbitonic" | "abitonic", ...): which expressions reach the ahead-of-time kernels (their labels count the
    model's launches) and which hiprtc (no labelled launch at all), and the result either way."""
    alg, et, kt, compare, get_key, n, how = row
    clo, ctx, q = dev[0], dev[1], dev[2]
    es = M.TYPES[et][1]
    route, _, spec = M.route(et, kt, compare, get_key)
    model_how, model = M.sorter_schedule(et, n, kt, compare, get_key)
    assert route == how == model_how and model is not None
    k = SORTER_ROWS.index(row)
    if how == "aot" and M.mode_of(es, *spec[:4]):
        kind = spec[3]
        a = whole_keys(es, kind, n, LAYOUTS[k % 5], 100 + k)
        s = np.sort(image(a, kind))
        want = unimage(s[::-1] if spec[4] else s, kind)
    elif how == "aot":
        shift, bits, size, kind, desc = spec
        a = partial_keys(es, shift, bits, kind, n, LAYOUTS[k % 5], 100 + k)
        want = O.sbitonic(a, threads=0, key_size=size, key_shift=shift, key_kind=kind, descending=bool(desc))
    elif get_key == "-(x)":
        a = whole_keys(es, 2, n, "random", 100 + k)
        want = O.sbitonic(a.view(np.float32), threads=0, key_kind=O.KEY_FLOAT, descending=True).view(a.dtype)
    else:
        shift, size = (16, 2) if get_key else (0, 1)
        a = partial_keys(es, shift, 8 * size, 0, n, LAYOUTS[k % 5], 100 + k)
        want = O.sbitonic(a, threads=0, key_size=size, key_shift=shift)
    s = clo.Sorter(alg, ctx, et, key_type=kt, compare=compare, get_key=get_key)
    src, dst = View(dev, n, es, k % 2 == 0), View(dev, n, es, k % 2 == 1)
    bin_, bout = clo.Buffer(ctx, n * es, device_ptr=src.ptr), clo.Buffer(ctx, n * es, device_ptr=dst.ptr)
    try:
        src.put(a)
        dst.put(np.zeros(n, a.dtype))

        def call():
            s.with_device_data(q, bin_, bout, n)
            q.finish()

        counts = timed(call)
        if how == "aot":
            assert counts == M.label_counts(model), row
        else:
            assert not any(counts.values()), row
        dst.check(want, str(row))
        src.check(a, str(row) + ": the source")
    finally:
        q.finish()
        s.close()
        for b in (bin_, bout, src, dst):
            b.close()
