"""The thin C-ABI entries of include/clo_hip.h inside a client's stream capture, and the replays of the graph
(no allocation and no host synchronisation inside the calls). Every case follows one protocol:

1. every buffer and workspace is allocated up front (the scan's workspace initialised), nothing while a capture is open;
2. one eager call with the arguments that will be captured (code objects get loaded outside the capture), checked;
3. capture begin, the call(s), capture end: every status 0, the call's own looked at first, the capture ended and the
   graph destroyed whatever happens;
4. three replays (six across the scan's epoch wrap), each on new input contents written into the SAME device buffers
   by a copy on the stream outside the graph, the outputs refilled with a canary first; after the replay the outputs
   equal the CPU model bit for bit, the inputs are what was written (unless the call is in place), the status word
   of the workspace is clear where the entry has one;
5. the data distribution changes from replay to replay, so the shape frozen at capture meets inputs it was not
   captured on;
6. one more eager call on the same workspace afterwards.

No case can pass on a replay that returns the previous replay's output: the canary refill removes it and the
expected result belongs to other contents. Models are the suite's own: numpy's stable argsort in the key order of
test_gpu_sort_by_key.order_key, oracle_lib.serial_scan, rbk_model, sbk_model, hist_model, rng_model, oracle_lib.sbitonic
and oracle_lib.gselect.

Two deliberate readings of the list of cases:
- the typed (floating-point) scan is compared with an eager call on the same input and with tests/fscan_model.py,
  bit for bit, not with a float64 sum under a tolerance; one of its rounds uses small integers, whose float sums are
  exact, and is compared with oracle_lib.serial_scan of the same integers as well;
- oracle_lib.sbitonic restates upstream's network, which exists for powers of two only (for any other numel it would
  walk past the end of the array) and whose tie order the flip form behind clo_hip_bitonic_any does not keep. So the
  tie order against oracle_lib.sbitonic is checked where it is defined, clo_hip_bitonic_tiled with a key shift at 2^15,
  and clo_hip_bitonic_any at 5000 with a key shift is checked for the sorted key sequence, for being a permutation
  of its input, and for being bit-equal to the eager call on the same input (the network is deterministic).

The timing layer and the launch observer stay off; everything runs in this one process."""
import ctypes as C

import numpy as np
import pytest

import hist_model
import oracle_lib as O
import rbk_model
import rng_model as M
import sbk_model
import test_gpu_sort_by_key as SBK

pytestmark = pytest.mark.gpu

CANARY = 0xC3
_VP, _SZ, _CI, _CU = C.c_void_p, C.c_size_t, C.c_int, C.c_uint
T_INT, T_UINT, T_LONG, T_ULONG, T_HALF, T_FLOAT = 4, 5, 6, 7, 8, 9     # CloType numbers
_NP = {"int": np.int32, "uint": np.uint32, "long": np.int64, "ulong": np.uint64, "half": np.float16, "float": np.float32}
_CLO = {"int": T_INT, "uint": T_UINT, "long": T_LONG, "ulong": T_ULONG, "half": T_HALF, "float": T_FLOAT}
EPOCH_MAX = (1 << 30) - 1


def _lib():
    from cl_ops_amd._hip import lib
    return lib


def _bind(name, restype, *argtypes):
    """A function object of this file's own for an entry cl_ops_amd/_hip.py does not declare."""
    f = _lib()[name]
    f.restype = restype
    f.argtypes = list(argtypes)
    return f


class Entries:
    def __init__(self):
        self.sort_kv = _bind("clo_hip_radix_sort_kv", _CI, *([_VP] * 6 + [_SZ] + [_CI] * 5 + [_VP, _SZ, _VP]))
        self.kv_ws = _bind("clo_hip_radix_kv_workspace_bytes", _SZ, _SZ, _CI, _CI, _CI)
        self.rbk = _bind("clo_hip_reduce_by_key", _CI, _VP, _VP, _VP, _VP, _VP, _SZ, _CI, _CI, _CI, _CI, _VP, _SZ, _VP)
        self.rbk_ws = _bind("clo_hip_reduce_by_key_workspace_bytes", _SZ, _SZ)
        self.rbk_tile = _bind("clo_hip_reduce_by_key_tile", _SZ, _CI, _CI)
        self.sbk = _bind("clo_hip_scan_by_key", _CI, _VP, _VP, _VP, _SZ, _CI, _CI, _CI, _CI, _CI, _VP, _SZ, _VP)
        self.sbk_ws = _bind("clo_hip_scan_by_key_workspace_bytes", _SZ, _SZ)
        self.sbk_tile = _bind("clo_hip_scan_by_key_tile", _SZ, _CI, _CI)
        self.hist = _bind("clo_hip_histogram", _CI, _VP, _VP, _VP, _SZ, _CI, _CI, _CI, _CI, C.c_uint64, _CU, _SZ, _CI, _CU,
                          _VP, _SZ, _VP)
        self.hist_tile = _bind("clo_hip_histogram_tile", _SZ, _CI, _CI)
        self.hist_lds_bins = _bind("clo_hip_histogram_lds_bins", _SZ, _CI)
        self.rng_fill = _bind("clo_hip_rng_fill", _CI, _CI, _VP, _SZ, _VP, _SZ, _CU, _CU, _CI, _VP)
        self.gselect = _bind("clo_hip_gselect", _CI, _VP, _VP, _SZ, _CI, _CI, _CI, _CI, _CI, _CI, _VP)


@pytest.fixture(scope="module")
def dev(gpu):
    """(package, context, a queue of this file's own without profiling, the entries _hip.py does not declare)."""
    import cl_ops_amd as clo
    ctx, _ = gpu
    q = clo.Queue(ctx)
    assert _lib().clo_hip_timing_enabled() == 0
    yield clo, ctx, q, Entries()
    q.close()


@pytest.fixture(autouse=True)
def library_switches(monkeypatch):
    """The environment switches are what the library read last, possibly under another test's environment: every
    test starts and ends on the library's own choices. The function given to the test sets CLO_RADIX_SWEEP."""
    lib = _lib()
    monkeypatch.delenv("CLO_RADIX_SWEEP", raising=False)
    lib.clo_hip_env_refresh()

    def sweep(value):
        if value is not None:
            monkeypatch.setenv("CLO_RADIX_SWEEP", value)
            lib.clo_hip_env_refresh()

    yield sweep
    monkeypatch.undo()
    lib.clo_hip_env_refresh()


class Mem:
    """Device memory of nbytes, written and read through the queue's stream."""

    def __init__(self, dev, nbytes):
        clo, ctx, self.q, _ = dev
        self.n = nbytes
        self.b = clo.Buffer(ctx, max(nbytes, 16))

    @property
    def ptr(self):
        return self.b.ptr

    def put(self, array, offset=0):
        self.b.write(self.q, array, offset)

    def get(self, dtype, count, offset=0):
        return self.b.read(self.q, dtype, count, offset)

    def fill(self, byte=CANARY):
        from cl_ops_amd import _hip
        _hip.check(_lib().clo_hip_memset_async(self.ptr, byte, max(self.n, 16), self.q.stream), "clo_hip_memset_async")

    def close(self):
        self.b.close()


@pytest.fixture
def mem(dev):
    made = []

    def make(nbytes):
        made.append(Mem(dev, nbytes))
        return made[-1]

    yield make
    _lib().clo_hip_stream_synchronize(dev[2].stream)
    for m in made:
        m.close()


def canary(dtype, count):
    return np.full(count * np.dtype(dtype).itemsize, CANARY, np.uint8).view(dtype)


def same(got, want, what):
    """Bit for bit (NaNs included)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.dtype.itemsize == want.dtype.itemsize and got.size == want.size, (what, got.shape, want.shape)
    g, w = got.view(np.uint8), want.view(np.uint8)
    if not np.array_equal(g, w):
        bad = np.flatnonzero(g != w)
        raise AssertionError("%s: %d of %d bytes differ, the first at element %d" % (what, bad.size, g.size, bad[0] // got.dtype.itemsize))


def first(*calls):
    """The first non-zero status of the calls, made in order; nothing is called after it."""
    for call in calls:
        st = call()
        if st != 0:
            return st
    return 0


class Case:
    """load(k) -> what round k expects: writes round k's inputs into the device buffers and refills the outputs with the
    canary; enqueue() -> the first non-zero status of the thin calls (0: all went in); verify(k, want) reads back and
    asserts. status_ws: workspaces whose status word must be clear after every round."""

    def __init__(self, load, enqueue, verify, status_ws=()):
        self._load, self.enqueue, self._verify, self.status_ws = load, enqueue, verify, status_ws
        self.want = None

    def load(self, k):
        self.want = self._load(k)

    def verify(self, k):
        self._verify(k, self.want)


def run_protocol(dev, case, replays=3, before_capture=None):
    """Steps 2 to 6 of the protocol; round 0 is the eager warm-up, rounds 1 .. replays the replays, round replays + 1
    the eager call afterwards. Returns nothing: it asserts."""
    lib, q = _lib(), dev[2]
    stream = q.stream

    def finish(k, how):
        st = lib.clo_hip_stream_synchronize(stream)
        assert st == 0, "%s, round %d: the stream ended with status %d" % (how, k, st)
        for ws in case.status_ws:
            st = lib.clo_hip_check_status(ws.ptr, stream)
            assert st == 0, "%s, round %d: clo_hip_check_status = %d" % (how, k, st)
        case.verify(k)

    case.load(0)
    st = case.enqueue()
    assert st == 0, "eager call: status %d (%s)" % (st, lib.clo_hip_error_string(st))
    finish(0, "eager")
    if before_capture:
        before_capture()
    case.load(1)                               # (the captured calls do not run; the buffers hold round 1 for the first replay)
    st = lib.clo_hip_stream_synchronize(stream)
    assert st == 0
    graph = _VP()
    st = lib.clo_hip_graph_capture_begin(stream)
    assert st == 0, "clo_hip_graph_capture_begin: %d" % st
    st_call = case.enqueue()
    st_end = lib.clo_hip_graph_capture_end(stream, C.byref(graph))
    try:
        assert st_call == 0, "status %d under capture (%s)" % (st_call, lib.clo_hip_error_string(st_call))
        assert st_end == 0, "clo_hip_graph_capture_end: %d (%s)" % (st_end, lib.clo_hip_error_string(st_end))
        assert graph.value
        for k in range(1, replays + 1):
            if k > 1:
                case.load(k)
            st = lib.clo_hip_graph_launch(graph, stream)
            assert st == 0, "clo_hip_graph_launch, replay %d: %d" % (k, st)
            finish(k, "replay")
    finally:
        lib.clo_hip_stream_synchronize(stream)
        if graph.value:
            lib.clo_hip_graph_destroy(graph)
    case.load(replays + 1)
    st = case.enqueue()
    assert st == 0, "eager call after the replays: status %d" % st
    finish(replays + 1, "eager after the replays")


def rounds(kinds, replays=3):
    """The distribution of every round: the eager calls take the first, the replays walk through all of them."""
    return [kinds[0]] + [kinds[i % len(kinds)] for i in range(replays)] + [kinds[0]]


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_radix_sort
# ---------------------------------------------------------------------------------------------------------------------

SORT_KINDS = ["random", "equal", "sorted"]      # (test_gpu_sort_by_key.make_keys: uniform, all equal, already sorted)
_KIND = {"uint": 0, "int": 1, "float": 2, "ulong": 0}


def sort_input(etype, n, seed, kind):
    """(elements, their stable order). ulong: a 32-bit key field at bit 32 over value = index."""
    if etype == "ulong":
        key = SBK.make_keys("uint", n, seed, kind)
        a = (key.astype(np.uint64) << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        return a, np.argsort(SBK.order_key(key, "uint"), kind="stable")
    a = SBK.make_keys(etype, n, seed, kind)
    return a, np.argsort(SBK.order_key(a, etype), kind="stable")


# (element type, n, digit bits, CLO_RADIX_SWEEP, in place, views one element past a 256-byte boundary)
_RS = [("uint", n, db, None, False, False) for n in (16384, 16385, 70001, (1 << 20) + 3) for db in (4, 8)]
_RS += [("uint", n, db, "0", False, False) for n in (70001, (1 << 20) + 3) for db in (4, 8)]
_RS += [("int", 70001, 4, None, False, False), ("float", 70001, 4, None, False, False), ("float", 70001, 8, "0", False, False),
        ("int", 70001, 8, "0", True, False)]
_RS += [("ulong", 70001, 4, None, False, False), ("ulong", (1 << 20) + 3, 4, None, False, False), ("ulong", 70001, 8, "0", True, False)]
_RS += [("uint", 16384, 4, None, True, False), ("uint", 70001, 4, None, True, False), ("uint", (1 << 20) + 3, 8, "0", True, False)]
_RS += [("uint", 70001, 4, None, False, True), ("uint", 70001, 4, "0", False, True), ("ulong", 8191, 4, None, False, True)]


@pytest.mark.parametrize("etype,n,digit_bits,sweep,inplace,view", _RS)
def test_radix_sort(dev, mem, library_switches, etype, n, digit_bits, sweep, inplace, view):
    """The one-launch sort, the single-sweep passes and (CLO_RADIX_SWEEP=0, honoured by the thin entry through
    clo_hip_env_refresh) the chain-free passes: the path is chosen on the host when the call is enqueued, and the
    replays sort new contents on it."""
    lib = _lib()
    library_switches(sweep)
    dt = np.dtype(np.uint64 if etype == "ulong" else SBK._NP[etype])
    es = dt.itemsize
    shift, bits = (32, 32) if etype == "ulong" else (0, 32)
    polls = lib.clo_hip_radix_polls(n, es, digit_bits)
    if sweep == "0":
        assert polls == 0, "CLO_RADIX_SWEEP=0 did not reach the thin entry"
    elif n in (16385, 70001) and es == 4:
        assert polls == 1, "expected the single-sweep passes"
    off = (256 + es) if view else 0                        # one element past a 256-byte boundary of a 256-byte aligned allocation
    room = n * es + (512 if view else 0)
    src = mem(room)
    dst = src if inplace else mem(room)
    tmp = mem(n * es)
    wsb = lib.clo_hip_radix_workspace_bytes(n, es, bits, digit_bits)
    assert wsb > 0
    ws = mem(wsb)
    ws.fill(0)
    kinds = rounds(SORT_KINDS)
    sent = {}

    def load(k):
        a, order = sort_input(etype, n, 1000 * k + n % 977 + digit_bits, kinds[k])
        sent[k] = a
        if not inplace:
            dst.fill()
        tmp.fill()
        src.put(a, off)
        return a[order]

    def enqueue():
        return lib.clo_hip_radix_sort(src.ptr + off, dst.ptr + off, tmp.ptr, n, es, shift, bits, _KIND[etype], digit_bits,
                                      ws.ptr, wsb, dev[2].stream)

    def verify(k, want):
        tag = "%s n=%d round %d (%s)" % (etype, n, k, kinds[k])
        same(dst.get(dt, n, off), want, tag)
        if not inplace:
            same(src.get(dt, n, off), sent[k], tag + ": input")
            if view:
                same(dst.get(np.uint8, off), canary(np.uint8, off), tag + ": bytes below the view")
                same(dst.get(np.uint8, room - off - n * es, off + n * es), canary(np.uint8, room - off - n * es), tag + ": bytes above the view")

    run_protocol(dev, Case(load, enqueue, verify, status_ws=(ws,) if polls else ()))


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_radix_sort_kv
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [8193, (1 << 20) + 3])
@pytest.mark.parametrize("mode", ["values", "argsort without keys_out"])
def test_radix_sort_kv(dev, mem, n, mode):
    """Pack / sort / unpack at 8193 pairs, the passes that read and write the caller's arrays at 2^20 + 3."""
    lib, E = _lib(), dev[3]
    given = mode == "values"
    kin, vin, kout, vout = mem(4 * n), mem(4 * n), mem(4 * n), mem(4 * n)
    pa, pb = mem(8 * n), mem(8 * n)
    wsb = E.kv_ws(n, 4, 32, 4)
    assert wsb > 0
    ws = mem(wsb)
    ws.fill(0)
    polls = lib.clo_hip_radix_polls(n, 8, 4)
    kinds = rounds(SORT_KINDS)
    sent = {}

    def load(k):
        keys, order = sort_input("uint", n, 7000 * k + n % 911, kinds[k])
        values = np.random.default_rng(k + n).integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
        sent[k] = (keys, values)
        for b in (kout, vout, pa, pb):
            b.fill()
        kin.put(keys)
        vin.put(values)
        return keys[order], (values[order] if given else order.astype(np.uint32))

    def enqueue():
        return E.sort_kv(kin.ptr, vin.ptr if given else None, kout.ptr if given else None, vout.ptr, pa.ptr, pb.ptr, n, 4, 0, 32, 0, 4,
                         ws.ptr, wsb, dev[2].stream)

    def verify(k, want):
        tag = "n=%d %s round %d (%s)" % (n, mode, k, kinds[k])
        same(vout.get(np.uint32, n), want[1], tag + ": values")
        same(kout.get(np.uint32, n), want[0] if given else canary(np.uint32, n), tag + ": keys")
        same(kin.get(np.uint32, n), sent[k][0], tag + ": keys in")
        same(vin.get(np.uint32, n), sent[k][1], tag + ": values in")

    run_protocol(dev, Case(load, enqueue, verify, status_ws=(ws,) if polls else ()))


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_radix_sort_segmented
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout,key_bits", [("back to back", 24), ("4 pieces per segment", 32)])
def test_radix_sort_segmented(dev, mem, layout, key_bits):
    """The host arrays are read when the call is enqueued (they are zeroed right after it here): every replay sorts
    the same segmentation of new contents."""
    lib = _lib()
    n, nseg = 100000, 7
    rng = np.random.default_rng(77)
    cuts = np.sort(rng.integers(0, n + 1, nseg - 1))
    cuts[3] = cuts[2]                                      # an empty segment
    seg_counts = np.diff(np.concatenate(([0], cuts, [n]))).astype(np.int64)
    if layout == "back to back":
        nsrc, pn, po, ps = n, [], [], []
    else:
        # every segment in 4 pieces, the 28 pieces scattered (in a shuffled order, gaps between them) over a larger source
        pn, ps = [], []
        for s, c in enumerate(seg_counts):
            parts = np.diff(np.concatenate(([0], np.sort(rng.integers(0, c + 1, 3)), [c])))
            pn += [int(x) for x in parts]
            ps += [s] * 4
        po = [0] * len(pn)
        at = 13
        for i in rng.permutation(len(pn)):
            po[i] = at
            at += pn[i] + int(rng.integers(1, 2000))
        nsrc = at
    src, a, b = mem(4 * nsrc), mem(4 * n), mem(4 * n)
    wsb = lib.clo_hip_radix_seg_workspace_bytes(n, nseg, 4, 4)
    assert wsb > 0
    ws = mem(wsb)
    ws.fill(0)
    in_b = C.c_int(-1)
    mask = np.uint32((1 << key_bits) - 1)
    kinds = rounds(SORT_KINDS)
    sent = {}

    def load(k):
        x = SBK.make_keys("uint", nsrc, 31 * k + key_bits, kinds[k])
        sent[k] = x
        gathered = x if not pn else np.concatenate([x[po[i]:po[i] + pn[i]] for i in range(len(pn))])
        want = np.empty(n, np.uint32)
        at = 0
        for c in seg_counts:
            seg = gathered[at:at + c]
            want[at:at + c] = seg[np.argsort(seg & mask, kind="stable")]
            at += c
        a.fill()
        b.fill()
        src.put(x)
        return want

    def enqueue():
        sc = (_SZ * nseg)(*[int(c) for c in seg_counts])
        npc = len(pn)
        pieces = ((_SZ * npc)(*pn), (_SZ * npc)(*po), (_CI * npc)(*ps)) if npc else (None, None, None)
        in_b.value = -1
        st = lib.clo_hip_radix_sort_segmented(src.ptr, a.ptr, b.ptr, n, sc, nseg, pieces[0], pieces[1], pieces[2], npc, 4, 0, key_bits, 4,
                                              ws.ptr, wsb, dev[2].stream, C.byref(in_b))
        for arr in (sc,) + (pieces if npc else ()):       # consumed: a replay cannot look at them again
            C.memset(arr, 0, C.sizeof(arr))
        return st

    def verify(k, want):
        assert in_b.value == ((key_bits + 7) // 8) % 2
        same((b if in_b.value else a).get(np.uint32, n), want, "%s round %d (%s)" % (layout, k, kinds[k]))
        same(src.get(np.uint32, nsrc), sent[k], "%s round %d: source" % (layout, k))

    run_protocol(dev, Case(load, enqueue, verify))


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_scan_exclusive, the epoch wrap, two graphs on one workspace, the chunk chain
# ---------------------------------------------------------------------------------------------------------------------

SCAN_KINDS = ["full range", "small", "ones and zeros"]


def scan_values(et, n, seed, kind):
    rng = np.random.default_rng(seed)
    dt = np.dtype(_NP[et])
    info = np.iinfo(dt)
    if kind == "full range":                               # (uint sums wrap within a few elements)
        return rng.integers(info.min, info.max, n, dtype=dt, endpoint=True)
    if kind == "small":
        return rng.integers(max(info.min, -100), 100, n).astype(dt)
    return rng.integers(0, 2, n).astype(dt)


def scan_case(dev, mem, et, st, n, ws, wsb, seed, kinds):
    """The Case of one clo_hip_scan_exclusive of n elements on the workspace `ws` (initialised by the caller)."""
    lib = _lib()
    edt, sdt = np.dtype(_NP[et]), np.dtype(_NP[st])
    src, dst = mem(n * edt.itemsize), mem(n * sdt.itemsize)
    sent = {}

    def load(k):
        a = scan_values(et, n, seed + 17 * k, kinds[k])
        sent[k] = a
        dst.fill()
        src.put(a)
        return O.serial_scan(a, sdt)

    def enqueue():
        return lib.clo_hip_scan_exclusive(src.ptr, dst.ptr, n, edt.itemsize, int(edt.kind == "i"), sdt.itemsize, ws.ptr, wsb, dev[2].stream)

    def verify(k, want):
        tag = "%s -> %s n=%d round %d (%s)" % (et, st, n, k, kinds[k])
        same(dst.get(sdt, n), want, tag)
        same(src.get(edt, n), sent[k], tag + ": input")

    return Case(load, enqueue, verify, status_ws=(ws,))


def scan_workspace(dev, mem, n, es, ss):
    from cl_ops_amd import _hip
    lib = _lib()
    wsb = lib.clo_hip_scan_workspace_bytes(n, es, ss)
    ws = mem(wsb)
    _hip.check(lib.clo_hip_scan_workspace_init(ws.ptr, wsb, dev[2].stream), "clo_hip_scan_workspace_init")
    return ws, wsb


@pytest.mark.parametrize("st", ["uint", "ulong"])
@pytest.mark.parametrize("n", [1, 16385, (1 << 20) + 3])
def test_scan_exclusive(dev, mem, st, n):
    """The epoch of a call is read from the workspace by the kernel: a replay continues from wherever the call before
    it, eager or replayed, left the workspace."""
    ws, wsb = scan_workspace(dev, mem, n, 4, np.dtype(_NP[st]).itemsize)
    try:
        run_protocol(dev, scan_case(dev, mem, "uint", st, n, ws, wsb, n, rounds(SCAN_KINDS)))
    finally:
        _lib().clo_hip_scan_workspace_forget(ws.ptr)


@pytest.mark.parametrize("st", ["uint", "ulong"])
def test_scan_exclusive_across_the_epoch_wrap(dev, mem, st):
    """Six replays from epoch 2^30 - 3: the first runs under the last but one epoch, the second under the last (its
    kernel zeroes the workspace), the others after the wrap."""
    from cl_ops_amd import _hip
    lib = _lib()
    n, start, replays = 70001, (1 << 30) - 3, 6
    assert start + replays + 1 > EPOCH_MAX                 # the replays and the eager call after them cross the wrap
    assert start + 1 < EPOCH_MAX                           # the first replay still lies before it
    ws, wsb = scan_workspace(dev, mem, n, 4, np.dtype(_NP[st]).itemsize)

    def set_epoch():
        _hip.check(lib.clo_hip_scan_workspace_set_epoch(ws.ptr, start, dev[2].stream), "clo_hip_scan_workspace_set_epoch")

    try:
        run_protocol(dev, scan_case(dev, mem, "uint", st, n, ws, wsb, 5, rounds(SCAN_KINDS, replays)), replays=replays,
                     before_capture=set_epoch)
    finally:
        lib.clo_hip_scan_workspace_forget(ws.ptr)


def test_two_scan_graphs_share_a_workspace(dev, mem):
    """Graphs of two sizes (both shapes of look-back entries in one workspace, both under its full byte count),
    replayed A, B, A, B on one stream."""
    lib, q = _lib(), dev[2]
    na, nb = 70001, (1 << 20) + 3
    ws, wsb = scan_workspace(dev, mem, nb, 4, 8)
    kinds = rounds(SCAN_KINDS)
    cases = [scan_case(dev, mem, "uint", "ulong", na, ws, wsb, 1, kinds), scan_case(dev, mem, "uint", "ulong", nb, ws, wsb, 2, kinds)]
    graphs = [_VP(), _VP()]

    def finish(c, k, how):
        assert lib.clo_hip_stream_synchronize(q.stream) == 0
        assert lib.clo_hip_check_status(ws.ptr, q.stream) == 0, (how, k)
        c.verify(k)

    try:
        for c in cases:                                    # eager, both sizes
            c.load(0)
            assert c.enqueue() == 0
            finish(c, 0, "eager")
        statuses = []
        for c, g in zip(cases, graphs):
            c.load(1)
            assert lib.clo_hip_stream_synchronize(q.stream) == 0
            assert lib.clo_hip_graph_capture_begin(q.stream) == 0
            st_call = c.enqueue()
            statuses.append((st_call, lib.clo_hip_graph_capture_end(q.stream, C.byref(g))))
        assert statuses == [(0, 0), (0, 0)], statuses
        for k in (1, 2):
            for c, g in zip(cases, graphs):                # A, B, A, B
                if k > 1:
                    c.load(k)
                assert lib.clo_hip_graph_launch(g, q.stream) == 0
                finish(c, k, "replay")
        for c in cases:
            c.load(3)
            assert c.enqueue() == 0
            finish(c, 3, "eager after the replays")
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for g in graphs:
            if g.value:
                lib.clo_hip_graph_destroy(g)
        lib.clo_hip_scan_workspace_forget(ws.ptr)


@pytest.mark.parametrize("et,st", [("uint", "uint"), ("uint", "ulong"), ("int", "long")])
def test_scan_in_chunks_with_device_carry_and_reduce_in_one_graph(dev, mem, et, st):
    """The chunk chain of test_gpu_parity.test_scan_in_chunks_with_device_carry_and_reduce and clo_hip_reduce_sum in
    one graph, the carry words zeroed inside it: no host read between the chunks."""
    lib = _lib()
    edt, sdt = np.dtype(_NP[et]), np.dtype(_NP[st])
    n = 70001 + 262144
    cuts = [0, 1, 5000, 5000, 70001, 262144, n]           # includes an empty chunk
    signed = int(edt.kind == "i")
    src, dst, carry, total = mem(n * edt.itemsize), mem(n * sdt.itemsize), mem(16), mem(8)
    ws, wsb = scan_workspace(dev, mem, n, edt.itemsize, sdt.itemsize)
    stream = dev[2].stream
    kinds = rounds(SCAN_KINDS)
    sent = {}

    def load(k):
        a = scan_values(et, n, 3 + 5 * k, kinds[k])
        sent[k] = a
        for b in (dst, carry, total):
            b.fill()
        src.put(a)
        wide = a.astype(np.int64).view(np.uint64)
        return O.serial_scan(a, sdt), int(wide.sum(dtype=np.uint64))

    def chunk(k):
        lo, hi = cuts[k], cuts[k + 1]
        return lambda: lib.clo_hip_scan_exclusive_carry(src.ptr + lo * edt.itemsize, dst.ptr + lo * sdt.itemsize, hi - lo, edt.itemsize, signed,
                                                        sdt.itemsize, carry.ptr + 8 * (k & 1), carry.ptr + 8 * ((k + 1) & 1), ws.ptr, wsb, stream)

    def enqueue():
        return first(lambda: lib.clo_hip_memset_async(carry.ptr, 0, 16, stream),
                     *[chunk(k) for k in range(len(cuts) - 1)],
                     lambda: lib.clo_hip_reduce_sum(src.ptr, n, edt.itemsize, signed, total.ptr, stream))

    def verify(k, want):
        tag = "%s -> %s round %d (%s)" % (et, st, k, kinds[k])
        same(dst.get(sdt, n), want[0], tag)
        assert int(total.get(np.uint64, 1)[0]) == want[1], tag + ": total"
        mask = (1 << (8 * sdt.itemsize)) - 1
        assert int(carry.get(np.uint64, 2)[(len(cuts) - 1) & 1]) & mask == want[1] & mask, tag + ": last carry"
        same(src.get(edt, n), sent[k], tag + ": input")

    try:
        run_protocol(dev, Case(load, enqueue, verify, status_ws=(ws,)))
    finally:
        lib.clo_hip_scan_workspace_forget(ws.ptr)


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_scan_exclusive_typed
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("et", ["float", "half"])
def test_scan_exclusive_typed(dev, mem, et):
    """Every replay is bit-equal to an eager call on the same input and to tests/fscan_model.py (the header: every
    addition in an order fixed by the layout alone, the model restates which). The rounds of small integers have
    exact float sums: they equal the integer scan too."""
    import fscan_model
    lib = _lib()
    n = (1 << 16) + 5
    edt = np.dtype(_NP[et])
    src, out_g, out_e = mem(n * edt.itemsize), mem(4 * n), mem(4 * n)
    wsb = lib.clo_hip_scan_typed_workspace_bytes(n, T_FLOAT)
    ws = mem(max(wsb, 256))
    stream = dev[2].stream
    kinds = rounds(["random", "small integers", "random"])
    sent = {}

    def call(out):
        return lib.clo_hip_scan_exclusive_typed(src.ptr, out.ptr, n, _CLO[et], T_FLOAT, ws.ptr, max(wsb, 256), stream)

    def load(k):
        rng = np.random.default_rng(40 + k)
        ints = rng.integers(0, 4, n)                       # sums below 2^18: exact in float, the elements exact in half
        a = ints.astype(edt) if kinds[k] == "small integers" else (rng.random(n) - 0.25).astype(edt)
        sent[k] = a
        out_g.fill()
        out_e.fill()
        src.put(a)
        want = fscan_model.scan(a, np.float32)
        if kinds[k] == "small integers":
            same(want, O.serial_scan(ints.astype(np.uint32), np.uint32).astype(np.float32), "the model on small integers")
        return want

    def verify(k, want):
        tag = "%s -> float round %d (%s)" % (et, k, kinds[k])
        got = out_g.get(np.float32, n)
        assert call(out_e) == 0 and lib.clo_hip_stream_synchronize(stream) == 0     # the eager call on the same input
        same(got, out_e.get(np.float32, n), tag + ": replay against eager")
        assert got[0] == 0.0 and not np.array_equal(got.view(np.uint8), canary(np.float32, n).view(np.uint8)), tag
        same(got, want, tag + ": the model's sums" + (", which are exact" if kinds[k] == "small integers" else ""))
        same(src.get(edt, n), sent[k], tag + ": input")

    run_protocol(dev, Case(load, lambda: call(out_g), verify))


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_reduce_by_key, clo_hip_scan_by_key
# ---------------------------------------------------------------------------------------------------------------------

RUN_KINDS = ["random runs", "run length 1", "one run"]
_OPS = {"sum": 0, "min": 1, "max": 2}


def run_keys(n, seed, kind):
    rng = np.random.default_rng(seed)
    if kind == "run length 1":
        return (np.arange(n, dtype=np.uint32) * np.uint32(2654435761)) ^ np.uint32(seed)    # (odd multiplier: neighbours differ)
    if kind == "one run":
        return np.full(n, 0xDEAD0000 + seed, np.uint32)
    heads = rng.random(n) < 0.01
    heads[0] = True
    ids = rng.integers(0, 1 << 32, int(heads.sum()), dtype=np.uint64).astype(np.uint32)
    ids[1:][ids[1:] == ids[:-1]] ^= np.uint32(1)           # neighbouring runs have different keys
    return ids[np.cumsum(heads) - 1]


def by_key_values(vt, n, seed):
    rng = np.random.default_rng(seed)
    if vt == "uint":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)
    return rng.integers(-(1 << 31), 1 << 31, n).astype(np.int32)


_BY_KEY = [("uint", "ulong", "sum"), ("int", "int", "min"), ("int", "int", "max")]


@pytest.mark.parametrize("tiles", ["tile - 1", "tile + 1", "3 tile + 1"])
@pytest.mark.parametrize("vt,st,op", _BY_KEY)
def test_reduce_by_key(dev, mem, vt, st, op, tiles):
    """*num_runs_dev and the rows below it after every replay; the canary from row m on."""
    E = dev[3]
    tile = E.rbk_tile(4, 4)
    assert tile > 1
    n = {"tile - 1": tile - 1, "tile + 1": tile + 1, "3 tile + 1": 3 * tile + 1}[tiles]
    sdt = np.dtype(_NP[st])
    kin, vin, kout, aout, runs = mem(4 * n), mem(4 * n), mem(4 * n), mem(n * sdt.itemsize), mem(8)
    wsb = E.rbk_ws(n)
    ws = mem(max(wsb, 256))
    ws.fill(0)
    kinds = rounds(RUN_KINDS)
    sent = {}

    def load(k):
        keys, values = run_keys(n, 11 * k + 1, kinds[k]), by_key_values(vt, n, 13 * k + 2)
        sent[k] = (keys, values)
        for b in (kout, aout, runs):
            b.fill()
        kin.put(keys)
        vin.put(values)
        return rbk_model.rbk(keys, values, op, sdt)

    def enqueue():
        return E.rbk(kin.ptr, vin.ptr, kout.ptr, aout.ptr, runs.ptr, n, 4, _CLO[vt], _CLO[st], _OPS[op], ws.ptr, max(wsb, 256), dev[2].stream)

    def verify(k, want):
        tag = "%s n=%d round %d (%s)" % (op, n, k, kinds[k])
        wk, wa, m = want
        assert int(runs.get(np.uint64, 1)[0]) == m, tag + ": number of runs"
        gk, ga = kout.get(np.uint32, n), aout.get(sdt, n)
        same(gk[:m], wk, tag + ": keys")
        same(ga[:m], wa, tag + ": aggregates")
        same(gk[m:], canary(np.uint32, n - m), tag + ": key rows from m on")
        same(ga[m:], canary(sdt, n - m), tag + ": aggregate rows from m on")
        same(kin.get(np.uint32, n), sent[k][0], tag + ": keys in")
        same(vin.get(_NP[vt], n), sent[k][1], tag + ": values in")

    run_protocol(dev, Case(load, enqueue, verify))


@pytest.mark.parametrize("tiles", ["tile - 1", "tile + 1", "3 tile + 1"])
@pytest.mark.parametrize("vt,st,op,inclusive", [("uint", "ulong", "sum", 0), ("uint", "ulong", "sum", 1), ("int", "int", "min", 0),
                                                ("int", "int", "min", 1), ("int", "int", "max", 0), ("int", "int", "max", 1)])
def test_scan_by_key(dev, mem, vt, st, op, inclusive, tiles):
    E = dev[3]
    tile = E.sbk_tile(4, 4)
    assert tile > 1
    n = {"tile - 1": tile - 1, "tile + 1": tile + 1, "3 tile + 1": 3 * tile + 1}[tiles]
    sdt = np.dtype(_NP[st])
    kin, vin, out = mem(4 * n), mem(4 * n), mem(n * sdt.itemsize)
    wsb = E.sbk_ws(n)
    ws = mem(max(wsb, 256))
    ws.fill(0)
    kinds = rounds(RUN_KINDS)
    sent = {}

    def load(k):
        keys, values = run_keys(n, 7 * k + 3, kinds[k]), by_key_values(vt, n, 5 * k + 4)
        sent[k] = (keys, values)
        out.fill()
        kin.put(keys)
        vin.put(values)
        return sbk_model.sbk(keys, values, op, sdt, bool(inclusive))

    def enqueue():
        return E.sbk(kin.ptr, vin.ptr, out.ptr, n, 4, _CLO[vt], _CLO[st], _OPS[op], inclusive, ws.ptr, max(wsb, 256), dev[2].stream)

    def verify(k, want):
        tag = "%s inclusive=%d n=%d round %d (%s)" % (op, inclusive, n, k, kinds[k])
        same(out.get(sdt, n), want, tag)
        same(kin.get(np.uint32, n), sent[k][0], tag + ": keys in")
        same(vin.get(_NP[vt], n), sent[k][1], tag + ": values in")

    run_protocol(dev, Case(load, enqueue, verify))


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_histogram
# ---------------------------------------------------------------------------------------------------------------------

HIST_KINDS = ["uniform", "90 % in one bin", "outside the range"]
HIST_LOWER, HIST_SHIFT = 1000, 3


def hist_keys(n, num_bins, seed, kind):
    rng = np.random.default_rng(seed)
    span = num_bins << HIST_SHIFT
    if kind == "outside the range":                        # below the lower bound, and from the end of the last bin on
        below = rng.integers(0, HIST_LOWER, n)
        above = rng.integers(HIST_LOWER + span, 1 << 32, n)
        return np.where(rng.random(n) < 0.5, below, above).astype(np.uint32)
    keys = rng.integers(HIST_LOWER, HIST_LOWER + span, n)
    if kind == "90 % in one bin":
        b = int(rng.integers(0, num_bins))
        one = HIST_LOWER + (b << HIST_SHIFT) + rng.integers(0, 1 << HIST_SHIFT, n)
        keys = np.where(rng.random(n) < 0.9, one, keys)
    return keys.astype(np.uint32)


def hist_setup(dev, mem, what, bins):
    """(n, number of bins, sum dtype, with values?) for counts in uint or uint -> ulong sums."""
    E = dev[3]
    sdt = np.dtype(np.uint32 if what == "counts" else np.uint64)
    tile = E.hist_tile(4, 0 if what == "counts" else 4)
    lds = E.hist_lds_bins(sdt.itemsize)
    assert tile > 0 and lds > 256
    num_bins = {"256": 256, "lds_bins": lds, "lds_bins + 1": lds + 1}[bins]
    return 3 * tile + 1, num_bins, sdt, what != "counts"


@pytest.mark.parametrize("bins", ["256", "lds_bins", "lds_bins + 1"])
@pytest.mark.parametrize("what", ["counts", "sums"])
def test_histogram(dev, mem, what, bins):
    """accumulate 0: the fill that zeroes hist_out is a node of the graph, every replay overwrites the canary."""
    E = dev[3]
    n, num_bins, sdt, valued = hist_setup(dev, mem, what, bins)
    kin, vin, out = mem(4 * n), mem(4 * n), mem(num_bins * sdt.itemsize)
    kinds = rounds(HIST_KINDS)
    sent = {}

    def load(k):
        keys = hist_keys(n, num_bins, 3 * k + num_bins, kinds[k])
        values = by_key_values("uint", n, k + 9)
        sent[k] = (keys, values)
        out.fill()
        kin.put(keys)
        vin.put(values)
        return hist_model.histogram(keys, values if valued else None, sdt, HIST_LOWER, HIST_SHIFT, num_bins)

    def enqueue():
        return E.hist(kin.ptr, vin.ptr if valued else None, out.ptr, n, 4, 0, T_UINT, _CLO["uint" if sdt.itemsize == 4 else "ulong"],
                      HIST_LOWER, HIST_SHIFT, num_bins, 0, 0, None, 0, dev[2].stream)

    def verify(k, want):
        tag = "%s %d bins round %d (%s)" % (what, num_bins, k, kinds[k])
        if kinds[k] == "outside the range":
            assert not want.any()
        same(out.get(sdt, num_bins), want, tag)
        same(kin.get(np.uint32, n), sent[k][0], tag + ": keys")
        same(vin.get(np.uint32, n), sent[k][1], tag + ": values")

    run_protocol(dev, Case(load, enqueue, verify))


@pytest.mark.parametrize("bins", ["256", "lds_bins", "lds_bins + 1"])
@pytest.mark.parametrize("what", ["counts", "sums"])
def test_histogram_accumulates_across_replays(dev, mem, what, bins):
    """accumulate 1 on the same data: after k replays hist_out is the prefill plus k times the histogram, modulo the
    sum type; the eager calls before and after add once each."""
    lib, E, q = _lib(), dev[3], dev[2]
    n, num_bins, sdt, valued = hist_setup(dev, mem, what, bins)
    kin, vin, out = mem(4 * n), mem(4 * n), mem(num_bins * sdt.itemsize)
    keys, values = hist_keys(n, num_bins, num_bins, "90 % in one bin"), by_key_values("uint", n, 1)
    rng = np.random.default_rng(6)
    prefill = rng.integers(0, 1 << 32, num_bins, dtype=np.uint64).astype(sdt)
    prefill[::3] = np.iinfo(sdt).max                       # (these bins wrap with the first element added)
    kin.put(keys)
    vin.put(values)
    model = lambda onto: hist_model.histogram(keys, values if valued else None, sdt, HIST_LOWER, HIST_SHIFT, num_bins, onto=onto)

    def enqueue():
        return E.hist(kin.ptr, vin.ptr if valued else None, out.ptr, n, 4, 0, T_UINT, _CLO["uint" if sdt.itemsize == 4 else "ulong"],
                      HIST_LOWER, HIST_SHIFT, num_bins, 1, 0, None, 0, q.stream)

    def finish(want, how):
        assert lib.clo_hip_stream_synchronize(q.stream) == 0
        same(out.get(sdt, num_bins), want, "%s %d bins, %s" % (what, num_bins, how))

    out.put(prefill)
    assert enqueue() == 0
    want = model(prefill)
    finish(want, "eager")
    out.put(prefill)
    want = prefill
    assert lib.clo_hip_stream_synchronize(q.stream) == 0
    graph = _VP()
    assert lib.clo_hip_graph_capture_begin(q.stream) == 0
    st_call = enqueue()
    st_end = lib.clo_hip_graph_capture_end(q.stream, C.byref(graph))
    try:
        assert (st_call, st_end) == (0, 0), (st_call, st_end)
        for k in (1, 2, 3):
            assert lib.clo_hip_graph_launch(graph, q.stream) == 0
            want = model(want)
            finish(want, "replay %d" % k)
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        if graph.value:
            lib.clo_hip_graph_destroy(graph)
    assert enqueue() == 0
    finish(model(want), "eager after the replays")
    same(kin.get(np.uint32, n), keys, "keys")
    same(vin.get(np.uint32, n), values, "values")


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_rng_fill
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", M.NAMES)
def test_rng_fill(dev, mem, name):
    """The states live in device memory and advance with every fill: three replays give draws 1 - 5, 6 - 10 and
    11 - 15 of every state, and the states read back are the model's."""
    lib, E, q = _lib(), dev[3], dev[2]
    S, draws = 4096, 5
    numel = S * draws
    gen = M.NAMES.index(name)
    seeded = M.dev_gid_states(name, S, 12345)
    raw = np.ascontiguousarray(seeded).view(np.uint8)
    states, out = mem(raw.size), mem(4 * numel)
    assert raw.size == S * M.SEED_SIZE[name]

    def enqueue():
        return E.rng_fill(gen, states.ptr, S, out.ptr, numel, 32, 0, 0, q.stream)

    def finish(st, how):
        want, st = M.fill(name, st, numel)
        assert lib.clo_hip_stream_synchronize(q.stream) == 0
        same(out.get(np.uint32, numel), want, "%s, %s" % (name, how))
        same(M.state_from_bytes(name, states.get(np.uint8, raw.size), S), st, "%s, %s: states" % (name, how))
        return st

    states.put(raw)
    out.fill()
    assert enqueue() == 0
    finish(seeded, "eager")
    states.put(raw)                                        # back to the seeds: the replays draw from the start
    assert lib.clo_hip_stream_synchronize(q.stream) == 0
    graph = _VP()
    assert lib.clo_hip_graph_capture_begin(q.stream) == 0
    st_call = enqueue()
    st_end = lib.clo_hip_graph_capture_end(q.stream, C.byref(graph))
    st = seeded
    try:
        assert (st_call, st_end) == (0, 0), (st_call, st_end)
        for k in (1, 2, 3):
            out.fill()
            assert lib.clo_hip_graph_launch(graph, q.stream) == 0
            st = finish(st, "replay %d (draws %d - %d)" % (k, 5 * k - 4, 5 * k))
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        if graph.value:
            lib.clo_hip_graph_destroy(graph)
    out.fill()
    assert enqueue() == 0
    finish(st, "eager after the replays (draws 16 - 20)")


# ---------------------------------------------------------------------------------------------------------------------
# bitonic sorts and gselect
# ---------------------------------------------------------------------------------------------------------------------

def shifted_input(n, seed, kind, shift):
    """uint elements with few distinct keys above `shift` (ties show) over random low bits."""
    rng = np.random.default_rng(seed)
    key = {"random": rng.integers(0, 50, n), "equal": np.full(n, 7), "sorted": np.sort(rng.integers(0, 50, n))}[kind]
    return ((key.astype(np.uint32) << np.uint32(shift)) | rng.integers(0, 1 << shift, n).astype(np.uint32)).astype(np.uint32)


@pytest.mark.parametrize("shift", [0, 16])
def test_bitonic_tiled(dev, mem, shift):
    """2^15 uint in place; with the key above bit 16 the tie order is the restated reference network's."""
    lib = _lib()
    n = 1 << 15
    data = mem(4 * lib.clo_hip_bitonic_padded_numel(n))
    launches = C.c_int(0)
    kinds = rounds(SORT_KINDS)

    def load(k):
        a = SBK.make_keys("uint", n, 50 + k, kinds[k]) if shift == 0 else shifted_input(n, 50 + k, kinds[k], shift)
        data.put(a)
        return np.sort(a, kind="stable") if shift == 0 else O.sbitonic(a, key_shift=shift)

    def enqueue():
        return lib.clo_hip_bitonic_tiled(data.ptr, n, 4, shift, 32 - shift, 4, 0, 0, C.byref(launches), dev[2].stream)

    def verify(k, want):
        same(data.get(np.uint32, n), want, "shift %d round %d (%s)" % (shift, k, kinds[k]))

    run_protocol(dev, Case(load, enqueue, verify))


def test_bitonic_any(dev, mem):
    """5000 uint by the key above bit 16, in place (see the head of this file: the key sequence, a permutation of the
    input, and the bits of an eager call on the same input)."""
    lib = _lib()
    n, shift = 5000, 16
    data, eager = mem(4 * n), mem(4 * n)
    stream = dev[2].stream
    kinds = rounds(SORT_KINDS)
    sent = {}

    def call(buf):
        return lib.clo_hip_bitonic_any(buf.ptr, n, 4, shift, 32 - shift, 4, 0, 0, None, stream)

    def load(k):
        a = shifted_input(n, 90 + k, kinds[k], shift)
        sent[k] = a
        data.put(a)
        return np.sort(a >> np.uint32(shift), kind="stable")

    def verify(k, want):
        tag = "round %d (%s)" % (k, kinds[k])
        got = data.get(np.uint32, n)
        same(got >> np.uint32(shift), want, tag + ": keys")
        same(np.sort(got), np.sort(sent[k]), tag + ": not a permutation of the input")
        eager.put(sent[k])
        assert call(eager) == 0 and lib.clo_hip_stream_synchronize(stream) == 0
        same(got, eager.get(np.uint32, n), tag + ": against the eager call")

    run_protocol(dev, Case(load, lambda: call(data), verify))


def test_gselect(dev, mem):
    lib, E = _lib(), dev[3]
    n, shift = 2049, 16
    src, dst = mem(4 * n), mem(4 * n)
    kinds = rounds(SORT_KINDS)
    sent = {}

    def load(k):
        a = shifted_input(n, 20 + k, kinds[k], shift)
        sent[k] = a
        dst.fill()
        src.put(a)
        want = a[np.argsort(a >> np.uint32(shift), kind="stable")]
        same(want, O.gselect(a, key_shift=shift), "the two models")
        return want

    def enqueue():
        return E.gselect(src.ptr, dst.ptr, n, 4, shift, 32 - shift, 4, 0, 0, dev[2].stream)

    def verify(k, want):
        same(dst.get(np.uint32, n), want, "round %d (%s)" % (k, kinds[k]))
        same(src.get(np.uint32, n), sent[k], "round %d: input" % k)

    run_protocol(dev, Case(load, enqueue, verify))


# ---------------------------------------------------------------------------------------------------------------------
# clo_hip_msd_histogram + clo_hip_msd_partition
# ---------------------------------------------------------------------------------------------------------------------

def test_msd_histogram_and_partition(dev, mem):
    """Both in one graph, the bucket sizes on the device (each entry zeroes or overwrites its own)."""
    lib = _lib()
    n, bits = 200003, 3
    src, dst, cnt, cnt2 = mem(4 * n), mem(4 * n), mem(8 << bits), mem(8 << bits)
    wsb = lib.clo_hip_msd_workspace_bytes(n, 4, bits)
    assert wsb > 0
    ws = mem(wsb)
    ws.fill(0)
    stream = dev[2].stream
    kinds = rounds(SORT_KINDS)
    sent = {}

    def load(k):
        a = SBK.make_keys("uint", n, 60 + k, kinds[k])
        if kinds[k] == "equal":
            a = np.full(n, 0xA0000000 + k, np.uint32)     # (one bucket that is not the first)
        sent[k] = a
        for b in (dst, cnt, cnt2):
            b.fill()
        src.put(a)
        bucket = (a >> np.uint32(32 - bits)).astype(np.int64)
        return a[np.argsort(bucket, kind="stable")], np.bincount(bucket, minlength=1 << bits).astype(np.uint64)

    def enqueue():
        return first(lambda: lib.clo_hip_msd_histogram(src.ptr, n, 4, 0, 32, bits, cnt.ptr, stream),
                     lambda: lib.clo_hip_msd_partition(src.ptr, dst.ptr, n, 4, 0, 32, bits, cnt2.ptr, ws.ptr, wsb, stream))

    def verify(k, want):
        tag = "round %d (%s)" % (k, kinds[k])
        same(dst.get(np.uint32, n), want[0], tag)
        same(cnt.get(np.uint64, 1 << bits), want[1], tag + ": clo_hip_msd_histogram")
        same(cnt2.get(np.uint64, 1 << bits), want[1], tag + ": the partition's counts")
        same(src.get(np.uint32, n), sent[k], tag + ": input")

    run_protocol(dev, Case(load, enqueue, verify, status_ws=(ws,)))


# ---------------------------------------------------------------------------------------------------------------------
# one pipeline in one graph: no host read between the stages
# ---------------------------------------------------------------------------------------------------------------------

PIPE_N, PIPE_BINS, PIPE_SHIFT = (1 << 18) + 3, 4096, 3
PIPE_KINDS = ["uniform", "90 % in one bin", "sorted"]
# device arrays of the pipeline: (name, bytes)
PIPE_ARRAYS = [("keys", 4 * PIPE_N), ("counts", 4 * PIPE_BINS), ("offsets", 4 * PIPE_BINS), ("sorted", 4 * PIPE_N), ("order", 4 * PIPE_N),
               ("pa", 8 * PIPE_N), ("pb", 8 * PIPE_N), ("uniq", 4 * PIPE_N), ("lens", 4 * PIPE_N), ("runs", 8), ("rank", 4 * PIPE_N)]
PIPE_OUTPUTS = ["counts", "offsets", "sorted", "order", "uniq", "lens", "runs", "rank"]


def pipe_sizes(E):
    lib = _lib()
    return {"scan": lib.clo_hip_scan_workspace_bytes(PIPE_BINS, 4, 4), "sort": E.kv_ws(PIPE_N, 4, 32, 4),
            "rbk": max(E.rbk_ws(PIPE_N), 256), "sbk": max(E.sbk_ws(PIPE_N), 256)}


def pipe_keys(seed, kind):
    """Keys with about eight duplicates each, one in 16 beyond the last bin."""
    rng = np.random.default_rng(seed)
    span = PIPE_BINS << PIPE_SHIFT
    keys = rng.integers(0, span, PIPE_N)
    if kind == "90 % in one bin":
        keys = np.where(rng.random(PIPE_N) < 0.9, (1234 << PIPE_SHIFT) + rng.integers(0, 1 << PIPE_SHIFT, PIPE_N), keys)
    keys = np.where(rng.random(PIPE_N) < 1 / 16, rng.integers(span, 1 << 32, PIPE_N), keys).astype(np.uint32)
    return np.sort(keys) if kind == "sorted" else keys


def pipe_model(keys):
    counts = hist_model.histogram(keys, None, np.uint32, 0, PIPE_SHIFT, PIPE_BINS)
    order = np.argsort(SBK.order_key(keys, "uint"), kind="stable")
    uniq, lens, m = rbk_model.rbk(keys[order], None, "sum", np.uint32)
    return {"counts": counts, "offsets": O.serial_scan(counts, np.uint32), "sorted": keys[order], "order": order.astype(np.uint32),
            "uniq": uniq, "lens": lens, "runs": np.array([m], np.uint64), "rank": sbk_model.sbk(keys[order], None, "sum", np.uint32, False)}


def pipe_enqueue(E, p, w, wb, stream):
    """p: device pointers by name; w, wb: the four workspaces and their sizes."""
    lib = _lib()
    n = PIPE_N
    return first(
        lambda: E.hist(p["keys"], None, p["counts"], n, 4, 0, T_UINT, T_UINT, 0, PIPE_SHIFT, PIPE_BINS, 0, 0, None, 0, stream),
        lambda: lib.clo_hip_scan_exclusive(p["counts"], p["offsets"], PIPE_BINS, 4, 0, 4, w["scan"], wb["scan"], stream),
        lambda: E.sort_kv(p["keys"], None, p["sorted"], p["order"], p["pa"], p["pb"], n, 4, 0, 32, 0, 4, w["sort"], wb["sort"], stream),
        lambda: E.rbk(p["sorted"], None, p["uniq"], p["lens"], p["runs"], n, 4, T_UINT, T_UINT, 0, w["rbk"], wb["rbk"], stream),
        lambda: E.sbk(p["sorted"], None, p["rank"], n, 4, T_UINT, T_UINT, 0, 0, w["sbk"], wb["sbk"], stream))


def pipe_check(got, want, keys_back, keys, tag):
    """got: name -> bytes read back (uint8)."""
    m = int(want["runs"][0])
    for name in PIPE_OUTPUTS:
        g = got[name].view(want[name].dtype)
        if name in ("uniq", "lens"):
            same(g[:m], want[name], tag + ": " + name)
            same(g[m:], canary(np.uint32, PIPE_N - m), tag + ": " + name + " from row m on")
        else:
            same(g, want[name], tag + ": " + name)
    same(keys_back, keys, tag + ": keys")


def test_pipeline_in_one_graph(dev, mem):
    """histogram -> scan of the counts, and on the same keys argsort -> run lengths -> rank within the run."""
    from cl_ops_amd import _hip
    lib, E = _lib(), dev[3]
    stream = dev[2].stream
    arr = {name: mem(nbytes) for name, nbytes in PIPE_ARRAYS}
    wb = pipe_sizes(E)
    w = {name: mem(nbytes) for name, nbytes in wb.items()}
    for name in ("sort", "rbk", "sbk"):
        w[name].fill(0)
    _hip.check(lib.clo_hip_scan_workspace_init(w["scan"].ptr, wb["scan"], stream), "clo_hip_scan_workspace_init")
    p = {name: b.ptr for name, b in arr.items()}
    wp = {name: b.ptr for name, b in w.items()}
    kinds = rounds(PIPE_KINDS)
    sent = {}

    def load(k):
        keys = pipe_keys(70 + k, kinds[k])
        sent[k] = keys
        for name in PIPE_OUTPUTS + ["pa", "pb"]:
            arr[name].fill()
        arr["keys"].put(keys)
        return pipe_model(keys)

    def verify(k, want):
        got = {name: arr[name].get(np.uint8, arr[name].n) for name in PIPE_OUTPUTS}
        pipe_check(got, want, arr["keys"].get(np.uint32, PIPE_N), sent[k], "round %d (%s)" % (k, kinds[k]))

    polls = lib.clo_hip_radix_polls(PIPE_N, 8, 4)
    try:
        run_protocol(dev, Case(load, lambda: pipe_enqueue(E, p, wp, wb, stream), verify,
                               status_ws=(w["scan"],) + ((w["sort"],) if polls else ())))
    finally:
        lib.clo_hip_scan_workspace_forget(w["scan"].ptr)


def test_pipeline_under_torch_cuda_graph(dev):
    """The same calls on torch tensors, captured by torch.cuda.graph on the stream torch captures on (one stream, no
    forked branches), after a warm-up on a side stream."""
    import torch
    from cl_ops_amd import _hip
    lib, E = _lib(), dev[3]
    torch.cuda.set_device(0)
    t = {name: torch.empty(nbytes, dtype=torch.uint8, device="cuda") for name, nbytes in PIPE_ARRAYS}
    wb = pipe_sizes(E)
    w = {name: torch.zeros(nbytes, dtype=torch.uint8, device="cuda") for name, nbytes in wb.items()}
    p = {name: x.data_ptr() for name, x in t.items()}
    wp = {name: x.data_ptr() for name, x in w.items()}
    assert all(v % 256 == 0 for v in wp.values())
    kinds = rounds(PIPE_KINDS)

    def load(k):
        keys = pipe_keys(170 + k, kinds[k])
        for name in PIPE_OUTPUTS + ["pa", "pb"]:
            t[name].fill_(CANARY)
        t["keys"].copy_(torch.from_numpy(keys.view(np.uint8)))
        return keys, pipe_model(keys)

    def finish(k, keys, want, how):
        torch.cuda.synchronize()
        assert lib.clo_hip_check_status(wp["scan"], torch.cuda.current_stream().cuda_stream) == 0
        got = {name: t[name].cpu().numpy() for name in PIPE_OUTPUTS}
        pipe_check(got, want, t["keys"].cpu().numpy().view(np.uint32), keys, "%s, round %d (%s)" % (how, k, kinds[k]))

    try:
        side = torch.cuda.Stream()
        keys, want = load(0)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                      # the warm-up: code objects load here, not under capture
            _hip.check(lib.clo_hip_scan_workspace_init(wp["scan"], wb["scan"], side.cuda_stream), "clo_hip_scan_workspace_init")
            st = pipe_enqueue(E, p, wp, wb, side.cuda_stream)
        torch.cuda.current_stream().wait_stream(side)
        assert st == 0, "warm-up: status %d" % st
        finish(0, keys, want, "warm-up")
        keys, want = load(1)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            st = pipe_enqueue(E, p, wp, wb, torch.cuda.current_stream().cuda_stream)
        assert st == 0, "status %d under torch.cuda.graph (%s)" % (st, lib.clo_hip_error_string(st))
        for k in (1, 2, 3):
            if k > 1:
                keys, want = load(k)
            g.replay()
            finish(k, keys, want, "replay")
        keys, want = load(4)
        st = pipe_enqueue(E, p, wp, wb, torch.cuda.current_stream().cuda_stream)
        assert st == 0
        finish(4, keys, want, "eager after the replays")
        del g
    finally:
        torch.cuda.synchronize()
        lib.clo_hip_scan_workspace_forget(wp["scan"])
