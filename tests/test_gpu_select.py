"""CloSelect (include/clo_select.h) on the GPU against the numpy model of tests/select_model.py, bit for bit. Every array
is a view inside a larger allocation with 256 guard bytes of a canary pattern on each side (the Region of
test_gpu_histogram.py); the outputs and num_out are pre-filled with the pattern, and after every call num_out is the
model's k, the rows written equal the model's, and the guards, every input and — for a select — every row at index >= k
are unchanged. With T = clo_hip_select_tile: sizes around the tile edges and keep patterns (none, all, alternating, the
first / the last element of every tile, one element at a tile edge, random) for both ops by flags and by comparison;
every op, pred and value form; every key type with its special values and the threshold among the keys; flags other
than 0 / 1; element-aligned views; a tile count that sends the count scan through its loop a second time; a threshold
another kernel wrote just before on the same stream; two objects on two streams; the host-data form; the thin ABI's
status codes; clo_hip_select captured into a linear graph and replayed after the flags and the threshold were
rewritten; and one case with element indices above 2^31 against torch.nonzero."""
import numpy as np
import pytest

from select_model import OPS, PREDS, keep_mask, select
from test_gpu_histogram import Region
from test_gpu_merge import KEY_TYPES, _NP, keys_of_type

pytestmark = pytest.mark.gpu

# value forms: keys only; 4-byte values; 8-byte values; indices with keys_out; indices alone; indices alone without
# keys_in (flagged only)
_VS = {"keys": 0, "v4": 4, "v8": 8, "arg": 4, "arg_only": 4, "arg_no_keys": 4}
MODES = ("keys", "v4", "v8", "arg", "arg_only")


@pytest.fixture(scope="module")
def dev(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    return clo, ctx, q


def tile_of(dev, kt, mode="keys"):
    t = dev[0].select_tile(np.dtype(_NP[kt]).itemsize, _VS[mode])
    assert t > 0 and t % 1024 == 0
    return t


def values_for(mode, n):
    """Values that carry the element's index; the 8-byte ones with a non-zero high word that differs per element."""
    if mode == "v4":
        return np.arange(n, dtype=np.uint32) ^ np.uint32(0x5A000000)
    if mode == "v8":
        i = np.arange(n, dtype=np.uint64)
        return ((np.uint64(0xC0DE0000) + (i * np.uint64(2654435761) & np.uint64(0xFFFF))) << np.uint64(32)) | i
    return None


def run_select(dev, op, pred, kt, keys, fot, mode, what, offs=(0, 0, 0, 0, 0), obj=None, q=None):
    """One call on views at byte offsets offs = (keys_in, values_in, flags or threshold, keys_out, values_out); checks
    everything and returns k. fot: the flag bytes, or the threshold (one key)."""
    clo, ctx, q0 = dev
    q = q or q0
    rdev = (clo, ctx, q)
    dt = np.dtype(_NP[kt])
    keys = np.ascontiguousarray(keys, dtype=dt)
    n, vs = keys.size, _VS[mode]
    fot = np.ascontiguousarray(fot, dtype=np.uint8) if pred == "flagged" else np.array([fot], dtype=dt).reshape(1)
    what = "%s %s %s %s, %s" % (op, pred, kt, mode, what)
    vals = values_for(mode, n)
    s = obj or clo.Select(op, pred, ctx, kt, vs)
    k_r = Region(rdev, keys.nbytes, offs[0], keys, 0) if mode != "arg_no_keys" else None
    v_r = Region(rdev, vals.nbytes, offs[1], vals, 1) if vals is not None else None
    f_r = Region(rdev, fot.nbytes, offs[2], fot, 0)
    ko_r = Region(rdev, n * dt.itemsize, offs[3], None, 2) if mode in ("keys", "v4", "v8", "arg") else None
    vo_r = Region(rdev, n * vs, offs[4], None, 2) if vs else None
    num_r = Region(rdev, 8, 0, None, 1)
    view = lambda r: r.view if r is not None else None
    try:
        assert s.with_device_data(q, view(k_r), view(v_r), f_r.view, view(ko_r), view(vo_r), num_r.view, n), what
        q.finish()
        k = int(num_r.base.read(q, np.uint8, num_r.host.size)[num_r.at:num_r.at + 8].view(np.uint64)[0])
        p, want_k = select(op, pred, keys, fot if pred == "flagged" else fot[0])
        assert k == want_k, "%s: k = %d, the model keeps %d" % (what, k, want_k)
        num_r.check(np.array([k], np.uint64), what + ": num_out")
        if ko_r:
            ko_r.check(keys[p], what + ": keys_out")                   # ... and nothing behind the rows written
        if vo_r:
            vo_r.check(vals[p] if vals is not None else p, what + ": values_out")
        if k_r:
            k_r.check(keys, what + ": keys_in")
        if v_r:
            v_r.check(vals, what + ": values_in")
        f_r.check(fot, what + ": flags_or_threshold")
        return k
    finally:
        for r in (k_r, v_r, f_r, ko_r, vo_r, num_r):
            if r:
                r.close()
        if obj is None:
            s.close()


PATTERNS = ("none", "all", "alternating", "first of every tile", "last of every tile", "one at a tile edge", "p = 0.01", "p = 0.5", "p = 0.99")


def mask_of(pattern, n, T, seed):
    i = np.arange(n)
    if pattern == "none":
        return np.zeros(n, bool)
    if pattern == "all":
        return np.ones(n, bool)
    if pattern == "alternating":
        return i % 2 == 1
    if pattern == "first of every tile":
        return i % T == 0
    if pattern == "last of every tile":
        return (i % T == T - 1) | (i == n - 1)
    if pattern == "one at a tile edge":
        return i == min(T, n - 1) if n else np.zeros(0, bool)       # the first element of the second tile, or the last there is
    return np.random.default_rng(seed).random(n) < float(pattern[4:])


def inputs_for(pred, mask, seed):
    """uint keys and flags_or_threshold under which exactly the elements of the mask are kept. Flags take every value
    of a byte, not 0 / 1 alone."""
    rng = np.random.default_rng(seed)
    n = mask.size
    if pred == "flagged":
        return rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32), np.where(mask, rng.integers(1, 256, n), 0).astype(np.uint8)
    thr = 1 << 20
    lo, hi = rng.integers(0, thr, n, dtype=np.uint64), rng.integers(thr + 1, 1 << 32, n, dtype=np.uint64)
    eq = np.full(n, thr, np.uint64)
    kept, rest = {"lt": (lo, hi), "le": (np.where(rng.random(n) < 0.3, eq, lo), hi), "gt": (hi, lo), "ge": (np.where(rng.random(n) < 0.3, eq, hi), lo),
                  "eq": (eq, np.where(rng.random(n) < 0.5, lo, hi)), "ne": (np.where(rng.random(n) < 0.5, lo, hi), eq)}[pred]
    return np.where(mask, kept, rest).astype(np.uint32), np.uint32(thr)


@pytest.mark.parametrize("pred", ["flagged", "lt"])
@pytest.mark.parametrize("op", OPS)
def test_sizes_and_patterns(dev, op, pred):
    """Sizes 0, 1, 3, T - 1, T, T + 1, 2 T + 5 x the keep patterns; the value forms take turns."""
    case = 0
    for pattern in PATTERNS:
        for which in range(7):
            mode = MODES[case % len(MODES)]
            case += 1
            T = tile_of(dev, "uint", mode)
            n = (0, 1, 3, T - 1, T, T + 1, 2 * T + 5)[which]
            mask = mask_of(pattern, n, T, case)
            keys, fot = inputs_for(pred, mask, 1000 + case)
            k = run_select(dev, op, pred, "uint", keys, fot, mode, "%s, n = %d" % (pattern, n))
            assert k == int(mask.sum())


@pytest.mark.parametrize("pred", PREDS)
@pytest.mark.parametrize("op", OPS)
def test_every_form(dev, op, pred):
    """Both ops x every pred x every value form, three tiles and a bit, about half kept."""
    for j, mode in enumerate(MODES + (("arg_no_keys",) if pred == "flagged" else ())):
        T = tile_of(dev, "uint", mode)
        n = 2 * T + 5
        mask = mask_of("p = 0.5", n, T, 7 + j)
        keys, fot = inputs_for(pred, mask, 70 + j)
        assert run_select(dev, op, pred, "uint", keys, fot, mode, "n = %d" % n) == int(mask.sum())


@pytest.mark.parametrize("kt", KEY_TYPES)
def test_key_types(dev, kt):
    """Comparisons on every key type: few distinct keys that include the type's specials (+-0, +-inf, NaNs of both signs
    and several payloads, the integers' ends), in random order, and thresholds taken from among them."""
    rng = np.random.default_rng(len(kt) * 131 + ord(kt[0]))
    case = 0
    for pred in PREDS[1:]:
        mode = MODES[case % len(MODES)]
        T = tile_of(dev, kt, mode)
        keys = rng.permutation(keys_of_type(kt, 2 * T + 3, 5 + case))
        distinct = keys[np.unique(keys.view("u%d" % keys.dtype.itemsize), return_index=True)[1]]
        for thr in distinct[rng.permutation(distinct.size)[:4]]:
            op = OPS[case % 2]
            case += 1
            k = run_select(dev, op, pred, kt, keys, thr, mode, "threshold with bits %#x" % int(np.array([thr]).view("u%d" % keys.dtype.itemsize)[0]))
            assert k == int(keep_mask(pred, keys, thr).sum())
    # the keys are opaque to a flagged selection
    T = tile_of(dev, kt, "v8")
    keys = rng.permutation(keys_of_type(kt, T + 9, 3))
    flags = (rng.integers(0, 3, keys.size) * 127).astype(np.uint8)
    run_select(dev, "partition", "flagged", kt, keys, flags, "v8", "flags 0, 127, 254")


def test_element_aligned_views(dev):
    """Every array one element past a 16-byte boundary: nothing may assume more than the element's alignment."""
    cases = (("uchar", "v8", (1, 8, 1, 1, 8)), ("char", "arg", (1, 0, 1, 1, 4)), ("ushort", "v4", (2, 4, 1, 2, 4)), ("uint", "keys", (4, 0, 1, 4, 0)),
             ("uint", "v4", (4, 4, 3, 4, 4)), ("float", "arg", (4, 0, 1, 4, 4)), ("ulong", "v8", (8, 8, 1, 8, 8)), ("double", "arg_only", (8, 0, 1, 0, 4)),
             ("half", "keys", (2, 0, 5, 2, 0)), ("uint", "arg_no_keys", (0, 0, 1, 0, 4)))
    for i, (kt, mode, offs) in enumerate(cases):
        T = tile_of(dev, kt, mode)
        keys = np.random.default_rng(i).permutation(keys_of_type(kt, 2 * T + 37, 8 + i))
        flags = np.where(mask_of("p = 0.5", keys.size, T, i), 200, 0).astype(np.uint8)
        for op in OPS:
            run_select(dev, op, "flagged", kt, keys, flags, mode, "flags at %s" % (offs,), offs=offs)
            if mode != "arg_no_keys":
                pred = PREDS[1 + i % 6]
                thr_offs = offs[:2] + (np.dtype(_NP[kt]).itemsize,) + offs[3:]      # the threshold: one key, one element past the boundary
                run_select(dev, op, pred, kt, keys, keys[5], mode, "views at %s" % (thr_offs,), offs=thr_offs)


def test_the_count_scan_takes_a_second_trip(dev):
    """One tile more than the count scan takes per trip of its loop, and 7 elements: the carry from trip to trip."""
    from cl_ops_amd.select import SELECT_SCAN_TRIP
    T = tile_of(dev, "uint", "keys")
    n = (SELECT_SCAN_TRIP + 1) * T + 7
    assert -(-n // T) == SELECT_SCAN_TRIP + 2
    mask = mask_of("p = 0.5", n, T, 3)
    keys, flags = inputs_for("flagged", mask, 4)
    assert run_select(dev, "select", "flagged", "uint", keys, flags, "keys", "%d tiles" % (SELECT_SCAN_TRIP + 2)) == int(mask.sum())
    keys, thr = inputs_for("lt", mask, 5)
    assert run_select(dev, "partition", "lt", "uint", keys, thr, "keys", "%d tiles" % (SELECT_SCAN_TRIP + 2)) == int(mask.sum())


def test_one_object_large_small_large(dev):
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    for op, pred in (("select", "flagged"), ("partition", "ge")):
        s = clo.Select(op, pred, ctx, "uint", 4)
        for j, n in enumerate((40 * T + 3, 5, 0, 70 * T + 7, 3 * T)):
            keys, fot = inputs_for(pred, mask_of("p = 0.5", n, T, j), 30 + j)
            run_select(dev, op, pred, "uint", keys, fot, "v4" if j % 2 == 0 else "arg", "call %d, n = %d" % (j, n), obj=s)
        s.close()


def test_threshold_written_by_the_kernel_before(dev):
    """The pivot is computed on the device: a flagged select with one flag set picks keys[j] into a device buffer, and
    the comparison that follows on the same stream, with no host wait between the two, takes that buffer as its
    threshold."""
    clo, ctx, q = dev
    T = tile_of(dev, "int", "keys")
    n = 3 * T + 11
    rng = np.random.default_rng(77)
    keys = rng.integers(-1000, 1000, n).astype(np.int32)
    for j, (op, pred) in enumerate((("select", "lt"), ("partition", "ge"), ("select", "eq"))):
        at = int(np.argsort(keys, kind="stable")[n // 2 + 100 * j])     # a key near the median: both sides are non-empty
        flags = np.zeros(n, np.uint8)
        flags[at] = 9
        k_r, f_r = Region(dev, keys.nbytes, 0, keys, 0), Region(dev, n, 0, flags, 1)
        pivot_r, ko_r = Region(dev, keys.nbytes, 0, None, 2), Region(dev, keys.nbytes, 0, None, 2)
        num1_r, num2_r = Region(dev, 8, 0, None, 1), Region(dev, 8, 0, None, 1)
        pick, cmp_ = clo.Select("select", "flagged", ctx, "int", 0), clo.Select(op, pred, ctx, "int", 0)
        thr_view = clo.Buffer(ctx, 4, device_ptr=pivot_r.ptr)           # the first row of the first call's output
        try:
            assert pick.with_device_data(q, k_r.view, None, f_r.view, pivot_r.view, None, num1_r.view, n)
            assert cmp_.with_device_data(q, k_r.view, None, thr_view, ko_r.view, None, num2_r.view, n)
            q.finish()
            pivot_r.check(keys[at:at + 1], "the pivot")
            num1_r.check(np.array([1], np.uint64), "the pivot's count")
            p, k = select(op, pred, keys, keys[at])
            assert 0 < k < n
            num2_r.check(np.array([k], np.uint64), "%s %s: num_out" % (op, pred))
            ko_r.check(keys[p], "%s %s with a threshold from the device: keys_out" % (op, pred))
        finally:
            thr_view.close()
            for x in (k_r, f_r, pivot_r, ko_r, num1_r, num2_r, pick, cmp_):
                x.close()


def test_two_objects_on_two_streams(dev):
    """Two objects, each with its own workspace, enqueued on two queues without a wait in between, three rounds."""
    clo, ctx, q = dev
    T = tile_of(dev, "uint", "v4")
    n = 150 * T + 9
    qs = [clo.Queue(ctx), clo.Queue(ctx)]
    specs = (("select", "flagged", "v4"), ("partition", "gt", "arg"))
    objs = [clo.Select(op, pred, ctx, "uint", 4) for op, pred, _ in specs]
    try:
        for rnd in range(3):
            sent = []
            for i, (op, pred, mode) in enumerate(specs):
                keys, fot = inputs_for(pred, mask_of("p = 0.5", n, T, 10 * rnd + i), 50 + 10 * rnd + i)
                fot = np.ascontiguousarray(fot).reshape(-1)
                vals = values_for(mode, n)
                rdev = (clo, ctx, qs[i])
                regs = [Region(rdev, keys.nbytes, 0, keys, 0), Region(rdev, vals.nbytes, 0, vals, 1) if vals is not None else None,
                        Region(rdev, fot.nbytes, 0, fot, 0), Region(rdev, keys.nbytes, 0, None, 2), Region(rdev, 4 * n, 0, None, 2), Region(rdev, 8, 0, None, 1)]
                sent.append((keys, fot, vals, regs))
            for i in range(2):
                qs[i].finish()                                          # the uploads; from here on nothing waits
            for i, (keys, fot, vals, regs) in enumerate(sent):
                view = lambda r: r.view if r is not None else None
                assert objs[i].with_device_data(qs[i], regs[0].view, view(regs[1]), regs[2].view, regs[3].view, regs[4].view, regs[5].view, n)
            for i in range(2):
                qs[i].finish()
            for i, (keys, fot, vals, regs) in enumerate(sent):
                op, pred, mode = specs[i]
                p, k = select(op, pred, keys, fot if pred == "flagged" else fot[0])
                what = "round %d, %s %s" % (rnd, op, pred)
                regs[5].check(np.array([k], np.uint64), what + ": num_out")
                regs[3].check(keys[p], what + ": keys_out")
                regs[4].check(vals[p] if vals is not None else p, what + ": values_out")
                for r in regs:
                    if r:
                        r.close()
    finally:
        for x in objs + qs:
            x.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "v8", "arg", "arg_only"])
def test_host_data_form(dev, mode):
    clo, ctx, q = dev
    T = tile_of(dev, "int", mode)
    keys = np.random.default_rng(1).permutation(keys_of_type("int", 2 * T + 9, 1))
    vals = values_for(mode, keys.size)
    flags = (np.arange(keys.size) % 3 == 0).astype(np.uint8) * np.uint8(7)
    for op in OPS:
        for pred in ("flagged", "le"):
            s = clo.Select(op, pred, ctx, "int", _VS[mode])
            fot = flags if pred == "flagged" else keys[11]
            ko, vo, k = s.with_host_data(keys, fot, vals, keys_out=mode != "arg_only", q_exec=q if mode != "v4" else None)
            p, want_k = select(op, pred, keys, fot)
            assert k == want_k and (ko is None) == (mode == "arg_only") and (vo is None) == (mode == "keys")
            if ko is not None:
                assert np.array_equal(ko, keys[p]), (op, pred)
            if vo is not None:
                assert np.array_equal(vo, vals[p] if vals is not None else p), (op, pred)
            s.close()
    # the indices of the set flags alone: no keys at all
    s = clo.Select("select", "flagged", ctx, "int", 4)
    ko, vo, k = s.with_host_data(None, flags, q_exec=q)
    assert ko is None and k == int((flags != 0).sum()) and np.array_equal(vo, np.flatnonzero(flags).astype(np.uint32))
    s.close()


def test_host_data_form_with_a_queue_for_the_transfers(dev):
    """2 tiles + 1 elements; the transfers on a queue of their own, then no queue at all (the call makes and destroys
    one). The count is read first and says how many rows of a select are copied (all numel of a partition): flags and a
    threshold that keep some, and ones that keep none."""
    clo, ctx, q = dev
    T = tile_of(dev, "int", "v4")
    keys = np.random.default_rng(2).permutation(keys_of_type("int", 2 * T + 1, 3))
    vals = values_for("v4", keys.size)
    flags = (np.arange(keys.size) % 5 == 1).astype(np.uint8)
    qc = clo.Queue(ctx)
    try:
        for op in OPS:
            for pred, some, none in (("flagged", flags, np.zeros_like(flags)), ("gt", keys[7], keys.max())):   # nothing is above the largest
                s = clo.Select(op, pred, ctx, "int", 4)
                for qe, qcomm in ((q, qc), (None, None)):
                    for fot in (some, none):
                        ko, vo, k = s.with_host_data(keys, fot, vals, q_exec=qe, q_comm=qcomm)
                        p, want_k = select(op, pred, keys, fot)
                        what = (op, pred, qe is None, qcomm is None, fot is none)
                        assert k == want_k and np.array_equal(ko, keys[p]) and np.array_equal(vo, vals[p]), what
                        if fot is none:
                            assert k == 0 and ko.size == (keys.size if op == "partition" else 0), what
                s.close()
    finally:
        qc.close()


def test_thin_abi_status_codes(dev):
    clo, ctx, q = dev
    from cl_ops_amd._hip import lib
    EARGS, EUNSUPPORTED, EWORKSPACE = -1, -2, -3
    n = 1000
    need = lib.clo_hip_select_workspace_bytes(n, 4, 4)
    assert need > 0 and need % 256 == 0
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 100, 2 * n + 4, dtype=np.uint32)
    flags = rng.integers(0, 2, 2 * n + 4).astype(np.uint8)
    ki, fl, th = Region(dev, 8 * n + 16, 0, keys, 0), Region(dev, 2 * n + 4, 0, flags, 1), Region(dev, 16, 0, np.array([50, 0, 0, 0], np.uint32), 2)
    vi, ko, vo = (Region(dev, 16 * n + 16, 0, None, i) for i in range(3))
    num = Region(dev, 16, 0, None, 0)
    ws = clo.Buffer(ctx, need + 256)
    s = q.stream

    def call(k_p, v_p, f_p, ko_p, vo_p, op=0, pred=1, num_p=num.ptr, numel=n, ks=4, kind=0, vs=4, w=ws.ptr, wb=need):
        return lib.clo_hip_select(op, pred, k_p, v_p, f_p, ko_p, vo_p, num_p, numel, ks, kind, vs, w, wb, s)

    try:
        full = (ki.ptr, vi.ptr, th.ptr, ko.ptr, vo.ptr)
        for op in (-1, 2, 100):
            assert call(*full, op=op) == EARGS
        for pred in (-1, 7, 100):
            assert call(*full, pred=pred) == EARGS
        for kind in (-1, 3):
            assert call(*full, kind=kind) == EARGS
        for ks, vs in ((3, 4), (16, 4), (0, 0), (4, 2), (4, 16)):
            assert call(*full, ks=ks, vs=vs) == EUNSUPPORTED, (ks, vs)
        assert call(*full, ks=1, kind=2) == EUNSUPPORTED                                                # no 1-byte floating-point keys
        assert call(*full, num_p=None) == EARGS and call(*full, num_p=num.ptr + 4) == EARGS             # num_out: missing, misaligned
        assert call(*full, numel=1 << 32) == EARGS
        assert call(None, vi.ptr, th.ptr, ko.ptr, vo.ptr) == EARGS                                      # a comparison reads the keys
        assert call(None, None, th.ptr, None, vo.ptr) == EARGS
        assert call(None, None, fl.ptr, ko.ptr, vo.ptr, pred=0) == EARGS                                # flagged with keys_out, too
        assert call(ki.ptr, vi.ptr, None, ko.ptr, vo.ptr) == EARGS and call(ki.ptr, vi.ptr, None, ko.ptr, vo.ptr, pred=0) == EARGS
        assert call(ki.ptr, vi.ptr, th.ptr, ko.ptr, None) == EARGS                                      # values_out with value_size 4
        assert call(ki.ptr, None, th.ptr, None, None, vs=0) == EARGS                                    # both outputs missing
        assert call(ki.ptr, None, th.ptr, ko.ptr, vo.ptr, vs=8) == EARGS                                # the arg form is 4-byte
        assert call(ki.ptr, vi.ptr, th.ptr, ko.ptr, None, vs=0) == EARGS                                # values with value_size 0
        assert call(ki.ptr, None, th.ptr, ko.ptr, vo.ptr, vs=0) == EARGS
        for i in range(5):                                                                              # one misaligned pointer at a time
            args = list(full)
            args[i] += 2
            assert call(*args) == EARGS, i
        args = list(full)
        args[1] += 4
        assert call(*args, vs=8) == EARGS                                                               # 4-aligned is not 8-aligned
        assert call(*full, w=ws.ptr + 64) == EARGS and call(*full, w=None) == EARGS                     # the workspace: misaligned, missing
        assert call(*full, wb=need - 1) == EWORKSPACE and call(*full, wb=0) == EWORKSPACE               # short
        q.finish()
        for r in (ko, vo, num):
            r.check(None, "a refused thin call wrote")
        # and what is asked for works: a workspace of exactly the size; flags at an odd address; 8-byte keys of kind 2
        # over the same bytes; numel 0 needs no workspace, no inputs, and still writes num_out
        first = lambda: int(num.base.read(q, np.uint8, num.host.size)[num.at:num.at + 8].view(np.uint64)[0])
        assert call(*full) == 0
        q.finish()
        assert first() == int((keys[:n] < 50).sum())
        assert call(None, None, fl.ptr + 1, None, vo.ptr, pred=0, op=1) == 0
        q.finish()
        assert first() == int((flags[1:n + 1] != 0).sum())
        assert call(ki.ptr, None, th.ptr, ko.ptr, None, pred=6, ks=8, kind=2, vs=0, numel=n // 2) == 0
        q.finish()
        assert first() == int((keys.view(np.uint64)[:n // 2] != np.uint64(50)).sum())
        assert call(None, None, None, ko.ptr, None, pred=0, vs=0, numel=0, w=None, wb=0) == 0
        q.finish()
        assert first() == 0
    finally:
        ws.close()
        for r in (ki, fl, th, vi, ko, vo, num):
            r.close()


@pytest.mark.parametrize("mode", ["keys", "v4", "arg"])
def test_graph_capture_and_replay(dev, mode):
    """Two calls of clo_hip_select — a flagged select, then a partition by "lt" — captured from one client stream (a
    linear graph) after one eager warm-up and replayed three times, the flags and the threshold rewritten and the
    outputs and both counts refilled with a canary before each replay (the protocol of test_gpu_graph_capture.py): k and
    the rows follow the buffers."""
    import test_gpu_graph_capture as GC
    from cl_ops_amd._hip import lib
    clo, ctx, _ = dev
    q = clo.Queue(ctx)
    gdev = (clo, ctx, q, None)
    T = tile_of(dev, "uint", mode)
    n, vs = 3 * T + 5, _VS[mode]
    valued = mode == "v4"
    need = lib.clo_hip_select_workspace_bytes(n, 4, vs)
    made = [GC.Mem(gdev, x) for x in (4 * n, 4 * n, n, 4, 4 * n, 4 * n, 8, 4 * n, 4 * n, 8, need, need)]
    ki, vi, fl, th, ko1, vo1, num1, ko2, vo2, num2, ws1, ws2 = made
    keys = np.random.default_rng(1).integers(0, 1000, n, dtype=np.uint32)
    vals = values_for("v4", n)
    rates = [0.5, 0.01, 0.99, 0.3, 0.5]
    ks = set()

    def load(r):
        flags = np.where(np.random.default_rng(200 + r).random(n) < rates[r], 1 + r, 0).astype(np.uint8)
        thr = np.uint32(1000 * rates[r])
        for m in (ko1, vo1, num1, ko2, vo2, num2):
            m.fill()
        for mem_, arr in ((ki, keys), (vi, vals), (fl, flags), (th, np.array([thr], np.uint32))):
            mem_.put(arr)
        want = select("select", "flagged", keys, flags), select("partition", "lt", keys, thr)
        ks.add((want[0][1], want[1][1]))
        return want

    def one(op, pred, fot, ko, vo, num, ws):
        return lambda: lib.clo_hip_select(op, pred, ki.ptr, vi.ptr if valued else None, fot.ptr, ko.ptr, vo.ptr if vs else None, num.ptr, n,
                                          4, 0, vs, ws.ptr, need, q.stream)

    def enqueue():
        return GC.first(one(0, 0, fl, ko1, vo1, num1, ws1), one(1, 1, th, ko2, vo2, num2, ws2))

    def verify(r, want):
        for (p, k), ko, vo, num, name in ((want[0], ko1, vo1, num1, "flagged select"), (want[1], ko2, vo2, num2, "lt partition")):
            tag = "%s %s round %d" % (name, mode, r)
            assert int(num.get(np.uint64, 1)[0]) == k, tag + ": num_out"
            rest = GC.canary(np.uint32, n - p.size)
            GC.same(ko.get(np.uint32, n), np.concatenate((keys[p], rest)), tag + ": keys_out")
            GC.same(vo.get(np.uint32, n), np.concatenate(((vals[p] if valued else p), rest)) if vs else GC.canary(np.uint32, n), tag + ": values_out")
        GC.same(ki.get(np.uint32, n), keys, "keys_in")

    try:
        GC.run_protocol(gdev, GC.Case(load, enqueue, verify))
        assert len(ks) >= 4, ks                                         # k differed between the replays
    finally:
        lib.clo_hip_stream_synchronize(q.stream)
        for x in made:
            x.close()
        q.close()


def test_indices_above_2p31(dev):
    """numel = 2^31 + T + 3 uchar keys, "eq" to a value planted at about 2^11 places that include the first element, both
    sides of index 2^31 and the last element; the indices alone, against torch.nonzero on the device (taken in chunks
    below 2^31 elements). Rows >= k keep their canary."""
    import torch
    clo, ctx, q = dev
    T = tile_of(dev, "uchar", "arg_only")
    n = (1 << 31) + T + 3
    free = torch.cuda.mem_get_info()[0]
    if free < (20 << 30):
        pytest.skip("needs about 16 GiB of free device memory (2 GiB of keys, 8 GiB of indices, torch's scratch), %.1f GiB are free" % (free / 2 ** 30))
    g = torch.Generator(device="cuda").manual_seed(31)
    keys = torch.empty(n, dtype=torch.uint8, device="cuda")
    step = 1 << 28
    for lo in range(0, n, step):
        hi = min(lo + step, n)
        keys[lo:hi] = torch.randint(0, 200, (hi - lo,), dtype=torch.uint8, device="cuda", generator=g)      # never 201
    planted = torch.randint(0, n, (1 << 11,), dtype=torch.int64, device="cuda", generator=g)
    planted = torch.cat((planted, torch.tensor([0, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, n - 1], dtype=torch.int64, device="cuda")))
    keys[planted] = 201
    thr = torch.tensor([201], dtype=torch.uint8, device="cuda")
    out = torch.full((n,), -0x3C3C3C3D, dtype=torch.int32, device="cuda")                               # bytes C3 C3 C3 C3
    cnt = torch.full((1,), -1, dtype=torch.int64, device="cuda")
    want = torch.cat([torch.nonzero(keys[lo:min(lo + step, n)] == 201).flatten() + lo for lo in range(0, n, step)])
    torch.cuda.synchronize()
    as_buffer = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
    bufs = [as_buffer(t) for t in (keys, thr, out, cnt)]
    s = clo.Select("select", "eq", ctx, "uchar", 4)
    try:
        assert s.with_device_data(q, bufs[0], None, bufs[1], None, bufs[2], bufs[3], n)
        q.finish()
        k = int(cnt[0])
        assert k == want.numel() and (1 << 11) - 8 <= k <= (1 << 11) + 5
        got = out[:k].to(torch.int64) & 0xFFFFFFFF                                                      # the indices are uint
        assert bool((got == want).all()), "the indices differ from torch.nonzero"
        assert int(got[-1]) == n - 1 and int(got[0]) == 0
        for lo in range(k, n, step):
            assert bool((out[lo:min(lo + step, n)] == -0x3C3C3C3D).all()), "rows >= k were written"
    finally:
        for x in bufs + [s]:
            x.close()
        del keys, out, want
        torch.cuda.empty_cache()
