"""Seeded random sweeps over the sort / scan entry points (GPU): sizes that straddle
every path boundary (one-launch sorts, single-sweep passes, 8 192- and 16 384-element
tiles), every radix, element types, in place / out of place, stable pairs — against
numpy. Everything goes through the C-ABI of libcl_ops_hip.so.

The second half is the STRATIFIED fuzz of reduce by key, scan by key, histogram, merge, search, the set operations,
select, top-k, expand, the segmented reduction and the segmented sort: the kernels of those eleven are templates over (key size or type x value -> sum conversion, value form x op, mode
or path), and draw_cases() walks the list of those instantiations, written out below from the public type rules, so that
the committed seeds together launch every one; sizes, run structures, bounds, layouts, thresholds, view offsets and the
reuse of one object over a random sequence of sizes are random per case. draw_cases() and the *_inputs() functions touch
no GPU: tests/test_fuzz_reach_cpu.py imports them."""
import math

import numpy as np
import pytest

import oracle_lib as O
import sbk_model
import test_gpu_expand as TE
import test_gpu_histogram as TH
import test_gpu_merge as TM
import test_gpu_reduce_by_key as TR
import test_gpu_scan_by_key as TS
import test_gpu_search as TSE
import test_gpu_segreduce as TSR
import test_gpu_segsort as TSS
import test_gpu_select as TSL
import test_gpu_setop as TSO
import test_gpu_topk as TT
from merge_model import order_key, sort_keys
from segsort_model import segsort

pytestmark = pytest.mark.gpu

# boundaries of the radix paths, in elements: one launch <= 16384 (8192 of 8 bytes), sweeps up to
# 1024 tiles of 8192 (4096), big tiles from 32 MiB (8-byte) / 256 MiB (4-byte)
EDGES_4 = [1, 2, 17, 4095, 4096, 4097, 8192, 16384, 16385, 32768 + 1, (1 << 20) - 1, (1 << 23), (1 << 23) + 8193, (1 << 24) + 5]
EDGES_8 = [1, 3, 4096, 8192, 8193, 16385, (1 << 19) + 77, (1 << 22), (1 << 22) + 4097, (1 << 23) - 1, (1 << 23) + 16385]


@pytest.mark.parametrize("seed", range(6))
def test_fuzz_satradix_keys(gpu, seed):
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(1000 + seed)
    for _ in range(8):
        et = rng.choice(["uchar", "ushort", "uint", "ulong", "int", "long", "float", "double"])
        dt = clo.api.CLO_TYPE_NP[et]
        edges = EDGES_8 if dt.itemsize == 8 else EDGES_4
        n = int(rng.choice(edges)) + int(rng.integers(0, 3))
        radix = int(rng.choice([2, 4, 8, 16, 32, 64, 128, 256]))
        if n < radix:
            n = radix
        if np.issubdtype(dt, np.floating):
            a = ((rng.random(n) - 0.5) * 10.0 ** int(rng.integers(0, 30))).astype(dt)
        else:
            info = np.iinfo(dt)
            span = int(rng.choice([8, 1 << 10, int(info.max) - int(info.min)]))   # few distinct values ... the whole range
            lo = int(info.min) if info.min < 0 and span > 1 << 10 else 0
            a = rng.integers(lo, lo + min(span, int(info.max) - lo), n, dtype=np.int64 if dt.itemsize < 8 or info.min < 0 else np.uint64, endpoint=True).astype(dt)
        s = clo.Sorter("satradix", ctx, et, options="radix=%d" % radix)
        exp = np.sort(a)
        if rng.integers(0, 2):
            got = s.with_host_data(a, q)
        else:   # device buffers, in place or into a second buffer
            src = clo.Buffer(ctx, a.nbytes)
            src.write(q, a)
            if rng.integers(0, 2):
                s.with_device_data(q, src, None, n)
                got = src.read(q, dt, n)
            else:
                dst = clo.Buffer(ctx, a.nbytes)
                s.with_device_data(q, src, dst, n)
                got = dst.read(q, dt, n)
                assert np.array_equal(src.read(q, dt, n).view(np.uint8), a.view(np.uint8)), "data_in changed"
                dst.close()
            src.close()
        s.close()
        assert np.array_equal(got.view(np.uint8), exp.view(np.uint8)), "type %s n %d radix %d" % (et, n, radix)


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_satradix_pairs_stable(gpu, seed):
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(2000 + seed)
    for _ in range(5):
        n = int(rng.choice(EDGES_8)) + int(rng.integers(0, 3))
        radix = int(rng.choice([4, 16, 64, 256]))
        n = max(n, radix)
        keys = rng.integers(0, int(rng.choice([4, 1 << 12, 1 << 32])), n, dtype=np.uint64)
        a = (keys << np.uint64(32)) | np.arange(n, dtype=np.uint64)
        s = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)", options="radix=%d" % radix)
        got = s.with_host_data(a, q)
        s.close()
        assert np.array_equal(got, O.stable_sort(a, key_size=4, key_shift=32)), "n %d radix %d" % (n, radix)


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_scan(gpu, seed):
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(3000 + seed)
    one = None
    for _ in range(10):
        et, st = [("uint", "uint"), ("uint", "ulong"), ("uchar", "uint"), ("int", "long"), ("ushort", "ulong"), ("ulong", "ulong")][int(rng.integers(0, 6))]
        edt, sdt = clo.api.CLO_TYPE_NP[et], clo.api.CLO_TYPE_NP[st]
        n = int(rng.choice([1, 5, 4096, 16384, 16385, (1 << 20) + 3, (1 << 24) - 1, (1 << 24), (1 << 24) + 32769]))
        info = np.iinfo(edt)
        a = rng.integers(int(info.min), min(int(info.max), 1 << 40), n, dtype=np.int64, endpoint=False).astype(edt)
        sc = clo.Scanner("blelloch", ctx, et, st)
        got = sc.with_host_data(a, q)
        sc.close()
        wide = a.astype(np.int64 if info.min < 0 else np.uint64)
        exp = np.concatenate((np.zeros(1, wide.dtype), np.cumsum(wide[:-1], dtype=wide.dtype))).astype(sdt)
        assert np.array_equal(got, exp), "%s -> %s, n %d" % (et, st, n)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_key_fields(gpu, seed):
    """Random KEY FIELDS of the element (get_key = a shift and a mask of any width) at sizes on every path of the
    radix sort, radix 4 / 16 / 256: numpy's stable sort by the field. (Round 3: a 28-bit field on the single-sweep
    passes came out wrong with every test of whole-type keys green; tools/fuzz_keyfield_gpu.py is the long run.)"""
    import cl_ops_amd as clo
    ctx, q = gpu
    rng = np.random.default_rng(4000 + seed)
    sizes4 = [5, 4097, 16385, 40000, (1 << 17) + 3, (1 << 20) + 1, (1 << 22) + 77, (1 << 23) + 8193]
    sizes8 = [3, 8193, 30000, (1 << 16) + 3, (1 << 19) + 1, (1 << 21) + 77, (1 << 22) + 4097]
    for _ in range(10):
        es = int(rng.choice([4, 8]))
        et, dt = ("uint", np.uint32) if es == 4 else ("ulong", np.uint64)
        bits = 8 * es
        n = int(rng.choice(sizes4 if es == 4 else sizes8)) + int(rng.integers(0, 5))
        width = int(rng.integers(1, bits + 1))
        shift = int(rng.integers(0, bits - width + 1))
        mask = (1 << width) - 1
        a = rng.integers(0, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
        key = (a >> dt(shift)) & dt(mask)
        kt = "uint" if width <= 32 else "ulong"
        get_key = "(%s) (((x) >> %d) & 0x%x%s)" % (kt, shift, mask, "ul" if es == 8 else "u")
        radix = int(rng.choice([4, 16, 256]))
        s = clo.Sorter("satradix", ctx, et, key_type=kt, get_key=get_key, options="radix=%d" % radix)
        got = s.with_host_data(a, q)
        s.close()
        assert np.array_equal(got, a[np.argsort(key, kind="stable")]), "%s n=%d %s radix=%d" % (et, n, get_key, radix)


@pytest.mark.parametrize("seed", range(4))
def test_fuzz_segmented_sort(gpu, seed):
    """clo_hip_radix_sort_segmented (round 4): random segment counts and lengths (empty ones, one tile, many counter-scan
    chunks), the source as the segments back to back or as up to 256 pieces scattered over a larger array, key fields at
    any shift, both digit widths, both element sizes — against a stable numpy sort per segment."""
    import ctypes as C
    import torch
    from cl_ops_amd import _hip
    from cl_ops_amd._hip import lib
    rng = np.random.default_rng(4000 + seed)
    for case in range(10):
        es = int(rng.choice([4, 8]))
        dt, tdt = (np.uint32, np.int32) if es == 4 else (np.uint64, np.int64)
        n = int(rng.choice([1, 37, 8192, 8193, 100000, (1 << 20) + 5, (1 << 22) + 12345]))
        nseg = int(rng.choice([1, 2, 7, 64, 255, 256]))
        cuts = np.sort(rng.integers(0, n + 1, nseg - 1)) if nseg > 1 else np.array([], dtype=np.int64)
        seg_counts = np.diff(np.concatenate(([0], cuts, [n]))).astype(np.int64)
        shift = int(rng.integers(0, 8 * es - 1))
        bits = int(rng.integers(1, 8 * es - shift + 1))
        digit_bits = int(rng.choice([4, 8]))
        pieces = bool(rng.integers(0, 2)) and nseg <= 64
        if pieces:          # every segment in up to 4 pieces, scattered over a source three times the size
            per = 4
            big = rng.integers(0, np.iinfo(dt).max, 3 * n + 5 * per * nseg + 64, dtype=dt, endpoint=True)
            pn, ps = [], []
            for k in range(nseg):
                c = np.sort(rng.integers(0, seg_counts[k] + 1, per - 1))
                for x in np.diff(np.concatenate(([0], c, [seg_counts[k]]))):
                    pn.append(int(x)); ps.append(k)
            order = rng.permutation(len(pn))                       # where the pieces lie has nothing to do with their order
            po = np.zeros(len(pn), dtype=np.int64)
            at = 3
            for i in order:
                po[i] = at
                at += pn[i] + int(rng.integers(0, 5))
            assert at <= big.size
            src_np = big
            gathered = np.concatenate([big[po[i]:po[i] + pn[i]] for i in range(len(pn))]) if n else big[:0]
        else:
            src_np = rng.integers(0, np.iinfo(dt).max, n, dtype=dt, endpoint=True)
            gathered = src_np
        src = torch.from_numpy(src_np.view(tdt).copy()).cuda()
        ta = src if not pieces else torch.zeros(max(n, 1), dtype=src.dtype, device="cuda")
        tb = torch.zeros(max(n, 1), dtype=src.dtype, device="cuda")
        need = lib.clo_hip_radix_seg_workspace_bytes(n, nseg, es, digit_bits)
        ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
        in_b = C.c_int(-1)
        if pieces:
            npc = len(pn)
            extra = ((C.c_size_t * npc)(*pn), (C.c_size_t * npc)(*[int(x) for x in po]), (C.c_int * npc)(*ps), npc)
        else:
            extra = (None, None, None, 0)
        _hip.check(lib.clo_hip_radix_sort_segmented(src.data_ptr(), ta.data_ptr(), tb.data_ptr(), n, (C.c_size_t * nseg)(*[int(x) for x in seg_counts]), nseg,
                                                    *extra, es, shift, bits, digit_bits, ws.data_ptr(), need, torch.cuda.current_stream().cuda_stream, C.byref(in_b)))
        torch.cuda.synchronize()
        got = (tb if in_b.value else ta).cpu().numpy().view(dt)[:n]
        exp = np.empty_like(gathered)
        at = 0
        mask = dt((1 << bits) - 1)
        for c in seg_counts:
            seg = gathered[at:at + c]
            exp[at:at + c] = seg[np.argsort((seg >> dt(shift)) & mask, kind="stable")]
            at += c
        assert np.array_equal(got, exp), "seed %d case %d: es %d n %d nseg %d shift %d bits %d digit %d pieces %s" % (seed, case, es, n, nseg, shift, bits, digit_bits, pieces)
        if pieces:
            assert np.array_equal(src.cpu().numpy().view(dt), src_np), "the source of a gathered sort changed"


@pytest.mark.parametrize("seed", range(3))
def test_fuzz_sharded_sort_loopback(gpu, seed):
    """The sharded C path on one rank over real RCCL (`loopback=1`): random slice counts and key distributions that
    leave sub-buckets and whole slices EMPTY or put everything into one (fixed bits, a handful of values, one range of
    the key space, ascending keys, all equal), sizes on both sides of the slicing threshold — against numpy's sort.
    The same object sorts several inputs in a row (buffers, events and the adaptive table are reused)."""
    import torch
    from cl_ops_amd.multigpu import CShardedSorter
    rng = np.random.default_rng(5000 + seed)
    for etype in ("uint", "ulong"):
        dt, tdt = (np.uint32, np.int32) if etype == "uint" else (np.uint64, np.int64)
        top = int(np.iinfo(dt).max)
        opt = [None, "slices=1", "slices=2", "slices=4", "slices=8", "radix=256,slices=4"][int(rng.integers(0, 6))]
        s = CShardedSorter(etype, 0, options=(opt + "," if opt else "") + "loopback=1,slice_min=%d" % (16 << 20))
        for case in range(6):
            n = int(rng.choice([0, 1, 70000, (1 << 22) - 3, (1 << 22) + 4099, (1 << 23) + 17]))
            mode = int(rng.integers(0, 6))
            if mode == 0:
                a = rng.integers(0, top, n, dtype=dt, endpoint=True)
            elif mode == 1:     # some bits fixed
                a = (rng.integers(0, top, n, dtype=dt, endpoint=True) & dt(rng.integers(0, top, dtype=dt, endpoint=True) | rng.integers(0, top, dtype=dt, endpoint=True))) \
                    | dt(rng.integers(0, top, dtype=dt, endpoint=True) & rng.integers(0, top, dtype=dt, endpoint=True) & rng.integers(0, top, dtype=dt, endpoint=True))
            elif mode == 2:     # a handful of values
                vals = rng.integers(0, top, int(rng.integers(1, 17)), dtype=dt, endpoint=True)
                a = vals[rng.integers(0, vals.size, n)]
            elif mode == 3:     # one range of the key space
                lo = int(rng.integers(0, top, dtype=dt, endpoint=True))
                span = min(top - lo, top >> int(rng.integers(0, 8 * np.dtype(dt).itemsize - 4)))
                a = (dt(lo) + rng.integers(0, span, n, dtype=dt, endpoint=True)).astype(dt)
            elif mode == 4:     # ascending
                a = (np.arange(n, dtype=np.uint64) * np.uint64(max(1, (top // max(n, 1)) >> int(rng.integers(0, 8))))).astype(dt)
            else:               # all equal
                a = np.full(n, rng.integers(0, top, dtype=dt, endpoint=True), dtype=dt)
            t = torch.from_numpy(np.ascontiguousarray(a).view(tdt).copy()).cuda() if n else torch.empty(0, dtype=torch.int32 if etype == "uint" else torch.int64, device="cuda")
            out, m = s.sort(t)
            s.check()
            torch.cuda.synchronize()
            assert m == n, (etype, opt, mode, n)
            assert np.array_equal(out.cpu().numpy().view(dt)[:n], np.sort(a)), (etype, opt, mode, n)
        s.close()


# ----------------------------------------------------------------------------------------------------------------------
# The stratified fuzz of the eleven families
# ----------------------------------------------------------------------------------------------------------------------

_KT_BY_SIZE = {1: ["uchar"], 2: ["ushort"], 4: ["uint", "int", "float"], 8: ["ulong", "double"]}     # reduce / scan by key
_BK_PAIRS = [("uint", "uint"), ("int", "long"), ("uint", "ulong"), ("ulong", "ulong")]
_BK_KINDS = ["len_uint", "len_ulong"] + [(vt, st, op) for vt, st in _BK_PAIRS for op in ("sum", "min", "max")]
_HIST_KT = {(1, 0): "uchar", (1, 1): "char", (2, 0): "ushort", (2, 1): "short", (4, 0): "uint", (4, 1): "int", (8, 0): "ulong", (8, 1): "long"}
_HIST_CVT = {"cnt_uint": (None, "uint"), "cnt_ulong": (None, "ulong"), "uint->uint": ("uint", "uint"), "int->long": ("int", "long"),
             "uint->ulong": ("uint", "ulong"), "long->long": ("long", "long")}
_HIST_BINS = ["copies", "peel", "global"]      # <= the 32-copy limit | up to histogram_lds_bins | histogram_lds_bins + 1
_MERGE_MODES = ["keys", "v4", "v8", "arg", "arg_only"]
_SELECT_CMP = list(TSL.PREDS[1:])

# Every kernel instantiation a family has, from the public type rules (include/clo_reduce.h, clo_scan_by_key.h,
# clo_histogram.h, clo_merge.h, clo_search.h, clo_setop.h, clo_select.h; DESIGN.md for the three forms of the
# histogram), not from the kernels' enums. search: (key type, upper, NEEDLES_SORTED); setop: (key type, value mode, op);
# select: (key type, value form, by flags | by comparison), the indices of the set flags without keys_in being a form of
# the flagged selection alone. topk (include/clo_topk.h): (key type, value form, order), the "sorted" order with its own
# kernel per (key size, value size) that reads the keys from the workspace where keys_out is not given (arg_only), and
# the k-th key alone, which stops after the digit sweeps and has no order. expand (include/clo_expand.h): (form, count
# type, value size, 0 for an object without values); segreduce (include/clo_segreduce.h): (form, count type, (value, sum)
# pair, op); segsort (include/clo_segsort.h): (key type, value mode, form, count type).
_COUNT_TYPES = ("uint", "ulong")
STRATA = {
    "expand": [(form, ct, vs) for form in TE.FORMS for ct in _COUNT_TYPES for vs in (0, 1, 2, 4, 8)],
    "segreduce": [(form, ct, pair, op) for form in TSR.FORMS for ct in _COUNT_TYPES for pair in TSR.PAIRS for op in TSR.OPS],
    "segsort": [(kt, mode, form, ct) for kt in TSS.KEY_NP for mode in TSS.MODES for form in TSS.FORMS for ct in _COUNT_TYPES],
    "rbk": [(ks, kind) for ks in (1, 2, 4, 8) for kind in ["keys_only"] + _BK_KINDS],
    "sbk": [(ks, kind, incl) for ks in (1, 2, 4, 8) for kind in _BK_KINDS for incl in (False, True)],
    "hist": [(ks, sg, cvt, b) for ks in (1, 2, 4, 8) for sg in (0, 1) for cvt in _HIST_CVT for b in _HIST_BINS],
    "merge": [(kt, mode) for kt in TM.KEY_TYPES for mode in _MERGE_MODES],
    "search": [(kt, upper, flag) for kt in TSE.KEY_TYPES for upper in (False, True) for flag in (False, True)],
    "setop": [(kt, mode, op) for kt in TM.KEY_TYPES for mode in _MERGE_MODES for op in TSO.OPS],
    "select": [(kt, mode, cls) for kt in TM.KEY_TYPES for mode in TSL.MODES for cls in ("flagged", "cmp")] + [(kt, "arg_no_keys", "flagged") for kt in TM.KEY_TYPES],
    "topk": [(kt, mode, order) for kt in TM.KEY_TYPES for mode in TT.MODES for order in TT.ORDERS] + [(kt, "kth_only", None) for kt in TM.KEY_TYPES],
}
# seeds x cases >= 2 x strata: half the cases of a seed open a new stratum (with a new object), the other half reuse
# the object of the case before them on a stratum it can run
SEEDS = {"expand": 2, "segreduce": 4, "segsort": 8, "rbk": 2, "sbk": 3, "hist": 4, "merge": 2, "search": 2, "setop": 8, "select": 4, "topk": 4}
CASES = {"expand": 60, "segreduce": 72, "segsort": 60, "rbk": 60, "sbk": 76, "hist": 72, "merge": 60, "search": 60, "setop": 60, "select": 62, "topk": 62}
# expand's object fixes its stratum and there are 20 of them: its seeds open a new object at half of their cases all the
# same, so that the other half reuses one (every stratum three times over the two seeds)
_FRESH = {"expand": 30}
_SALT = {"expand": 69, "segreduce": 70, "segsort": 71, "rbk": 61, "sbk": 62, "hist": 63, "merge": 64, "search": 65, "setop": 66, "select": 67, "topk": 68}


def _size(x):
    return np.dtype(x).itemsize


def _vsize(family, vt):
    return 0 if vt is None else _size((TH._NP if family == "hist" else TR._NP)[vt])


def tile_of(family, ks, vs):
    """Elements per tile, from the library's getters (host code only)."""
    import cl_ops_amd as clo
    if family == "search":
        t = clo.search_tile(ks)                       # needles per tile
    else:
        t = {"rbk": clo.reduce_by_key_tile, "sbk": clo.scan_by_key_tile, "hist": clo.histogram_tile, "merge": clo.merge_tile, "setop": clo.setop_tile,
             "select": clo.select_tile, "topk": clo.topk_tile}[family](ks, vs)
    assert t > 0
    return int(t)


def hist_limits(ss):
    """(the largest num_bins with 32 LDS copies: num_bins * 32 * ss <= 32 KiB, the largest with counters in LDS)."""
    import cl_ops_amd as clo
    L = int(clo.histogram_lds_bins(ss))
    assert L > 256
    return (32 << 10) // (32 * ss), L


def search_limits(ks):
    """(P, L): the pivots of the general path's sampled table and the longest haystack range staged in LDS."""
    import cl_ops_amd as clo
    P, L = int(clo.search_pivots(ks)), int(clo.search_lds_keys(ks))
    assert 2 <= P <= L
    return P, L


# the haystack sizes at which the search changes form
_HAY_EDGES = [lambda P, L: 0, lambda P, L: 1, lambda P, L: P - 1, lambda P, L: P, lambda P, L: P + 1, lambda P, L: L - 1, lambda P, L: L,
              lambda P, L: L + 1, lambda P, L: 2 * L + 5]

_EDGE_SIZES = [lambda t: 0, lambda t: 1, lambda t: t - 1, lambda t: t, lambda t: t + 1, lambda t: 2 * t - 1, lambda t: 2 * t + 1, lambda t: 3 * t + 1]


def _draw_n(rng, tile, edge=None):
    """Mostly below 4 tiles, a tail up to about 2^20, never only tile multiples. edge: one of _EDGE_SIZES instead
    (every seed deals each of them to one of its cases, whatever that case's tile is)."""
    if edge is not None:
        return _EDGE_SIZES[edge](tile)
    u = rng.random()
    if u < 0.15:
        return int(rng.integers(2, 600))              # a few waves of one work-group
    if u < 0.8:
        return int(rng.integers(2, 4 * tile))
    return int(2.0 ** rng.uniform(math.log2(4 * tile), 20.0)) + int(rng.integers(0, 7))


def _draw_off(rng, es):
    """An element-aligned byte offset in 0 .. 31."""
    return 0 if not es else int(es * rng.integers(0, 32 // es))


def _draw_structure(rng, n, tile):
    """A mixture of geometric stretches (each with a mean of its own from 1 to 50 000), sometimes unsorted key numbers,
    and one run longer than two tiles where n allows it."""
    s = {"kind": "unsorted" if rng.random() < 0.15 else "mixture", "seed": int(rng.integers(0, 1 << 30)), "cuts": [], "means": [], "long": None}
    if s["kind"] == "mixture":
        parts = int(rng.integers(1, 5))
        s["cuts"] = sorted(int(x) for x in rng.integers(0, n + 1, parts - 1))
        s["means"] = [max(1, int(50000.0 ** rng.random())) for _ in range(parts)]
    if n > 2 * tile + 1:
        ln = 2 * tile + 1 + int(rng.integers(0, min(tile, n - 2 * tile - 1) + 1))
        s["long"] = (int(rng.integers(0, n - ln + 1)), ln)
    return s


def _object_for(family, rng, stratum):
    """The constructor arguments of a new object that can run the stratum."""
    if family in ("expand", "segreduce"):
        return stratum
    if family == "segsort":
        return (stratum[0], TSS.VS[stratum[1]], stratum[2], stratum[3])
    if family in ("rbk", "sbk"):
        kt = str(rng.choice(_KT_BY_SIZE[stratum[0]]))
        kind = stratum[1]
        if kind == "keys_only":
            vt, st = _BK_PAIRS[int(rng.integers(0, 4))]
            op = str(rng.choice(["sum", "min", "max"]))
        elif kind == "len_uint":
            vt, st, op = "uint", "uint", "sum"
        elif kind == "len_ulong":
            vt, st, op = [("uint", "ulong"), ("ulong", "ulong")][int(rng.integers(0, 2))] + ("sum",)
        else:
            vt, st, op = kind
        return (kt, vt, st, op) if family == "rbk" else (kt, vt, st, op, stratum[2])
    if family == "hist":
        vt, st = _HIST_CVT[stratum[2]]
        return (_HIST_KT[stratum[:2]], vt or "uint", st, bool(rng.integers(0, 2)))
    if family == "search":
        return (stratum[0],)
    if family == "setop":
        return (stratum[2], stratum[0], TM._VS[stratum[1]])
    if family == "select":          # op and pred are arguments of every call: see _Selects
        return (stratum[0], TSL._VS[stratum[1]])
    if family == "topk":            # which and order are arguments of clo_topk_new: see _TopKs
        return (stratum[0], TT._VS[stratum[1]])
    return (stratum[0], TM._VS[stratum[1]])


def compatible(family, obj):
    """The strata an object can run."""
    if family in ("expand", "segreduce"):
        return [obj]
    if family == "segsort":
        return [(obj[0], m, obj[2], obj[3]) for m in TSS.MODES if TSS.VS[m] == obj[1]]
    if family in ("rbk", "sbk"):
        kt, vt, st, op = obj[:4]
        ks = _size(TR._NP[kt])
        kinds = [(vt, st, op)] + (["len_" + st] if op == "sum" and st in ("uint", "ulong") else [])
        if family == "rbk":
            return [(ks, k) for k in ["keys_only"] + kinds]
        return [(ks, k, obj[4]) for k in kinds]
    if family == "hist":
        kt, vt, st, _ = obj
        key = [k for k, v in _HIST_KT.items() if v == kt][0]
        cvts = [c for c, p in _HIST_CVT.items() if p == (vt, st)] + (["cnt_" + st] if st in ("uint", "ulong") else [])
        return [key + (c, b) for c in cvts for b in _HIST_BINS]
    if family == "search":
        return [(obj[0], upper, flag) for upper in (False, True) for flag in (False, True)]
    if family == "setop":
        return [(obj[1], m, obj[0]) for m in _MERGE_MODES if TM._VS[m] == obj[2]]
    if family == "select":
        return [(obj[0], m, cls) for m in TSL.MODES for cls in ("flagged", "cmp") if TSL._VS[m] == obj[1]] + \
            ([(obj[0], "arg_no_keys", "flagged")] if obj[1] == 4 else [])
    if family == "topk":
        return [(obj[0], m, order) for m in TT.MODES for order in TT.ORDERS if TT._VS[m] == obj[1]] + ([(obj[0], "kth_only", None)] if obj[1] == 0 else [])
    return [(obj[0], m) for m in _MERGE_MODES if TM._VS[m] == obj[1]]


def _draw_call(family, rng, stratum, obj, edge=None, state=None):
    """Everything of one call but the object: plain numbers, strings and lists. state: what select and topk carry from
    case to case (see _draw_select, _draw_topk)."""
    c = {}
    if family in ("expand", "segreduce", "segsort"):
        return _draw_segmented(family, rng, stratum, edge, state)
    if family == "search":
        return _draw_search(rng, stratum, edge)
    if family == "setop":
        return _draw_setop(rng, stratum, obj, edge)
    if family == "select":
        return _draw_select(rng, stratum, obj, edge, state)
    if family == "topk":
        return _draw_topk(rng, stratum, obj, edge, state)
    if family in ("rbk", "sbk"):
        kt, vt, st, op = obj[:4]
        kind = stratum[1]
        given = None if kind in ("len_uint", "len_ulong") else vt
        if kind == "keys_only" and op == "sum" and rng.random() < 0.5:
            given = None                                   # the keys alone, from a call without values too (min / max need them)
        ks, vs, ss = _size(TR._NP[kt]), _vsize(family, given), _size(TR._NP[st])
        tile = tile_of(family, ks, vs)
        n = _draw_n(rng, tile, edge)
        c.update(kt=kt, vt=given, st=st, op=op, n=n, tile=tile, structure=_draw_structure(rng, n, tile),
                 palette_seed=int(rng.integers(0, 50)), value_seed=int(rng.integers(0, 1 << 30)))
        if family == "rbk":
            c.update(want_k=bool(kind == "keys_only" or rng.random() < 0.8), want_a=kind != "keys_only",
                     offs=[_draw_off(rng, ks), _draw_off(rng, vs or 4), _draw_off(rng, ks), _draw_off(rng, ss)])
        else:
            c.update(inclusive=obj[4], in_place=bool(given is not None and vs == ss and rng.random() < 0.2),
                     offs=[_draw_off(rng, ks), _draw_off(rng, vs or 4), _draw_off(rng, ss)])
    elif family == "hist":
        kt, vt, st, acc = obj
        given = None if stratum[2].startswith("cnt_") else vt
        info = np.iinfo(TH._NP[kt])
        ks, vs, ss = info.bits // 8, _vsize(family, given), _size(TH._NP[st])
        tile = tile_of(family, ks, vs)
        copies, L = hist_limits(ss)
        nb = {"copies": int(rng.integers(1, copies + 1)), "peel": int(rng.choice([copies + 1, int(rng.integers(copies + 1, L + 1)), L])),
              "global": L + 1}[stratum[3]]
        shift = int(rng.integers(0, 4)) if rng.random() < 0.5 else int(rng.integers(0, info.bits))
        u = rng.random()
        lo, hi = int(info.min), int(info.max)
        if u < 0.3:          # within num_bins << shift of the type's maximum: the wrap trap
            lower = hi - int(rng.integers(0, min(nb << shift, hi - lo) + 1, dtype=np.uint64))
        elif u < 0.4:
            lower = lo
        else:
            lower = lo + int(rng.integers(0, hi - lo, dtype=np.uint64, endpoint=True))
        layout = str(rng.choice(["uniform", "skewed", "sorted", "handful"]))
        c.update(kt=kt, vt=given, st=st, accumulate=acc, n=_draw_n(rng, tile, edge), tile=tile, num_bins=nb, shift=shift, lower=lower, layout=layout,
                 outside=0.0 if layout == "sorted" else float(rng.choice([0.0, 0.2])), data_seed=int(rng.integers(0, 1 << 30)),
                 offs=[_draw_off(rng, ks), _draw_off(rng, vs or 4), _draw_off(rng, ss)])
    else:
        kt, vs = obj
        mode = stratum[1]
        ks = _size(TM._NP[kt])
        tile = tile_of(family, ks, vs)
        na, nb = (0 if rng.random() < 0.08 else _draw_n(rng, tile) for _ in range(2))
        if edge is not None:
            na, nb = [(_draw_n(rng, tile, edge), nb), (na, _draw_n(rng, tile, edge))][int(rng.integers(0, 2))]
        if na + nb == 0:     # (both empty: test_gpu_merge.py's test_both_empty)
            nb = 1
        has_v, has_k = mode in ("v4", "v8"), mode != "arg_only"
        c.update(kt=kt, mode=mode, na=na, nb=nb, tile=tile, ranges=str(rng.choice(["overlapping", "a_below_b", "b_below_a", "interleaved"])),
                 data_seed=int(rng.integers(0, 1 << 30)),
                 offs=[_draw_off(rng, ks), _draw_off(rng, vs if has_v else 0), _draw_off(rng, ks), _draw_off(rng, vs if has_v else 0),
                       _draw_off(rng, ks if has_k else 0), _draw_off(rng, vs)])
    return c


HAY_KINDS = ["specials", "equal", "distinct", "tie_run"]          # tie_run: one run longer than L laid across a pivot position
NEEDLE_KINDS = ["uniform", "hits", "neighbours", "below", "above", "one_key"]
SETOP_RANGES = ["overlapping", "a_below_b", "b_below_a", "interleaved", "a_eq_b", "a_subset_b"]
SETOP_RUNS = ["specials", "short", "distinct"]                     # + one long run in A, in B or in both: c["long"]
SELECT_KEYS = ["specials", "uniform"]
THRESHOLDS = ["present", "between", "least", "greatest"]
TOPK_KEYS = ["specials", "uniform", "few", "one_digit", "sorted", "reversed"]
# k itself, a uniform rank, or a place in the tie run of the key at a drawn rank of the sort (topk_inputs resolves it)
TOPK_CUTS = ["k=0", "k=1", "k=2", "k=n-1", "k=n", "k=n+1", "k=10n", "rank", "run_first", "run_inside", "run_last", "next_run_first"]


def _draw_search(rng, stratum, edge):
    kt, upper, flag = stratum
    ks = _size(TSE._NP[kt])
    tile = tile_of("search", ks, 0)
    P, L = search_limits(ks)
    if rng.random() < 0.4:
        nh = _HAY_EDGES[int(rng.integers(0, len(_HAY_EDGES)))](P, L)
        if rng.random() < 0.25:
            nh = max(0, nh + int(rng.integers(-2, 3)))
    else:
        nh = _draw_n(rng, L)
    nn = _draw_n(rng, tile, edge)
    hay = str(rng.choice(HAY_KINDS[:3] + (["tie_run"] * 3 if nh >= L + 3 else [])))
    tie = None
    if hay == "tie_run":                                   # pivot k of the general path lies at k * numel_h / P
        ln = L + 1 + int(rng.integers(0, min(L, nh - L - 2) + 1))
        piv = int(rng.integers(1, P)) * nh // P
        tie = (max(0, min(piv - int(rng.integers(0, ln)), nh - ln)), ln)
    return dict(kt=kt, upper=upper, sorted=flag, nh=nh, nn=nn, tile=tile, L=L, P=P, hay=hay, tie=tie,
                needles=str(rng.choice(NEEDLE_KINDS)) if nh else "uniform", data_seed=int(rng.integers(0, 1 << 30)),
                offs=[_draw_off(rng, ks), _draw_off(rng, ks), _draw_off(rng, 4)])


def _draw_setop(rng, stratum, obj, edge):
    kt, mode, op = stratum
    ks, vs = _size(TM._NP[kt]), obj[2]
    tile = tile_of("setop", ks, vs)
    na, nb = (0 if rng.random() < 0.08 else _draw_n(rng, tile) for _ in range(2))
    to_a = bool(rng.integers(0, 2))
    if edge is not None:
        na, nb = (_draw_n(rng, tile, edge), nb) if to_a else (na, _draw_n(rng, tile, edge))
    if na + nb == 0:         # (both empty: test_gpu_setop.py's thin-ABI test)
        na, nb = (0, 1) if to_a else (1, 0)
    ranges = str(rng.choice(SETOP_RANGES if na and nb else SETOP_RANGES[:4]))
    if ranges == "a_eq_b":   # the size that was dealt an edge stays
        na = nb = na if to_a else nb
    elif ranges == "a_subset_b" and na > nb:
        na, nb = nb, na
    long = None              # (where, the run's length in A, in B): longer than two tiles, of different lengths in both
    fits = [w for w, ok in (("a", na > 2 * tile + 1), ("b", nb > 2 * tile + 1), ("both", min(na, nb) > 2 * tile + 2)) if ok]
    if fits and rng.random() < 0.7:
        where = str(rng.choice(fits))
        length = lambda n: 2 * tile + 1 + int(rng.integers(0, min(tile, n - 2 * tile - 1) + 1))
        la, lb = length(na) if where != "b" else 0, length(nb) if where != "a" else 0
        if la == lb:
            la, lb = (la, lb + 1) if lb < nb else (la + 1, lb) if la < na else (la - 1, lb)
        long = (where, la, lb)
    has_v, has_k = mode in ("v4", "v8"), mode != "arg_only"
    return dict(kt=kt, mode=mode, op=op, na=na, nb=nb, tile=tile, ranges=ranges, runs=str(rng.choice(SETOP_RUNS)), long=long,
                pass_vb=bool(rng.integers(0, 2)), data_seed=int(rng.integers(0, 1 << 30)),
                offs=[_draw_off(rng, ks), _draw_off(rng, vs if has_v else 0), _draw_off(rng, ks), _draw_off(rng, vs if has_v else 0),
                      _draw_off(rng, ks if has_k else 0), _draw_off(rng, vs)])


def _draw_select(rng, stratum, obj, edge, state):
    """op and pred are dealt, not drawn, so that the committed seeds hold every (key type, pred) and every (op, pred):
    a comparison takes the next pred in turn for its key type, and every pred takes the two ops in turn, counted over all
    seeds in state. A case on the object of the case before keeps that case's (op, pred) half of the time when it may."""
    kt, mode, cls = stratum
    ks, vs = _size(TM._NP[kt]), obj[1]
    tile = tile_of("select", ks, vs)
    before = state["before"]
    if before is not None and (before["pred"] == "flagged") == (cls == "flagged") and rng.random() < 0.5:
        op, pred = before["op"], before["pred"]
    else:
        pred = "flagged"
        if cls == "cmp":
            turn = state.setdefault(("kt", kt), TM.KEY_TYPES.index(kt))
            state[("kt", kt)] = turn + 1
            pred = _SELECT_CMP[turn % len(_SELECT_CMP)]
        turn = state.setdefault(("pred", pred), 0)
        state[("pred", pred)] = turn + 1
        op = TSL.OPS[turn % 2]
    valued = mode in ("v4", "v8")
    return dict(kt=kt, mode=mode, op=op, pred=pred, n=_draw_n(rng, tile, edge), tile=tile, pattern=str(rng.choice(TSL.PATTERNS)),
                keys=str(rng.choice(SELECT_KEYS)), threshold=str(rng.choice(THRESHOLDS)) if cls == "cmp" else None, data_seed=int(rng.integers(0, 1 << 30)),
                offs=[_draw_off(rng, ks), _draw_off(rng, vs if valued else 0), _draw_off(rng, 1 if cls == "flagged" else ks),
                      _draw_off(rng, ks if mode in ("keys", "v4", "v8", "arg") else 0), _draw_off(rng, vs)])


def _draw_topk(rng, stratum, obj, edge, state):
    """which is dealt, not drawn, so that the committed seeds hold every (key type, which) and every (form, order,
    which): a case takes the direction that its key type and its (form, order) together have seen less often, counted
    over all seeds in state. A case on the object of the case before keeps that case's which half of the time when its
    order is the same: it then runs on the same CloTopK. The k-th key alone is asked of an "input" object. The byte that
    varies in "one_digit" keys is dealt as well."""
    kt, mode, order = stratum
    order = order or "input"
    ks, vs = _size(TM._NP[kt]), obj[1]
    tile = tile_of("topk", ks, vs)
    before = state["before"]
    seen = state.setdefault("which", {})
    if before is not None and before["order"] == order and rng.random() < 0.5:
        which = before["which"]
    else:
        turn = state["turn"] = state.get("turn", -1) + 1
        load = lambda w: (seen.get((kt, w), 0) + seen.get((mode, order, w), 0), seen.get((kt, w), 0), (TT.WHICH.index(w) + turn) % 2)
        which = min(TT.WHICH, key=load)
    for what in ((kt, which), (mode, order, which)):
        seen[what] = seen.get(what, 0) + 1
    import cl_ops_amd as clo
    keys = str(rng.choice(TOPK_KEYS))
    digit = None
    if keys == "one_digit":                                 # the varying byte is dealt too: a key size takes its bytes in turn
        digit = state[("digit", ks)] = (state.get(("digit", ks), -1) + 1) % ks
    return dict(kt=kt, mode=mode, order=order, which=which, n=_draw_n(rng, tile, edge), tile=tile, cap=int(clo.topk_sorted_max(ks, vs)), keys=keys,
                digit=digit, cut=str(rng.choice(TOPK_CUTS)), cut_u=[float(rng.random()), float(rng.random())],
                kth=bool(mode == "kth_only" or rng.integers(0, 2)), data_seed=int(rng.integers(0, 1 << 30)),
                offs=[_draw_off(rng, ks), _draw_off(rng, vs if mode in ("v4", "v8") else 0), _draw_off(rng, ks if mode in ("keys", "v4", "v8", "arg") else 0),
                      _draw_off(rng, vs), _draw_off(rng, ks)])


def draw_cases(family, seed):
    """The cases of one seed as plain descriptions. The seed's share of the family's strata (the list, shuffled once, is
    dealt to the seeds in turn) is walked in order, each with a new object; between them, at random places, as many cases
    again reuse the object of the case before on a random stratum it can run, with a size of their own. (select deals
    its preds and ops, and topk its directions, in turn over ALL the family's seeds, so the seeds before this one are
    drawn first: still a function of (family, seed) alone.)"""
    state = {}
    if family in ("select", "topk", "segsort"):
        for earlier in range(seed):
            _draw_seed(family, earlier, state)
    return _draw_seed(family, seed, state)


def _draw_seed(family, seed, state):
    strata = STRATA[family]
    order = np.random.default_rng(_SALT[family]).permutation(len(strata))
    share = _FRESH.get(family, -(-len(strata) // SEEDS[family]))
    mine = [strata[int(order[(seed * share + k) % len(strata)])] for k in range(share)]
    total = CASES[family]
    assert 0 <= seed < SEEDS[family] and total >= share
    rng = np.random.default_rng([_SALT[family], seed])
    fresh = np.zeros(total, bool)
    fresh[0] = True
    fresh[1 + rng.permutation(total - 1)[:share - 1]] = True
    edges = dict(zip((int(x) for x in rng.permutation(total)[:len(_EDGE_SIZES)]), range(len(_EDGE_SIZES))))
    cases, obj, k = [], None, 0
    for i in range(total):
        if fresh[i]:
            stratum, k = mine[k], k + 1
            obj = _object_for(family, rng, stratum)
        else:
            options = compatible(family, obj)
            stratum = options[int(rng.integers(0, len(options)))]
        c = {"family": family, "seed": seed, "case": i, "reuse": not fresh[i], "object": obj}
        state["before"] = cases[-1] if cases and not fresh[i] else None         # the case before, on the same object
        c.update(_draw_call(family, rng, stratum, obj, edges.get(i), state))
        assert stratum_of(c) == stratum, (c, stratum)
        cases.append(c)
    return cases


def stratum_of(c):
    """The kernel instantiation a case launches, from the arguments of its call alone."""
    f = c["family"]
    if f == "expand":
        return (c["form"], c["ct"], c["vs"])
    if f == "segreduce":
        return (c["form"], c["ct"], (c["vt"], c["st"]), c["op"])
    if f == "segsort":
        return (c["kt"], c["mode"], c["form"], c["ct"])
    if f in ("rbk", "sbk"):
        ks = _size(TR._NP[c["kt"]])
        if f == "rbk" and not c["want_a"]:
            kind = "keys_only"
        elif c["vt"] is None:
            kind = "len_" + c["st"]
        else:
            kind = (c["vt"], c["st"], c["op"])
        return (ks, kind) if f == "rbk" else (ks, kind, c["inclusive"])
    if f == "hist":
        info = np.iinfo(TH._NP[c["kt"]])
        copies, L = hist_limits(_size(TH._NP[c["st"]]))
        cvt = "cnt_" + c["st"] if c["vt"] is None else "%s->%s" % (c["vt"], c["st"])
        return (info.bits // 8, int(info.min < 0), cvt, "copies" if c["num_bins"] <= copies else "peel" if c["num_bins"] <= L else "global")
    if f == "search":
        return (c["kt"], c["upper"], c["sorted"])
    if f == "setop":
        return (c["kt"], c["mode"], c["op"])
    if f == "select":
        return (c["kt"], c["mode"], "flagged" if c["pred"] == "flagged" else "cmp")
    if f == "topk":                 # (with neither output the call ends after the digit sweeps, whatever the object's order)
        return (c["kt"], c["mode"], None if c["mode"] == "kth_only" else c["order"])
    return (c["kt"], c["mode"])


def by_key_inputs(c):
    """(keys, values) of a reduce-by-key or scan-by-key case."""
    n, tile, s = c["n"], c["tile"], c["structure"]
    if s["kind"] == "unsorted":
        runs = TR.structure("unsorted", n, tile, seed=s["seed"])
    else:
        parts, base = [], 0
        bounds = [0] + list(s["cuts"]) + [n]
        for k, mean in enumerate(s["means"]):
            r = TR.structure("geo%d" % mean, bounds[k + 1] - bounds[k], tile, seed=s["seed"] + k)
            parts.append(r + base)
            base += int(r[-1]) + 1 if r.size else 0
        runs = np.concatenate(parts).astype(np.int64)
    if s["long"]:
        at, ln = s["long"]
        runs[at:at + ln] = runs[at]
    return TR.make_keys(c["kt"], runs, seed=c["palette_seed"]), TR.make_values(c["vt"], n, c["value_seed"])


def longest_run(keys):
    if not keys.size:
        return 0
    return int(np.diff(np.append(np.flatnonzero(sbk_model.heads_of(keys)), keys.size)).max())


def hist_inputs(c):
    """(keys, values, prior content of hist_out) of a histogram case."""
    kt, n, lower, shift, nb = c["kt"], c["n"], c["lower"], c["shift"], c["num_bins"]
    rng = np.random.default_rng(c["data_seed"])
    bits = lambda m: rng.integers(0, 1 << 63, m, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, m, dtype=np.uint64)
    if c["layout"] == "handful":
        few = rng.integers(0, TH.span_of(kt, lower, shift, nb), 5, dtype=np.uint64)
        near = TH.key_at(kt, lower, few[rng.integers(0, 5, n)])
    else:
        near = TH.make_keys(kt, c["layout"], n, lower, shift, nb, seed=c["data_seed"])
    anywhere = bits(n).astype(TH._UBITS[near.itemsize]).view(near.dtype)
    keys = np.where(rng.random(n) < c["outside"], anywhere, near)
    sdt = np.dtype(TH._NP[c["st"]])
    return keys, TH.make_values(c["vt"], n, c["data_seed"]), bits(nb).astype(TH._UBITS[sdt.itemsize]).view(sdt)


def merge_inputs(c):
    """(keys_a, keys_b) of a merge case, both in the merge's order."""
    kt, na, nb, seed = c["kt"], c["na"], c["nb"], c["data_seed"]
    if c["ranges"] == "overlapping":
        return TM.keys_of_type(kt, na, seed), TM.keys_of_type(kt, nb, seed + 1)
    both = TM.keys_of_type(kt, na + nb, seed)
    if c["ranges"] == "a_below_b":
        return both[:na], both[na:]
    if c["ranges"] == "b_below_a":
        return both[nb:], both[:nb]
    to_a = np.zeros(na + nb, bool)
    to_a[np.random.default_rng(seed).permutation(na + nb)[:na]] = True
    return both[to_a], both[~to_a]


def _ubits(rng, n, ut):
    """n uniform words of the unsigned type ut."""
    return rng.integers(0, 1 << (8 * np.dtype(ut).itemsize), n, dtype=np.uint64).astype(ut)


def key_of_order(o, dt):
    """The inverse of merge_model.order_key: the keys of type dt whose order keys are o."""
    dt = np.dtype(dt)
    ut = np.dtype(TM._U[dt.itemsize])
    o = np.ascontiguousarray(o, dtype=ut)
    sign = ut.type(1 << (8 * ut.itemsize - 1))
    if dt.kind == "u":
        return o.view(dt).copy()
    if dt.kind == "i":
        return (o ^ sign).view(dt)
    return np.where((o & sign) != 0, o ^ sign, ~o).view(dt)


def search_inputs(c):
    """(haystack, needles) of a search case: the haystack in the library's order, the needles too where the case
    promises it."""
    kt, nh, nn = c["kt"], c["nh"], c["nn"]
    dt = np.dtype(TSE._NP[kt])
    ut = np.dtype(TM._U[dt.itemsize])
    rng = np.random.default_rng(c["data_seed"])
    if c["hay"] == "specials":
        hay = TM.keys_of_type(kt, nh, c["data_seed"])
    elif c["hay"] == "equal":
        hay = np.repeat(TM.keys_of_type(kt, 1, c["data_seed"]), nh)
    else:
        hay = sort_keys(_ubits(rng, nh, ut).view(dt))
        if c["tie"]:
            at, ln = c["tie"]
            hay[at:at + ln] = hay[at]
    oh = order_key(hay)
    top = (1 << (8 * dt.itemsize)) - 1
    kind = c["needles"]
    if kind == "hits":
        o = oh[rng.integers(0, nh, nn)]
    elif kind == "neighbours":                              # +-1 in order-key space (it wraps at the ends)
        o = oh[rng.integers(0, nh, nn)] + np.where(rng.random(nn) < 0.5, 1, top).astype(ut)
    elif kind == "below":                                   # (a first key that is the type's least has nothing below it)
        o = rng.integers(0, max(int(oh[0]), 1), nn, dtype=np.uint64).astype(ut)
    elif kind == "above":
        o = rng.integers(min(int(oh[-1]) + 1, top), top, nn, dtype=np.uint64, endpoint=True).astype(ut)
    else:
        o = order_key(_ubits(rng, nn, ut).view(dt))
        if kind == "one_key":
            o[rng.random(nn) < 0.9] = oh[rng.integers(0, nh)]
    ndl = key_of_order(o, dt)
    return hay, (sort_keys(ndl) if c["sorted"] else ndl)


def _setop_keys(c, n, which):
    """n sorted keys of a setop case; which numbers the draw (A and B take their keys from one pool)."""
    kt, seed = c["kt"], c["data_seed"]
    if c["runs"] == "specials":
        return TM.keys_of_type(kt, n, seed + which)
    dt = np.dtype(TM._NP[kt])
    total = c["na"] + c["nb"]
    distinct = max(2, total // 4) if c["runs"] == "short" else 4 * total + 2
    pool = _ubits(np.random.default_rng(seed), distinct, TM._U[dt.itemsize])
    return sort_keys(pool[np.random.default_rng([seed, which]).integers(0, distinct, n)].view(dt))


def _long_run(keys, x, ln, seed):
    """keys with ln elements somewhere replaced by the key x, in order again."""
    if not ln:
        return keys
    at = int(np.random.default_rng([seed, ln]).integers(0, keys.size - ln + 1))
    keys = keys.copy()
    keys[at:at + ln] = x
    return sort_keys(keys)


def setop_inputs(c):
    """(keys_a, keys_b) of a setop case, both in the library's order."""
    na, nb, seed = c["na"], c["nb"], c["data_seed"]
    _, la, lb = c["long"] or (None, 0, 0)
    if c["ranges"] in ("a_eq_b", "a_subset_b"):              # the long run is B's, and A's through B
        b = _setop_keys(c, nb, 1)
        ln = min(max(la, lb), nb)
        b = _long_run(b, b[nb // 2], ln, seed)
        if c["ranges"] == "a_eq_b":
            return b.copy(), b
        return b[np.sort(np.random.default_rng(seed).permutation(nb)[:na])], b
    if c["ranges"] == "overlapping":
        a, b = _setop_keys(c, na, 1), _setop_keys(c, nb, 2)
    else:
        both = _setop_keys(c, na + nb, 1)
        if c["ranges"] == "a_below_b":
            a, b = both[:na], both[na:]
        elif c["ranges"] == "b_below_a":
            a, b = both[nb:], both[:nb]
        else:
            to_a = np.zeros(na + nb, bool)
            to_a[np.random.default_rng(seed).permutation(na + nb)[:na]] = True
            a, b = both[to_a], both[~to_a]
    if c["long"]:
        x = (a if la else b)[(na if la else nb) // 2]        # one key for both runs
        a, b = _long_run(a, x, la, seed), _long_run(b, x, lb, seed + 1)
    return a, b


def select_inputs(c):
    """(keys, flags or the threshold) of a select case, the typed sibling of test_gpu_select.py's inputs_for: the keep
    pattern decides which elements are kept. By flags: a kept element's flag is any byte but 0. By comparison: the keys
    come from a pool (the type's specials, or uniform words) that the threshold splits into those the pred keeps and the
    others, and every element draws from its side; where one side is empty (nothing is below the type's least key) all
    elements draw from the other, and the pattern gives way."""
    kt, n, pred = c["kt"], c["n"], c["pred"]
    dt = np.dtype(TM._NP[kt])
    ut = np.dtype(TM._U[dt.itemsize])
    rng = np.random.default_rng(c["data_seed"])
    mask = TSL.mask_of(c["pattern"], n, c["tile"], c["data_seed"])
    pool = np.unique(order_key(TM.keys_of_type(kt, 64, c["data_seed"]) if c["keys"] == "specials" else _ubits(rng, 4096, ut).view(dt)))
    if pred == "flagged":
        return key_of_order(pool[rng.integers(0, pool.size, n)], dt), np.where(mask, rng.integers(1, 256, n), 0).astype(np.uint8)
    top = (1 << (8 * dt.itemsize)) - 1
    if c["threshold"] == "present":
        t = pool[rng.integers(0, pool.size)]
    elif c["threshold"] == "between":                       # a key of the pool's inside that is then taken out of it
        assert pool.size >= 3
        t = pool[rng.integers(1, pool.size - 1)]
        pool = pool[pool != t]
    else:
        t = ut.type(0 if c["threshold"] == "least" else top)
        if rng.random() < 0.5:
            pool = np.unique(np.append(pool, t))
    sides = {"lt": pool < t, "le": pool <= t, "gt": pool > t, "ge": pool >= t, "eq": pool == t, "ne": pool != t}[pred]
    kept, rest = pool[sides], pool[~sides]
    if not kept.size or not rest.size:
        kept = rest = pool
    o = np.where(mask, kept[rng.integers(0, kept.size, n)], rest[rng.integers(0, rest.size, n)])
    for side, there in ((kept, mask), (rest, ~mask)):       # a threshold of the pool occurs often on its side, not once in the pool's size
        if (side == t).any():
            o[there & (rng.random(n) < 0.2)] = t
    return key_of_order(o, dt), key_of_order(np.array([t], ut), dt)[0]


def topk_inputs(c):
    """(keys, k) of a topk case. The cut is resolved here, on the keys: a rank r of the sort in the case's direction is
    drawn below numel (for "sorted" below the cap too), and k takes the first element of the tie run of the key at r, an
    element strictly inside it (the first where the run has fewer than three), its last, or the first of the next run.
    Where a "sorted" case then has min(k, numel) above the cap, k is the cap: no case is refused."""
    kt, n, cut = c["kt"], c["n"], c["cut"]
    dt = np.dtype(TM._NP[kt])
    ut = np.dtype(TM._U[dt.itemsize])
    rng = np.random.default_rng(c["data_seed"])
    if c["keys"] == "specials":
        keys = rng.permutation(TM.keys_of_type(kt, n, c["data_seed"]))
    elif c["keys"] == "uniform":
        keys = _ubits(rng, n, ut).view(dt)
    elif c["keys"] == "few":                                # ties that run over every tile
        pool = _ubits(rng, int(rng.integers(2, 6)), ut)
        keys = pool[rng.integers(0, pool.size, n)].view(dt)
    elif c["keys"] == "one_digit":                          # one byte of the order key varies
        shift = 8 * c["digit"]
        rest = int(_ubits(rng, 1, ut)[0]) & ~(0xFF << shift)
        keys = key_of_order((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(shift) | np.uint64(rest)).astype(ut), dt)
    else:                                                   # in the library's order, ascending or descending, with ties
        pool = _ubits(rng, n // 3 + 1, ut).view(dt)
        keys = sort_keys(pool[rng.integers(0, pool.size, n)])
        if c["keys"] == "reversed":
            keys = keys[::-1]
    keys = np.ascontiguousarray(keys)
    fixed = {"k=0": 0, "k=1": 1, "k=2": 2, "k=n-1": max(n - 1, 0), "k=n": n, "k=n+1": n + 1, "k=10n": 10 * n}
    lim = min(n, c["cap"]) if c["order"] == "sorted" else n
    if cut in fixed:
        k = fixed[cut]
    elif not lim:
        k = 1
    else:
        x = order_key(keys)
        xs = np.sort(~x if c["which"] == "largest" else x)
        r = int(c["cut_u"][0] * lim)
        lo, hi = int(np.searchsorted(xs, xs[r], "left")), int(np.searchsorted(xs, xs[r], "right"))     # the run holds ranks lo .. hi - 1
        k = {"rank": r + 1, "run_first": lo + 1, "run_inside": lo + 2 + int(c["cut_u"][1] * (hi - lo - 2)) if hi - lo >= 3 else lo + 1,
             "run_last": hi, "next_run_first": hi + 1}[cut]
    if c["order"] == "sorted" and min(k, n) > c["cap"]:
        k = c["cap"]
    return keys, int(k)


# ---- expand, the segmented reduction and the segmented sort: segments from counts or offsets ----

SEG_EMPTY = [0.0, 0.1, 0.5]                                          # the share of empty segments
PLACES = ["at", "below", "above"]                                    # the capacity (expand) or the rows, against the total
NUM_INS = ["absent", "below", "at", "above"]                         # num_in against numel_seg
BASES = ["zero", "small", "top"]                                     # offsets[0]; top: a uint array ends at 2^32 - 1, a ulong one lies above 2^40
SEGSORT_KEYS = ["random bits", "specials", "few", "all equal", "sorted", "reversed", "sorted per segment", "one byte varies"]


def _draw_segments(rng, n, tile, L, family):
    """A mixture of geometric stretches (each with a mean of its own from 1 to 50 000), a share of empty segments, one
    segment longer than two tiles where n allows it, sometimes a run of more than L empty segments (expand's per-row
    search) and sometimes more segments than rows."""
    parts = int(rng.integers(1, 5))
    s = {"seed": int(rng.integers(0, 1 << 30)), "cuts": sorted(int(x) for x in rng.integers(0, n + 1, parts - 1)),
         "means": [max(1, int(50000.0 ** rng.random())) for _ in range(parts)], "empty": float(rng.choice(SEG_EMPTY)), "long": None,
         "empty_run": L + 1 + int(rng.integers(0, L)) if rng.random() < 0.2 else 0, "many": bool(rng.random() < 0.15)}
    if n > 2 * tile + 1:
        ln = 2 * tile + 1 + int(rng.integers(0, min(tile, n - 2 * tile - 1) + 1))
        room = n - ln if family != "segreduce" else (n - ln) // 3        # (segreduce's n are merge steps: the rows are cut to fit)
        s["long"] = (int(rng.integers(0, room + 1)), ln)
    return s


def _draw_segmented(family, rng, stratum, edge, state):
    import cl_ops_amd as clo
    L = int(clo.expand_lds_segments())
    c = {}
    if family == "expand":
        form, ct, vs = stratum
        tile = int(clo.expand_tile(vs))
        outs = TE.SUBSETS[int(rng.integers(0, len(TE.SUBSETS)))]
        if not vs:
            outs = [o for o in TE.SUBSETS if not o[0]][int(rng.integers(0, 3))]
        sizes = [vs if outs[0] else 0, vs if outs[0] else 0, 4 if outs[1] else 0, 4 if outs[2] else 0]
        c.update(vs=vs, outs=[bool(o) for o in outs])
    elif family == "segreduce":
        form, ct, (vt, st), op = stratum
        sizes = [_size(TSR.NP[vt]), _size(TSR.NP[st])]
        tile = int(clo.segreduce_tile(*sizes))
        c.update(vt=vt, st=st, op=op, plant=[int(rng.integers(0, 50)), int(rng.integers(0, 50)), int(rng.integers(0, 2))])
    else:
        kt, mode, form, ct = stratum
        ks, vs = _size(TSS.KEY_NP[kt]), TSS.VS[mode]
        tile = int(clo.segsort_tile(ks, vs))
        sizes = [ks, vs if mode in ("v4", "v8") else 0, ks if mode != "arg without keys_out" else 0, vs]
        keys = str(rng.choice(SEGSORT_KEYS))
        digit = None
        if keys == "one byte varies":                            # the varying byte is dealt: a key size takes its bytes in turn
            digit = state[("digit", ks)] = (state.get(("digit", ks), -1) + 1) % ks
        c.update(kt=kt, mode=mode, keys=keys, digit=digit)
    assert tile > 0
    n = _draw_n(rng, tile, edge)
    c.update(form=form, ct=ct, n=n, tile=tile, L=L, segments=_draw_segments(rng, n, tile, L, family), place=str(rng.choice(PLACES)),
             place_by=int(rng.integers(1, tile)), num_in=str(rng.choice(NUM_INS)), num_in_u=float(rng.random()),
             base=str(rng.choice(BASES)) if form == "offsets" else "zero", data_seed=int(rng.integers(0, 1 << 30)),
             offs=[_draw_off(rng, _size(TE.CDT[ct]))] + [_draw_off(rng, x) for x in sizes])
    return c


def segment_counts(c):
    """The counts of a case: their sum is c["n"] rows; for segreduce the counts and their number together are c["n"] merge
    steps (the segments are cut off where the steps run out, and a last segment takes what is left)."""
    s, n = c["segments"], c["n"]
    rng = np.random.default_rng(s["seed"])
    bounds = [0] + list(s["cuts"]) + [n]
    ends = [np.zeros(0, np.int64)]
    for k, mean in enumerate(s["means"]):
        if bounds[k + 1] > bounds[k]:
            ends.append(bounds[k] + np.cumsum(TSS.geometric_fill(rng, bounds[k + 1] - bounds[k], mean)))
    e = np.unique(np.concatenate(ends))
    if s["long"]:
        at, ln = s["long"]
        e = np.unique(np.concatenate((e[(e <= at) | (e >= at + ln)], [at + ln] + ([at] if at else []))))
    counts = np.diff(np.concatenate(([0], e))).astype(np.int64)
    zeros = lambda k: np.zeros(k, np.int64)
    if s["empty"]:
        k = int(round(counts.size * s["empty"] / (1.0 - s["empty"])))
        counts = np.insert(counts, np.sort(rng.integers(0, counts.size + 1, k)), zeros(k))
    if s["empty_run"]:
        counts = np.insert(counts, int(rng.integers(0, counts.size + 1)), zeros(s["empty_run"]))
    if s["many"]:                                                     # more segments than rows
        k = n + 1 + int(rng.integers(0, n // 4 + 1))
        counts = np.insert(counts, np.sort(rng.integers(0, counts.size + 1, k)), zeros(k))
    if c["family"] == "segreduce":
        steps = np.cumsum(counts + 1)
        keep = int(np.searchsorted(steps, n, "right"))
        rest = n - (int(steps[keep - 1]) if keep else 0)
        counts = np.concatenate((counts[:keep], [rest - 1] if rest else []))
        assert int(counts.sum()) + counts.size == n
    else:
        if not counts.size:
            counts = zeros(1 + int(rng.integers(0, 3)))              # (at least one segment: numel_seg 0 has tests of its own)
        assert int(counts.sum()) == n
    return counts.astype(np.int64)


def segmented_args(c, counts):
    """(the capacity or the rows, num_in, the offsets' base) of a case, resolved on its counts."""
    m, total = counts.size, int(counts.sum())
    num_in = {"absent": None, "below": int(c["num_in_u"] * m), "at": m, "above": m + 1 + int(c["num_in_u"] * 1000)}[c["num_in"]]
    seen = total if num_in is None else int(counts[:num_in].sum())    # the total of the segments the call takes
    rows = {"at": seen, "below": max(seen - c["place_by"], 0), "above": seen + c["place_by"]}[c["place"]]
    base = {"zero": 0, "small": 1 + c["data_seed"] % 100000, "top": (1 << 32) - 1 - total if c["ct"] == "uint" else (1 << 40) + c["data_seed"]}[c["base"]]
    return rows, num_in, base


def expand_inputs(c):
    """(counts, capacity, num_in, base) of an expand case."""
    counts = segment_counts(c)
    return (counts,) + segmented_args(c, counts)


def segreduce_inputs(c):
    """(counts, values, num_in, base) of a segreduce case: TSR.values_for's values, and in every segment that crosses
    a tile edge by more than 100 merge steps on both sides the type's least and greatest value planted, one before and one
    behind the first edge inside it."""
    counts = segment_counts(c)
    rows, num_in, base = segmented_args(c, counts)
    vals = TSR.values_for(c["vt"], rows, c["data_seed"])
    info = np.iinfo(vals.dtype)
    T = c["tile"]
    idx = np.flatnonzero(counts > 200)
    start = np.cumsum(counts) - counts
    for r in idx.tolist():
        s, ln = int(start[r]), int(counts[r])
        edge = -(-(s + r + 1) // T) * T                               # the first tile edge behind the segment's first merge step s + r
        before, behind = s + (edge - (s + r)) - 1 - c["plant"][0], s + (edge - (s + r)) + c["plant"][1]
        if s + 50 <= before and behind < min(s + ln, rows) - 50:
            lo, hi = (before, behind) if c["plant"][2] else (behind, before)
            vals[lo], vals[hi] = info.min, info.max
    return counts, vals, num_in, base


def segsort_inputs(c):
    """(counts, keys, num_in, base) of a segsort case."""
    counts = segment_counts(c)
    n, num_in, base = segmented_args(c, counts)
    kt, kind = c["kt"], c["keys"]
    dt = np.dtype(TSS.KEY_NP[kt])
    ut = np.dtype(TM._U[dt.itemsize])
    rng = np.random.default_rng(c["data_seed"])
    if kind == "random bits":
        keys = _ubits(rng, n, ut).view(dt)
    elif kind == "specials":                                  # both zeros, NaNs of both signs with payloads, infinities, the types' extremes
        keys = rng.permutation(TM.keys_of_type(kt, n, c["data_seed"]))
    elif kind == "few":
        pool = _ubits(rng, int(rng.integers(2, 9)), ut)
        keys = pool[rng.integers(0, pool.size, n)].view(dt)
    elif kind == "all equal":
        keys = np.repeat(_ubits(rng, 1, ut), n).view(dt)
    elif kind == "one byte varies":
        shift = 8 * c["digit"]
        rest = int(_ubits(rng, 1, ut)[0]) & ~(0xFF << shift)
        keys = key_of_order((rng.integers(0, 256, n, dtype=np.uint64) << np.uint64(shift) | np.uint64(rest)).astype(ut), dt)
    else:                                                     # with ties: in the library's order over the whole array, reversed, or per segment
        pool = _ubits(rng, n // 3 + 1, ut).view(dt)
        keys = pool[rng.integers(0, pool.size, n)]
        if kind == "sorted per segment":                      # already the answer
            keys = np.ascontiguousarray(keys)
            p, _ = segsort(c["form"], TSS.source(c["form"], c["ct"], counts, base), keys, num_in)
            keys[:p.size] = keys[p]
        else:
            keys = sort_keys(keys)[::-1] if kind == "reversed" else sort_keys(keys)
    return counts, np.ascontiguousarray(keys), num_in, base


def _make_object(clo, ctx, family, obj):
    if family == "expand":
        return clo.Expand(obj[0], ctx, TE.VTYPE.get(obj[2]), obj[1])
    if family == "segreduce":
        return clo.SegReduce(obj[3], obj[0], ctx, obj[2][0], obj[2][1], obj[1])
    if family == "segsort":
        return clo.SegSort(obj[2], ctx, obj[0], obj[1], obj[3])
    if family == "rbk":
        return clo.ReduceByKey(ctx, obj[0], obj[1], obj[2], op=obj[3])
    if family == "sbk":
        return clo.ScanByKey(ctx, obj[0], obj[1], obj[2], op=obj[3], inclusive=obj[4])
    if family == "hist":
        return clo.Histogram(ctx, obj[0], obj[1], obj[2], options="accumulate" if obj[3] else None)
    if family == "search":
        return clo.Search(ctx, obj[0])
    if family == "setop":
        return clo.SetOp(obj[0], ctx, obj[1], obj[2])
    if family == "select":
        return _Selects(clo, ctx, obj[0], obj[1])
    if family == "topk":
        return _TopKs(clo, ctx, obj[0], obj[1])
    return clo.Merge(ctx, obj[0], obj[1])


class _Selects:
    """The fuzz's object of the select family: the CloSelect objects of one (key type, value size), one per (op, pred)
    asked for, all alive until the next object replaces this one. op and pred are arguments of clo_select_new, yet no
    kernel is built for them (include/clo_select.h), so a case that keeps the (op, pred) of the case before reuses that
    CloSelect and its workspace at a size of its own, and one that does not gets a second one next to it."""

    def __init__(self, clo, ctx, kt, vs):
        self.made, self.new = {}, lambda op, pred: clo.Select(op, pred, ctx, kt, vs)

    def get(self, op, pred):
        if (op, pred) not in self.made:
            self.made[(op, pred)] = self.new(op, pred)
        return self.made[(op, pred)]

    def close(self):
        for s in self.made.values():
            s.close()
        self.made = {}


class _TopKs(_Selects):
    """The same for topk: the CloTopK objects of one (key type, value size), one per (which, order) asked for. which and
    order are arguments of clo_topk_new (include/clo_topk.h), so a case that keeps the (which, order) of the case before
    reuses that CloTopK and its workspace (the digit tables, states and counts of the call before still in it) at a size
    of its own."""

    def __init__(self, clo, ctx, kt, vs):
        self.made, self.new = {}, lambda which, order: clo.TopK(which, order, ctx, kt, vs)


def _run_one(dev, c, handle):
    """The family's own run_case / run_merge: outputs equal the model, rows beyond m untouched, guards intact, inputs
    unchanged, the run count exact."""
    f, what = c["family"], "%s seed %d case %d" % (c["family"], c["seed"], c["case"])
    if f == "expand":
        counts, capacity, num_in, base = expand_inputs(c)
        TE.run_expand(dev, c["form"], c["ct"], c["vs"], tuple(c["outs"]), counts, what, capacity=capacity, num_in=num_in, base=base, offs=tuple(c["offs"]),
                      obj=handle)
    elif f == "segreduce":
        counts, vals, num_in, base = segreduce_inputs(c)
        TSR.run_seg(dev, c["op"], c["form"], c["ct"], c["vt"], c["st"], counts, vals.size, what, num_in=num_in, base=base, offs=tuple(c["offs"]), obj=handle,
                    vals=vals)
    elif f == "segsort":
        counts, keys, num_in, base = segsort_inputs(c)
        TSS.run_sort(dev, c["form"], c["ct"], c["kt"], c["mode"], counts, keys.size, what + ", %s keys" % c["keys"], num_in=num_in, base=base,
                     offs=tuple(c["offs"]), obj=handle, seed=c["data_seed"] % 1000, keys=keys)
    elif f == "rbk":
        keys, values = by_key_inputs(c)
        TR.run_case(dev, c["kt"], c["vt"], c["st"], c["op"], keys, values, what, offs=tuple(c["offs"]), want_k=c["want_k"], want_a=c["want_a"], obj=handle)
    elif f == "sbk":
        keys, values = by_key_inputs(c)
        TS.run_case(dev, c["kt"], c["vt"], c["st"], c["op"], c["inclusive"], keys, values, what, offs=tuple(c["offs"]), in_place=c["in_place"], obj=handle)
    elif f == "hist":
        keys, values, prior = hist_inputs(c)
        assert handle.accumulate == c["accumulate"]
        TH.run_case(dev, c["kt"], c["vt"], c["st"], keys, values, c["lower"], c["shift"], c["num_bins"], what, offs=tuple(c["offs"]), obj=handle, prefill=prior)
    elif f == "merge":
        a, b = merge_inputs(c)
        TM.run_merge(dev, c["kt"], a, b, c["mode"], what, offs=tuple(c["offs"]), obj=handle)
    elif f == "search":
        hay, ndl = search_inputs(c)
        TSE.run_search(dev, c["kt"], hay, ndl, ((c["upper"], c["sorted"]),), what, offs=tuple(c["offs"]), obj=handle)
    elif f == "setop":
        a, b = setop_inputs(c)
        TSO.run_setop(dev, c["op"], c["kt"], a, b, c["mode"], what, offs=tuple(c["offs"]), obj=handle, pass_vb=c["pass_vb"])
    elif f == "topk":
        keys, k = topk_inputs(c)
        TT.run_topk(dev, c["which"], c["order"], c["kt"], keys, k, c["mode"], what + ", %s keys, cut %s" % (c["keys"], c["cut"]), offs=tuple(c["offs"]),
                    obj=handle.get(c["which"], c["order"]), kth=c["kth"])
    else:
        keys, fot = select_inputs(c)
        TSL.run_select(dev, c["op"], c["pred"], c["kt"], keys, fot, c["mode"], what, offs=tuple(c["offs"]), obj=handle.get(c["op"], c["pred"]))


def _fuzz_family(gpu, family, seed):
    import cl_ops_amd as clo
    ctx, q = gpu
    dev = (clo, ctx, q)
    handle = None
    try:
        for c in draw_cases(family, seed):
            try:
                if not c["reuse"]:
                    if handle is not None:
                        handle.close()
                    handle = _make_object(clo, ctx, family, c["object"])
                _run_one(dev, c, handle)
            except Exception as e:  # noqa: BLE001 (the description makes the failure reproducible from the message alone)
                raise AssertionError("fuzz %s seed %d case %d: %s: %s\n%r" % (family, seed, c["case"], type(e).__name__, e, c)) from e
    finally:
        if handle is not None:
            handle.close()


@pytest.mark.parametrize("seed", range(SEEDS["rbk"]))
def test_fuzz_reduce_by_key(gpu, seed):
    _fuzz_family(gpu, "rbk", seed)


@pytest.mark.parametrize("seed", range(SEEDS["sbk"]))
def test_fuzz_scan_by_key(gpu, seed):
    _fuzz_family(gpu, "sbk", seed)


@pytest.mark.parametrize("seed", range(SEEDS["hist"]))
def test_fuzz_histogram(gpu, seed):
    _fuzz_family(gpu, "hist", seed)


@pytest.mark.parametrize("seed", range(SEEDS["merge"]))
def test_fuzz_merge(gpu, seed):
    _fuzz_family(gpu, "merge", seed)


@pytest.mark.parametrize("seed", range(SEEDS["search"]))
def test_fuzz_search(gpu, seed):
    _fuzz_family(gpu, "search", seed)


@pytest.mark.parametrize("seed", range(SEEDS["setop"]))
def test_fuzz_setop(gpu, seed):
    _fuzz_family(gpu, "setop", seed)


@pytest.mark.parametrize("seed", range(SEEDS["select"]))
def test_fuzz_select(gpu, seed):
    _fuzz_family(gpu, "select", seed)


@pytest.mark.parametrize("seed", range(SEEDS["topk"]))
def test_fuzz_topk(gpu, seed):
    _fuzz_family(gpu, "topk", seed)


@pytest.mark.parametrize("seed", range(SEEDS["expand"]))
def test_fuzz_expand(gpu, seed):
    _fuzz_family(gpu, "expand", seed)


@pytest.mark.parametrize("seed", range(SEEDS["segreduce"]))
def test_fuzz_segreduce(gpu, seed):
    _fuzz_family(gpu, "segreduce", seed)


@pytest.mark.parametrize("seed", range(SEEDS["segsort"]))
def test_fuzz_segsort(gpu, seed):
    _fuzz_family(gpu, "segsort", seed)
