"""The host side of the executed reference (test infrastructure).

oracle/ref_build.py compiles upstream's OpenCL C kernels for the host into oracle/_ref/libclo_ref_<config>.so;
this module loads those libraries and drives them with upstream's launch loops. The kernels that run are
upstream's program text. The loops below are a restatement of upstream's host code (it needs cf4ocl2 and GLib,
which are absent); every one cites the host file and lines it follows (paths relative to the reference tree's
src/cl_ops/). ccl_kernel_suggest_worksizes belongs to cf4ocl2, which is not in the tree: it follows SURVEY §8b.

Every buffer a kernel sees, __local scratch included, sits between two canary margins that are checked after
each launch: upstream's kernels check no bounds. The drivers therefore refuse the shapes upstream itself cannot
run (RefusedShape). Single-threaded: see oracle/clo_ref_rt.c.
"""
import ctypes as C
import os
import sys

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_DIR = os.path.join(_ROOT, "oracle", "_ref")
MARGIN = 512                      # bytes of canary on each side of every buffer
CANARY = 0xC5
NP_TYPES = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
            "long": np.int64, "ulong": np.uint64, "float": np.float32, "double": np.float64}
TYPE_NAMES = {np.dtype(v): k for k, v in NP_TYPES.items()}

LAUNCHES = []                     # (config, kernel, gws, lws) of every launch since the last clear()
CANARY_CHECKS = [0]               # number of margins verified


class RefusedShape(ValueError):
    """A shape upstream's kernels cannot run without leaving their buffers."""


class CanaryError(AssertionError):
    pass


def _ref_build():
    sys.path.insert(0, os.path.join(_ROOT, "oracle"))
    try:
        import ref_build
    finally:
        sys.path.pop(0)
    return ref_build


def reference_present():
    return _ref_build().have_reference()


def available():
    """True when the executed reference can be used: libraries are there, or can be expected to be."""
    return os.path.isdir(REF_DIR) or reference_present()


class Buf:
    """A numpy array between two canary margins."""

    def __init__(self, arr=None, dtype=None, count=None, fill=None):
        if arr is not None:
            arr = np.ascontiguousarray(arr)
            dtype, count = arr.dtype, arr.size
        self.nbytes = int(count) * np.dtype(dtype).itemsize
        self.raw = np.full(self.nbytes + 2 * MARGIN, CANARY, np.uint8)
        self.a = self.raw[MARGIN:MARGIN + self.nbytes].view(dtype)
        if arr is not None:
            self.a[:] = arr.reshape(-1)
        elif fill is not None:
            self.raw[MARGIN:MARGIN + self.nbytes] = fill
        self.ptr = C.c_void_p(self.raw.ctypes.data + MARGIN)

    def check(self, what=""):
        CANARY_CHECKS[0] += 2
        if not (np.all(self.raw[:MARGIN] == CANARY) and np.all(self.raw[MARGIN + self.nbytes:] == CANARY)):
            raise CanaryError("a kernel wrote outside its buffer: " + what)


def local(nbytes):
    """__local memory of one work-group: uninitialised on a device, a recognisable pattern here."""
    return Buf(dtype=np.uint8, count=nbytes, fill=0xA5)


class Lib:
    _cache = {}

    def __init__(self, config):
        path = os.path.join(REF_DIR, "libclo_ref_%s.so" % config)
        if not os.path.exists(path):
            raise FileNotFoundError("executed reference library missing: %s (run oracle/ref_build.py)" % path)
        self.config = config
        self.dll = C.CDLL(path)
        self.dll.clo_ref_launch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_size_t, C.c_int]
        self.dll.clo_ref_launch.restype = C.c_int
        self.names = C.string_at(C.addressof(C.c_char.in_dll(self.dll, "clo_ref_kernel_names"))).decode().split()

    @classmethod
    def get(cls, config):
        if config not in cls._cache:
            cls._cache[config] = cls(config)
        return cls._cache[config]

    def launch(self, kernel, args, gws, lws):
        """args: Buf (a __global or __local pointer) or a ctypes scalar, in the kernel's order."""
        body = C.cast(getattr(self.dll, "clo_ref_k_" + kernel), C.c_void_p)
        fibers = C.c_int.in_dll(self.dll, "clo_ref_k_%s_fibers" % kernel).value
        keep = [a.ptr if isinstance(a, Buf) else a for a in args]
        argv = (C.c_void_p * len(keep))(*[C.cast(C.pointer(k), C.c_void_p) for k in keep])
        rc = self.dll.clo_ref_launch(body, argv, gws, lws, fibers)
        LAUNCHES.append((self.config, kernel, int(gws), int(lws)))
        for i, a in enumerate(args):
            if isinstance(a, Buf):
                a.check("%s/%s argument %d, gws %d lws %d" % (self.config, kernel, i, gws, lws))
        if rc != 0:
            raise RuntimeError("%s/%s: launch failed (%d)" % (self.config, kernel, rc))


# ---------------------------------------------------------------------------------------------------------
# clo_common.c:141-199 and cf4ocl2's work-size rule
# ---------------------------------------------------------------------------------------------------------

def nlpo2(x):
    return 1 if x <= 1 else 1 << (int(x) - 1).bit_length()


def tzc(x):
    return (x & -x).bit_length() - 1


def is_pow2(x):
    return x >= 1 and (x & (x - 1)) == 0


def suggest_worksizes(real_ws, dev_max_lws, lws_max=0, with_gws=False):
    """(gws, lws): lws <= min(user max, device max), halved until <= real_ws; without a gws it must divide real_ws,
    with one real_ws is rounded up to a multiple of lws."""
    l = lws_max if (lws_max and lws_max < dev_max_lws) else dev_max_lws
    while l > 1 and l > real_ws:
        l >>= 1
    if not with_gws:
        while l > 1 and real_ws % l:
            l >>= 1
        return real_ws, l
    return -(-real_ws // l) * l, l


def _u32(v):
    return C.c_uint32(int(v))


# ---------------------------------------------------------------------------------------------------------
# scan/clo_scan_blelloch.c
# ---------------------------------------------------------------------------------------------------------

def scan_plan(numel, lws_max=0, dev_max_lws=256):
    """scan/clo_scan_blelloch.c:129-141: the work sizes and blocks_per_wg of the three launches."""
    realws = numel // 2                                               # :131
    if realws == 0:
        raise RefusedShape("upstream's scan launches numel / 2 = 0 work-items")
    gws1, lws = suggest_worksizes(realws, dev_max_lws, lws_max, with_gws=True)   # :132-133
    gws1 = min(gws1, lws * lws)                                       # :135
    ws2 = (gws1 // lws) // 2                                          # :136
    gws3 = -(-numel // lws) * lws                                     # :137 CLO_GWS_MULT
    bpw = -(-(numel // 2) // gws1)                                    # :140 CLO_DIV_CEIL
    return dict(lws=lws, gws1=gws1, ws2=ws2, gws3=gws3, bpw=bpw, three=gws1 > lws)


def scan(a, sum_dtype, lws_max=0, dev_max_lws=256, overrun_slack=False):
    """Exclusive scan of `a` by upstream's three kernels. data_out starts as zeros (the tail numel % (2*lws) is
    never written by the first kernel).

    Refused: a number of work-groups that is not a power of two when the second kernel runs (its tree scans
    2 * (groups / 2) sums and is only a scan for a power of two), and, unless `overrun_slack`, a numel that is no
    multiple of lws when the third kernel runs: addWorkgroupSums has no bound on gid and writes up to
    gws3 - numel sums past the end of data_out. With `overrun_slack` data_out is allocated gws3 elements long,
    as a device allocation with slack would be; only the first numel are returned."""
    a = np.ascontiguousarray(a)
    sum_dtype = np.dtype(sum_dtype)
    lib = Lib.get("scan_%s_%s" % (TYPE_NAMES[a.dtype], TYPE_NAMES[sum_dtype]))
    numel = a.size
    p = scan_plan(numel, lws_max, dev_max_lws)
    lws, groups = p["lws"], p["gws1"] // p["lws"]
    out_len = numel
    if p["three"]:
        if not is_pow2(groups):
            raise RefusedShape("workgroupSumsScan over %d sums" % groups)
        if p["gws3"] != numel:
            if not overrun_slack:
                raise RefusedShape("addWorkgroupSums writes %d elements past data_out" % (p["gws3"] - numel))
            out_len = p["gws3"]
    data_in, data_out = Buf(a), Buf(np.zeros(out_len, sum_dtype))
    wgsums = Buf(dtype=sum_dtype, count=groups, fill=0xEE)             # :144-145
    aux = local(sum_dtype.itemsize * lws * 2)                          # :150
    lib.launch("workgroupScan", [data_in, data_out, wgsums, aux, _u32(numel), _u32(p["bpw"])], p["gws1"], lws)   # :149-156
    if p["three"]:                                                     # :165
        aux2 = local(sum_dtype.itemsize * lws * 2)                     # :180
        lib.launch("workgroupSumsScan", [wgsums, aux2], p["ws2"], p["ws2"])              # :176-181
        lib.launch("addWorkgroupSums", [wgsums, data_out, _u32(p["bpw"])], p["gws3"], lws)   # :187-191
    return data_out.a[:numel].copy()


# ---------------------------------------------------------------------------------------------------------
# sorts: configuration names as oracle/ref_build.py spells them
# ---------------------------------------------------------------------------------------------------------

def sort_config(alg, a, key=None, descending=False):
    elem = TYPE_NAMES[np.dtype(a.dtype)]
    return "%s_%s%s_%s" % (alg, elem, "" if key in (None, elem) else "_k" + key, "desc" if descending else "asc")


def sbitonic(a, key=None, descending=False, lws_max=0, dev_max_lws=256):
    """sort/clo_sort_sbitonic.c:73-118."""
    a = np.ascontiguousarray(a)
    if not is_pow2(a.size) or a.size < 2:
        raise RefusedShape("the bitonic kernels have no bounds: numel must be a power of two")
    lib = Lib.get(sort_config("sbitonic", a, key, descending))
    gws, lws = suggest_worksizes(nlpo2(a.size) // 2, dev_max_lws, lws_max)       # :73-77
    tot_stages = tzc(gws * 2)                                          # :80
    data = Buf(a)
    for stage in range(1, tot_stages + 1):                             # :102
        for step in range(stage, 0, -1):                               # :108
            lib.launch("sbitonic", [data, _u32(stage), _u32(step)], gws, lws)   # :112
    return data.a.copy()


def gselect(a, key=None, descending=False, lws_max=0, dev_max_lws=256):
    """sort/clo_sort_gselect.c:75-113: one launch, out of place. gws = numel, so lws must divide it."""
    a = np.ascontiguousarray(a)
    if a.size < 1:
        raise RefusedShape("empty")
    lib = Lib.get(sort_config("gselect", a, key, descending))
    gws, lws = suggest_worksizes(a.size, dev_max_lws, lws_max)         # :75-78
    data_in, data_out = Buf(a), Buf(dtype=a.dtype, count=a.size, fill=0xEE)
    lib.launch("gselect", [data_in, data_out, C.c_uint64(a.size)], gws, lws)   # :105-111
    return data_out.a.copy()


# sort/clo_sort_abitonic.c:66-133: the kernels that can finish a stage from step 2..12, in preference order
_ABIT_LOOKUP = {
    2: ["abit_local_s2"], 3: ["abit_hyb_s3_3s8v", "abit_local_s3"],
    4: ["abit_hyb_s4_4s16v", "abit_hyb_s4_2s4v", "abit_local_s4"], 5: ["abit_local_s5"],
    6: ["abit_hyb_s6_3s8v", "abit_hyb_s6_2s4v", "abit_local_s6"], 7: ["abit_local_s7"],
    8: ["abit_hyb_s8_4s16v", "abit_hyb_s8_2s4v", "abit_local_s8"], 9: ["abit_hyb_s9_3s8v", "abit_local_s9"],
    10: ["abit_hyb_s10_2s4v", "abit_local_s10"], 11: ["abit_local_s11"],
    12: ["abit_hyb_s12_4s16v", "abit_hyb_s12_3s8v", "abit_hyb_s12_2s4v"],
}
_ABIT_PRIV = {4: "abit_priv_4s16v", 3: "abit_priv_3s8v", 2: "abit_priv_2s4v", 1: "abit_any"}


def abit_parse(name):
    """(family, K, S, V): sort/clo_sort_abitonic.in.h:112-113 (KPARSE_V after the last 's', KPARSE_S after the last '_')."""
    parts = name.split("_")
    if parts[1] == "any":
        return "any", 0, 1, 2
    if parts[1] == "local":
        return "local", int(parts[2][1:]), 1, 2
    s, v = parts[-1][:-1].split("s")
    if parts[1] == "priv":
        return "priv", 0, int(s), int(v)
    return "hyb", int(parts[2][1:]), int(s), int(v)


def abitonic_strategy(numel, lws_max=0, dev_max_lws=256, minps=1, maxps=4, maxsfs=0xFFFFFFFF):
    """sort/clo_sort_abitonic.c:58-313: per step 1..T a dict(kernel, gws, lws, set_step, num_steps, local_mem)."""
    n = nlpo2(numel)                                                   # :136
    tot = tzc(n)                                                       # :138
    _, lws_max_sfs = suggest_worksizes(1 << 20, dev_max_lws, lws_max)  # :148-151
    sfs = min(min(12, maxsfs), tzc(lws_max_sfs) + maxps)               # :155-157
    steps = []
    for step in range(1, tot + 1):                                     # :160
        any_gws, any_lws = suggest_worksizes(n // 2, dev_max_lws, lws_max)
        use_any = dict(kernel="abit_any", gws=any_gws, lws=any_lws, set_step=True, num_steps=1, local_mem=0)
        if step == 1:                                                  # :161-174
            steps.append(use_any)
        elif step > sfs:                                               # :175-227
            margin = min(step, maxps)                                  # :184
            gws = n // (1 << margin)                                   # :224
            steps.append(dict(kernel=_ABIT_PRIV[margin], gws=gws, lws=min(lws_max_sfs, gws), set_step=True,
                              num_steps=margin, local_mem=0))
        else:                                                          # :228-299
            for name in _ABIT_LOOKUP[step]:
                fam, _, s, v = abit_parse(name)
                priv_steps, local_mem = (s, v) if fam == "hyb" else (1, 2)       # :242-253
                gws, lws = suggest_worksizes(n // (1 << priv_steps), dev_max_lws, lws_max)   # :257-262
                if minps <= priv_steps <= maxps and lws >= (1 << (step - priv_steps)):      # :266-269
                    steps.append(dict(kernel=name, gws=gws, lws=lws, set_step=False, num_steps=step, local_mem=local_mem))
                    break
            else:
                steps.append(use_any)                                  # :283-298
    return steps


def abitonic(a, key=None, descending=False, lws_max=0, dev_max_lws=256, minps=1, maxps=4, maxsfs=0xFFFFFFFF):
    """sort/clo_sort_abitonic.c:377-432. Returns (sorted, [(kernel, stage, step)] in launch order)."""
    a = np.ascontiguousarray(a)
    if not is_pow2(a.size) or a.size < 2:
        raise RefusedShape("the bitonic kernels have no bounds: numel must be a power of two")
    lib = Lib.get(sort_config("abitonic", a, key, descending))
    tot = tzc(nlpo2(a.size))                                           # :378
    steps = abitonic_strategy(a.size, lws_max, dev_max_lws, minps, maxps, maxsfs)   # :381
    data = Buf(a)
    launches = []
    for stage in range(1, tot + 1):                                    # :401
        step = stage
        while step >= 1:                                               # :402
            s = steps[step - 1]                                        # :405
            abit_kernel(lib, s["kernel"], data, stage, step, s["gws"], s["lws"])    # :413-425
            launches.append((s["kernel"], stage, step))
            step -= s["num_steps"]                                     # :429
    return data.a.copy(), launches


def abit_kernel(lib, name, data, stage, step, gws, lws):
    """One abitonic launch: argument 2 is the step for the any / priv kernels (sort/clo_sort_abitonic.c:417-419)
    and lws * local_mem elements of __local memory for the local / hyb ones (:390-394)."""
    fam, K, _, v = abit_parse(name)
    n, es = data.a.size, data.a.dtype.itemsize
    if fam in ("any", "priv"):
        if gws * v != n or not (1 <= step <= stage) or (fam == "priv" and step < tzc(v)):
            raise RefusedShape("%s at step %d of stage %d over %d" % (name, step, stage, n))
        third = _u32(step)
    else:
        if gws * v != n or lws * v < (1 << K) or stage < K:
            raise RefusedShape("%s with lws %d at stage %d over %d" % (name, lws, stage, n))
        third = local(es * lws * v)
    lib.launch(name, [data, _u32(stage), third], gws, lws)


ABIT_KERNELS = ["abit_any"] + ["abit_local_s%d" % k for k in range(2, 12)] + sorted(set(_ABIT_PRIV.values()) - {"abit_any"}) + \
    [k for ks in _ABIT_LOOKUP.values() for k in ks if "hyb" in k]


# ---------------------------------------------------------------------------------------------------------
# sort/clo_sort_satradix.c
# ---------------------------------------------------------------------------------------------------------

def satradix(a, key=None, radix=16, lws_max=0, dev_max_lws=256, debug=False):
    """sort/clo_sort_satradix.c:166-313, in place (data_out NULL). The counters are scanned by the executed
    reference scan (uint -> uint). debug: also the three aux arrays of the first pass."""
    a = np.ascontiguousarray(a)
    if not is_pow2(radix) or radix < 2:
        raise RefusedShape("radix")                                    # :389-392
    if not is_pow2(a.size):
        raise RefusedShape("satradix_localsort has no bounds: numel must be a power of two")
    if a.size < radix:
        raise RefusedShape("numel < radix: the work-group would be larger than the array")
    es = a.dtype.itemsize
    ks = NP_TYPES[key]().itemsize if key else es
    bits = tzc(radix)                                                  # :167
    if ks < es and (8 * max(ks, 4)) % bits:
        # total_digits counts the element's bits (:168-169). Past the key's width OpenCL C takes the shift count modulo
        # the width of the (promoted) key, so a digit that straddles that width is sorted by one set of bits and
        # histogrammed by another: the scatter then leaves data_global.
        raise RefusedShape("a %d-bit digit straddles the width of a key narrower than its element" % bits)
    lib = Lib.get("satradix%d_%s%s" % (bits, TYPE_NAMES[a.dtype], "" if key in (None, TYPE_NAMES[a.dtype]) else "_k" + key))
    total_digits = es * 8 // bits                                      # :168-169
    numel_eff = nlpo2(a.size)                                          # :185
    _, lws_sort = suggest_worksizes(numel_eff, dev_max_lws, lws_max)   # :184-188
    lws_sort = max(lws_sort, radix)                                    # :190
    num_wgs = numel_eff // lws_sort + numel_eff % lws_sort             # :197
    naux = num_wgs * radix                                             # :235
    data = Buf(a)
    data_aux = Buf(dtype=a.dtype, count=numel_eff, fill=0xEE)          # :242
    offsets, counters, counters_sum = (Buf(dtype=np.uint32, count=naux, fill=0xEE) for _ in range(3))   # :247-257
    dbg = None
    for i in range(total_digits):                                      # :264
        start_bit = i * bits                                           # :266
        array_len = numel_eff // num_wgs                               # :267
        lib.launch("satradix_localsort", [data, data_aux, local(array_len * es), local(array_len * 4), _u32(start_bit)],
                   numel_eff, lws_sort)                                # :274-280
        lib.launch("satradix_histogram", [data_aux, offsets, counters, local(radix * 4), local(radix * 4),
                                          local(array_len * ks), _u32(start_bit), _u32(array_len)], numel_eff, lws_sort)   # :285-293
        counters_sum.a[:] = scan(counters.a, np.uint32, lws_max, dev_max_lws)     # :298-299
        if i == 0:
            dbg = (offsets.a.copy(), counters.a.copy(), counters_sum.a.copy())
        lib.launch("satradix_scatter", [data, data_aux, offsets, counters_sum, local(array_len * es), local(radix * 4),
                                        local(radix * 4), _u32(start_bit)], numel_eff, lws_sort)   # :303-310
    return (data.a.copy(),) + dbg if debug else data.a.copy()


# ---------------------------------------------------------------------------------------------------------
# rng/clo_rng.c and benchmarks/clo_rng_bench.c
# ---------------------------------------------------------------------------------------------------------

RNG_SEED_SIZE = {"lcg": 8, "xorshift64": 8, "xorshift128": 16, "mwc64x": 8, "parkmiller": 4, "tauslcg": 16}   # rng/clo_rng.c:60-68
RNG_HASH_CONFIG = {None: "nohash", "": "nohash", "KNUTH(x)": "knuth", "XS1(x)": "xs1"}


def rng_dev_gid_seeds(name, count, main_seed=0, hash=None):
    """rng/clo_rng.c:85-128: the DEV_GID path, clo_rng_init over `count` work-items. Returns the raw seed bytes."""
    lib = Lib.get("rng_%s_init_%s" % (name, RNG_HASH_CONFIG[hash]))
    seeds = Buf(dtype=np.uint8, count=count * RNG_SEED_SIZE[name], fill=0xEE)    # :112-113
    lib.launch("clo_rng_init", [C.c_uint64(int(main_seed) & (2 ** 64 - 1)), seeds], count, 1)   # :125-127
    return seeds.a.copy()


def rng_bench(name, seed_bytes, draws, bits=32, maxint=0, lws=64):
    """benchmarks/clo_rng_bench.c:297-311: `draws` launches of clo_rng_bench over one work-item per state; the
    kernel's third argument is maxint if set, else bits. Returns (draws x count outputs, final seed bytes)."""
    count = len(seed_bytes) // RNG_SEED_SIZE[name]
    if count % lws:
        lws = 1
    lib = Lib.get("rng_%s_%s" % (name, "maxint" if maxint else "bits"))
    seeds = Buf(np.ascontiguousarray(seed_bytes, dtype=np.uint8))
    result = Buf(dtype=np.uint32, count=count, fill=0xEE)
    out = np.empty((draws, count), np.uint32)
    value = _u32(maxint if maxint else bits)                           # :297
    for d in range(draws):
        lib.launch("clo_rng_bench", [seeds, result, value], count, lws)   # :305-306
        out[d] = result.a
    return out, seeds.a.copy()
