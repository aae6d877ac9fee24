"""The host schedules of the bitonic sorts, restated in plain Python: which kernels sort an array, in which order, and
with how many steps each. Three things decide it — log2 of the padded size, the element size and the key mode — and
all three are decided on the host:

  * tiled_run (clo_hip_bitonic_impl.h): Q, KLF, QS, plain_cost, s2_cost, strided_cost, use_m2 under
    CLO_BITONIC_MERGE2 = 0 / 1 / 2, the short plain pass first, the branches T < Q and T < KLF;
  * the tiled branch of clo_hip_bitonic_jit_sort (clo_hip_bitonic_jit.hip): KL_MAX, NS2, `h > Q && h <= NS2`;
  * tiled_impl's choice of mode from (key_shift, key_bits, key_size, key_kind);
  * clo_sort_new's routing (clo_sort_abstract.c): which compare / get_key strings the parser turns into a shift and a
    mask (ahead-of-time kernels) and which go to hiprtc.

A launch is (family, stage, first step, steps). Families of the ahead-of-time schedule, with the label their launches
are timed under: step (bitonic_step), tile_rt and presort (bitonic_presort), strided (bitonic_strided), strided2
(bitonic_strided2), merge and merge2 (bitonic_tile). Families of the run-time compiled one: jit_step, jit_tile,
jit_strided, jit_strided2l, jit_merge.

tests/test_gpu_bitonic_schedule.py holds the device to this model launch by launch;
tests/test_bitonic_reach_cpu.py walks its case table through the model."""
import re
from collections import namedtuple

Launch = namedtuple("Launch", "family stage first steps")

TBF = 9                      # thread bits of the compile-time-schedule kernels
JIT_TB = 8                   # thread bits of the run-time compiled tile kernels
MERGE2_EXTRA = 20            # CLO_MERGE2_EXTRA: us a two-tile merge costs over a merge pass
LABELS = ("bitonic_step", "bitonic_presort", "bitonic_strided", "bitonic_strided2", "bitonic_tile")
LABEL_OF = {"step": "bitonic_step", "tile_rt": "bitonic_presort", "presort": "bitonic_presort", "strided": "bitonic_strided",
            "strided2": "bitonic_strided2", "merge": "bitonic_tile", "merge2": "bitonic_tile"}

# CloType numbering (include/clo_common.h): name -> (number, bytes, key kind: 0 unsigned, 1 signed, 2 IEEE)
TYPES = {"char": (0, 1, 1), "uchar": (1, 1, 0), "short": (2, 2, 1), "ushort": (3, 2, 0), "int": (4, 4, 1), "uint": (5, 4, 0),
         "long": (6, 8, 1), "ulong": (7, 8, 0), "half": (8, 2, 2), "float": (9, 4, 2), "double": (10, 8, 2)}


def nlpo2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def log2u(x):
    l = 0
    while (1 << l) < x:
        l += 1
    return l


def q_of(es):
    """Register bits per thread: 32 values of at most 4 bytes, 16 values of 8 bytes."""
    return 4 if es == 8 else 5


def klf_of(es):
    return TBF + q_of(es)


def qs_of(es, mode):
    """Register bits of a plain strided pass: 64 values for whole-element keys, 2^(Q + 1) for the general compare."""
    return q_of(es) + 1 if mode == 0 else 6


def mode_of(es, key_shift, key_bits, key_size, key_kind):
    """tiled_impl: 1 / 2 / 3 for whole-element unsigned / signed / IEEE keys, 0 for everything else."""
    identity = key_shift == 0 and key_bits == 8 * es and key_size == es
    if identity and key_kind == 0:
        return 1
    if identity and key_kind == 1:
        return 2
    if es >= 2 and identity and key_kind == 2:
        return 3
    return 0


# ---- the cost table of tiled_run -------------------------------------------------------------------------------------

def plain_cost(k, qs):
    c = 0
    while k > 0:
        t = (k % qs if k % qs else qs) if k > qs else k
        c += 81 if t >= 6 else 72 + t
        k -= t
    return c


S2_SIDES = ("line", "half", "less")        # rows of at least a cache line, of half a line, shorter


def s2_side(b2, es):
    row = (1 << (klf_of(es) - b2)) * es
    return "line" if row >= 128 else ("half" if row >= 64 else "less")


def s2_cost(b2, es, side=None):
    """`side`: cost the pass as that side of the row-size branches would (the reach test asks whose side decides)."""
    side = side or s2_side(b2, es)
    return 75 + 2 * (b2 - q_of(es)) if side == "line" else (124 if side == "half" else 250)


def best_cut(h, es, mode, recost=None):
    """(cost, b2): the cheapest cut of h strided steps into plain passes first and at most ONE two-level pass of
    b2 = Q + 2 .. 2Q steps right above the tile (0: none). recost = (side, as_side): passes on `side` of s2_cost's
    branches are costed as `as_side` would cost them."""
    q, qs = q_of(es), qs_of(es, mode)
    best, best_b = plain_cost(h, qs), 0
    for b2 in range(q + 2, min(2 * q, h) + 1):
        side = s2_side(b2, es)
        if recost and recost[0] == side:
            side = recost[1]
        c = plain_cost(h - b2, qs) + s2_cost(b2, es, side)
        if c < best:
            best, best_b = c, b2
    return best, best_b


def strided_cost(h, es, mode):
    return best_cut(h, es, mode)[0]


def strided_passes(stage, p, stop, es, mode, recost=None):
    """The launches for steps p .. stop + 1 of `stage`, as the while loop of tiled_run cuts them."""
    qs = qs_of(es, mode)
    out = []
    while p > stop:
        h = p - stop
        best_b = best_cut(h, es, mode, recost)[1]
        if best_b == h:
            out.append(Launch("strided2", stage, p, best_b))
            p -= best_b
            continue
        ns = h - best_b
        if ns > qs:
            ns = ns % qs if ns % qs else qs        # several plain passes: the short one first
        out.append(Launch("strided", stage, p, ns))
        p -= ns
    return out


M2_TERMS = ("whole_keys", "switched_on", "enough_tiles", "four_bytes", "saves_a_pass")


def m2_terms(es, mode, T, stage, merge2):
    """The conjunction behind use_m2 as named terms (kl == KLF holds at every stage above the tile). With
    CLO_BITONIC_MERGE2=2 the last two are replaced by the switch itself."""
    klf = klf_of(es)
    tiles = 1 << (T - klf)
    h = stage - klf
    terms = {"whole_keys": mode != 0, "switched_on": merge2 != 0, "enough_tiles": tiles >= (2 if merge2 == 2 else 64)}
    if merge2 != 2:
        terms["four_bytes"] = es == 4
        terms["saves_a_pass"] = strided_cost(h, es, mode) > strided_cost(h - 1, es, mode) + MERGE2_EXTRA
    return terms


def m2_decider(es, mode, T, stage, merge2):
    """(use_m2, what decided it): taken — "forced" (CLO_BITONIC_MERGE2=2) or "saves_a_pass"; not taken — the one term
    that alone keeps it from being taken, or None when more than one does (flipping any single term changes nothing)."""
    terms = m2_terms(es, mode, T, stage, merge2)
    false = [k for k in M2_TERMS if k in terms and not terms[k]]
    if not false:
        return True, "forced" if merge2 == 2 else "saves_a_pass"
    return False, ("not:" + false[0]) if len(false) == 1 else None


def aot_schedule(es, mode, numel, merge2=1, recost=None):
    """tiled_run<E, MODE> for `numel` elements of `es` bytes: the ordered list of launches."""
    q, klf = q_of(es), klf_of(es)
    T = log2u(nlpo2(numel))
    if numel <= 1:
        return []
    if T < q:
        return [Launch("step", stage, step, 1) for stage in range(1, T + 1) for step in range(stage, 0, -1)]
    kl = min(T, klf)
    out = [Launch("presort" if kl == klf else "tile_rt", kl, kl, kl * (kl + 1) // 2)]
    for stage in range(kl + 1, T + 1):
        use_m2 = m2_decider(es, mode, T, stage, merge2)[0]
        stop = kl + 1 if use_m2 else kl
        out += strided_passes(stage, stage, stop, es, mode, recost)
        out.append(Launch("merge2", stage, kl + 1, kl + 1) if use_m2 else Launch("merge", stage, kl, kl))
    return out


def jit_schedule(es, numel, tiled=1):
    """clo_hip_bitonic_jit_sort for a power of two; any other numel runs the flip network, one launch per step."""
    if numel <= 1:
        return []
    T = log2u(numel)
    q = q_of(es)
    kl_max = JIT_TB + q
    if numel & (numel - 1):
        return [Launch("jit_step_any", stage, step, 1) for stage in range(1, T + 1) for step in range(stage, 0, -1)]
    if not tiled or T < q:
        return [Launch("jit_step", stage, step, 1) for stage in range(1, T + 1) for step in range(stage, 0, -1)]
    kl = min(T, kl_max)
    out = [Launch("jit_tile", kl, kl, kl * (kl + 1) // 2)]
    ns2 = min(JIT_TB, 2 * q)
    for stage in range(kl + 1, T + 1):
        p = stage
        while p > kl:
            h = p - kl
            if q < h <= ns2 and kl == kl_max:
                out.append(Launch("jit_strided2l", stage, p, h))
                p -= h
                continue
            ns = min(h - ns2 if h > ns2 else h, q)
            out.append(Launch("jit_strided", stage, p, ns))
            p -= ns
        out.append(Launch("jit_merge", stage, kl, kl))
    return out


def label_counts(launches):
    out = {l: 0 for l in LABELS}
    for l in launches:
        if l.family in LABEL_OF:
            out[LABEL_OF[l.family]] += 1
    return out


def last_stage(launches):
    """The launches of the last stage of a sort (for a sort inside one tile: its one launch)."""
    if not launches:
        return []
    top = max(l.stage for l in launches)
    return [l for l in launches if l.stage == top]


# ---- clo_sort_new: which strings the parser of the fixed family reads -------------------------------------------------

_CASTS = {"unsigned long": 8, "unsigned int": 4, "unsigned short": 2, "unsigned char": 1, "uchar": 1, "char": 1, "ushort": 2,
          "short": 2, "uint": 4, "int": 4, "ulong": 8, "long": 8}
_AS_TYPES = dict(_CASTS, half=2, float=4, double=8)


def parse_compare(text):
    """0 / 1: ascending / descending; None: the parser refuses (hiprtc builds it)."""
    if text is None:
        return 0
    t = re.sub(r"[\s()]", "", text)
    return {"a>b": 0, "a<b": 1}.get(t)


class _Cursor:
    def __init__(self, text):
        self.t, self.i = text, 0

    def ws(self):
        while self.i < len(self.t) and self.t[self.i].isspace():
            self.i += 1

    def accept(self, s):
        self.ws()
        if self.t.startswith(s, self.i):
            self.i += len(s)
            return True
        return False

    def number(self):
        self.ws()
        m = re.match(r"0[xX][0-9a-fA-F]+|\d+", self.t[self.i:])
        if not m:
            return None
        self.i += m.end()
        while self.i < len(self.t) and self.t[self.i] in "uUlL":
            self.i += 1
        s = m.group(0)
        return int(s, 16) if s[:2].lower() == "0x" else (int(s, 8) if len(s) > 1 and s[0] == "0" else int(s))


def _primary(c):
    save = c.i
    if c.accept("("):                                  # a cast: '(' type ')'
        c.ws()
        m = re.match(r"(?:unsigned )?[a-z]+(?![A-Za-z0-9_])", c.t[c.i:])
        if m and m.group(0) in _CASTS:
            j = c.i
            c.i += m.end()
            if c.accept(")"):
                f = _primary(c)
                size = _CASTS[m.group(0)]
                return f and (f[0], f[1] & ((1 << (8 * size)) - 1) if size < 8 else f[1])
            c.i = j
        c.i = save
    m = re.match(r"\s*as_([a-z]+)\s*(?=\()", c.t[c.i:])
    if m and m.group(1) in _AS_TYPES and " " not in m.group(1):
        c.i += m.end()
        f = _primary(c)
        size = _AS_TYPES[m.group(1)]
        return f and (f[0], f[1] & ((1 << (8 * size)) - 1) if size < 8 else f[1])
    if c.accept("("):
        f = _and(c)
        return f if f and c.accept(")") else None
    c.ws()
    if c.t[c.i:c.i + 1] == "x" and not re.match(r"[A-Za-z0-9_]", c.t[c.i + 1:c.i + 2] or " "):
        c.i += 1
        return (0, (1 << 64) - 1)
    return None


def _shift(c):
    f = _primary(c)
    while f and c.accept(">>"):
        n = c.number()
        if n is None or n > 63:
            return None
        f = (f[0] + n, f[1] >> n)
    return f


def _and(c):
    f = _shift(c)
    while f and c.accept("&"):
        n = c.number()
        if n is None:
            return None
        f = (f[0], f[1] & n)
    return f


def parse_get_key(text, es, key_size):
    """(key_shift, key_bits), or None when the parser refuses: the grammar is casts, as_type(), parentheses, `>>` and
    `&` with numbers over the one name x, and only a contiguous low mask is built."""
    f = (0, (1 << 64) - 1)
    if text is not None:
        c = _Cursor(text)
        f = _and(c)
        c.ws()
        if f is None or c.i != len(text):
            return None
    shift, mask = f
    if es < 8:
        mask &= 0 if shift >= 8 * es else ((1 << (8 * es)) - 1) >> shift
    elif shift > 0:
        mask &= ((1 << 64) - 1) >> shift
    if key_size < 8:
        mask &= (1 << (8 * key_size)) - 1
    if mask == 0 or mask & (mask + 1):
        return None
    return shift, bin(mask).count("1")


def route(elem_type, key_type=None, compare=None, get_key=None):
    """("aot", es, (key_shift, key_bits, key_size, key_kind, descending)) or ("jit", es, None): what clo_sort_new makes of
    the arguments of Sorter("sbitonic" | "abitonic", ...) (no compiler options)."""
    _, es, _ = TYPES[elem_type]
    _, ks, kind = TYPES[key_type or elem_type]
    field = parse_get_key(get_key, es, ks)
    desc = parse_compare(compare)
    if field is None or desc is None or (kind == 2 and field[1] != 8 * ks):
        return "jit", es, None
    return "aot", es, (field[0], field[1], ks, kind, desc)


def sorter_schedule(elem_type, numel, key_type=None, compare=None, get_key=None, merge2=1):
    """The launches of Sorter("sbitonic" | "abitonic", ...) on `numel` elements: both run the tiled schedule. A numel
    that is no power of two is padded for whole-element keys; a partial or compiled key runs the flip network, one
    launch per step (None here: the model holds no such schedule)."""
    how, es, spec = route(elem_type, key_type, compare, get_key)
    if how == "jit":
        return how, (jit_schedule(es, numel) if numel & (numel - 1) == 0 else None)
    shift, bits, ks, kind, _ = spec
    if numel & (numel - 1) and (shift != 0 or bits != 8 * es):
        return how, None
    return how, aot_schedule(es, mode_of(es, shift, bits, ks, kind), numel, merge2)
