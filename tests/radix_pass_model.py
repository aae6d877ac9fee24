"""A numpy model of one sort through the chain-free pair passes (clo_radix4_pair_kernel), and the key families
aimed at its scatter. It touches no GPU and reads no source file: the rules below restate DESIGN.md section 4.1 and
the comments of clo_hip_radix4.hip and clo_hip_radix_rank.h.

Which path takes a sort (clo_radix4_sort):
- at most 16 384 elements (8 192 of 8 bytes) with a digit of at most 4 bits: one launch;
- digits of 4 or 8 bits, 4- or 8-byte elements, fewer than 2^31 of them: the single-sweep passes when CLO_RADIX_SWEEP=1
  and there is more than one 512-thread tile, never when it is 0, and by the library's own choice from 2 to 256
  tiles;
- otherwise the pair passes: tiles of 512 threads x 16 items (8 items for 8-byte elements), or of 1024 threads from
  256 MiB of 4-byte elements and 32 MiB of 8-byte ones (elements of 1 and 2 bytes never).

A pass: digit_bits b <= 4 pairs two digits (LB = HB = b), a wider digit is one pass split 3+2, 3+3, 4+3, 4+4. Pass p
takes the key bits from key_shift + p (LB + HB) on; the last pass's digits are cut to the bits left, low digit first.
A pass that is not the last writes the next pass's digit byte per element on big tiles with LB = HB = 4; for elements
under 8 bytes four of them go out as one dword, gathered by byte permutes when next_shift is a multiple of 8 and by
shifts and masks otherwise.

A tile: `single` when one combined digit holds all of it (no split), else split stably by the combined digit. The
scatter hands VEC consecutive positions of the split tile to a thread (VEC = 4 under 8 bytes, else 1): on a full tile
they go out as one vector store when the first and the last digit agree (and the vector ends inside the array),
otherwise element by element; a partial tile goes element by element."""
import numpy as np

PAIRS = {1: (1, 1), 2: (2, 2), 3: (3, 3), 4: (4, 4), 5: (3, 2), 6: (3, 3), 7: (4, 3), 8: (4, 4)}
FAMILIES = ("one_digit_per_tile", "single_mixed", "short_runs", "two_runs", "sorted", "reversed", "skew90")
_U = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def items_of(elem_size):
    return 8 if elem_size == 8 else 16


def big_tile_bytes(elem_size):
    return (32 if elem_size == 8 else 256) << 20


def big_tiles(n, elem_size):
    return elem_size >= 4 and n * elem_size >= big_tile_bytes(elem_size)


def sweep_applies(n, elem_size, digit_bits, sweep):
    """sweep: None (the library's choice), 0 or 1 — CLO_RADIX_SWEEP."""
    if sweep == 0:
        return False
    if digit_bits not in (4, 8) or elem_size not in (4, 8) or n >= 1 << 31:
        return False
    tile = 512 * items_of(elem_size)
    tiles = (n + tile - 1) // tile
    if sweep == 1:
        return tiles > 1
    return 2 <= tiles <= 256


def path(n, elem_size, digit_bits, sweep=None):
    """'one_launch', 'sweep', 'pair512' or 'pair1024'."""
    if n <= 1024 * items_of(elem_size) and digit_bits <= 4:
        return "one_launch"
    if sweep_applies(n, elem_size, digit_bits, sweep):
        return "sweep"
    return "pair1024" if big_tiles(n, elem_size) else "pair512"


def shape(n, elem_size):
    """(threads, items, tile, VEC) of the pair passes for n elements."""
    threads = 1024 if big_tiles(n, elem_size) else 512
    items = items_of(elem_size)
    return threads, items, threads * items, (1 if elem_size >= 8 else 4)


def schedule(n, elem_size, key_shift, key_bits, digit_bits):
    """The passes of the sort: dicts with LB, HB, shift, mask_lo, mask_hi, mask, next_shift, last, dig (the pass
    writes a digit stream) and gather ('perm', 'shifts', or None where no dword of digits is gathered)."""
    LB, HB = PAIRS[digit_bits]
    PB = LB + HB
    passes = (key_bits + PB - 1) // PB
    big = big_tiles(n, elem_size)
    out = []
    for p in range(passes):
        rem = key_bits - p * PB
        bits = min(rem, PB)
        lo = min(bits, LB)
        hi = bits - lo
        d = dict(p=p, LB=LB, HB=HB, shift=key_shift + p * PB, mask_lo=(1 << lo) - 1, mask_hi=(1 << hi) - 1, lo_bits=lo, hi_bits=hi,
                 next_shift=key_shift + (p + 1) * PB, last=p + 1 == passes)
        d["mask"] = (d["mask_hi"] << LB) | d["mask_lo"]
        d["dig"] = big and LB == 4 and HB == 4 and not d["last"]
        d["gather"] = None
        if d["dig"] and elem_size < 8:
            d["gather"] = "perm" if d["next_shift"] % 8 == 0 and d["next_shift"] < 8 * elem_size else "shifts"
        out.append(d)
    return out


def field_mask(key_bits):
    return (1 << key_bits) - 1


def forward(a, key_shift, key_bits, kind):
    """The transform of the first read: 0 none, 1 two's complement (the sign bit flips), 2 IEEE (a set sign bit flips
    the whole field, a clear one is set)."""
    a = np.ascontiguousarray(a)
    ut = a.dtype.type
    if kind == 0:
        return a.copy()
    sign = ut(1 << (key_shift + key_bits - 1))
    if kind == 1:
        return a ^ sign
    field = ut(field_mask(key_bits) << key_shift)
    return a ^ np.where((a & sign) != 0, field, sign)


def inverse(a, key_shift, key_bits, kind):
    a = np.ascontiguousarray(a)
    ut = a.dtype.type
    if kind == 0:
        return a.copy()
    sign = ut(1 << (key_shift + key_bits - 1))
    if kind == 1:
        return a ^ sign
    field = ut(field_mask(key_bits) << key_shift)
    return a ^ np.where((a & sign) != 0, sign, field)


def pass_digit(a, d):
    """The combined digit hi:lo of every element in pass d, as the narrowest unsigned type (numpy's stable sorts of
    8- and 16-bit integers are radix sorts)."""
    x = (a >> a.dtype.type(d["shift"])) & a.dtype.type(d["mask"])
    return x.astype(np.uint8 if d["LB"] + d["HB"] <= 8 else np.uint16)


def _rows(dig, tile):
    """(full tiles as rows, the partial last tile or None)."""
    nfull = dig.size // tile
    full = dig[:nfull * tile].reshape(nfull, tile)
    part = dig[nfull * tile:]
    return full, (part if part.size else None)


def analyse_pass(dig, n, d, threads, items, vec):
    """What the tiles of one launch look like, from the combined digit of every element in input order."""
    tile = threads * items
    R2 = 1 << (d["LB"] + d["HB"])
    ntiles = (n + tile - 1) // tile
    full, part = _rows(dig, tile)
    hist = np.zeros((ntiles, R2), np.int64)
    CH = 128                                                # (tiles at a time: the temporaries stay in the cache)
    for c0 in range(0, full.shape[0], CH):
        rows = full[c0:c0 + CH]
        idx = (np.arange(rows.shape[0], dtype=np.int32)[:, None] * R2 + rows).ravel()
        hist[c0:c0 + rows.shape[0]] = np.bincount(idx, minlength=rows.shape[0] * R2).reshape(rows.shape[0], R2)
    if part is not None:
        hist[ntiles - 1] = np.bincount(part, minlength=R2)
    counts = np.minimum(tile, n - np.arange(ntiles, dtype=np.int64) * tile)
    single = (hist.max(axis=1) == counts)
    is_full = counts == tile
    # the scanned counters: global start of (tile, digit) in digit-major order, and the tile-local start of a digit
    per_digit = hist.sum(axis=0)
    dbase = np.cumsum(per_digit) - per_digit
    toff = dbase[None, :] + np.cumsum(hist, axis=0) - hist
    lstart = np.cumsum(hist, axis=1) - hist
    delta = toff - lstart                                   # global index = tile-local position + delta[tile, digit]
    r = dict(tiles=ntiles, single_full=int((single & is_full).sum()), single_partial=int((single & ~is_full).sum()),
             split_full=int((~single & is_full).sum()), split_partial=int((~single & ~is_full).sum()),
             run_lengths=set(np.unique(hist[hist > 0]).tolist()), whole_tile_run=bool((hist == tile).any()),
             all_digits=bool(((hist > 0).sum(axis=1) == R2).any()), vector_residues=set(), cuts=set(), partial_groups=0,
             guard_fails=0, item_edge=False)
    if vec == 1 and full.shape[0]:
        r["vector_residues"] = {0}
    for c0 in range(0, full.shape[0], CH):
        srt = np.sort(full[c0:c0 + CH], axis=1, kind="stable")
        if vec > 1:
            g = srt.reshape(srt.shape[0], tile // vec, vec)
            same = g[:, :, 0] == g[:, :, vec - 1]
            t_idx, g_idx = np.nonzero(same)
            gi0 = g_idx.astype(np.int64) * vec + delta[c0 + t_idx, g[t_idx, g_idx, 0].astype(np.int64)]
            r["vector_residues"] |= set(np.unique(gi0 % vec).tolist())
            r["guard_fails"] += int((gi0 > n - vec).sum())
            for k in range(1, vec):                         # the run changes between elements k - 1 and k of a vector
                if k not in r["cuts"] and (g[:, :, k] != g[:, :, k - 1]).any():
                    r["cuts"].add(k)
        # a run that ends on the last of a thread's `items` consecutive positions (and not at the tile's end)
        if not r["item_edge"]:
            r["item_edge"] = bool((srt[:, items - 1:tile - 1:items] != srt[:, items::items]).any())
    if part is not None:
        r["partial_groups"] = (part.size + vec - 1) // vec
    return r, hist, delta


def simulate(keys, elem_size, key_shift, key_bits, key_kind, digit_bits, only=None):
    """The passes of the sort of `keys` (raw element bits, an unsigned array): a list of (pass dict, record) and the
    sorted array with the inverse transform applied. only: the passes to analyse tile by tile (all are run; the others
    record only whether the launch moves anything and whether it sees one digit)."""
    a = np.ascontiguousarray(keys)
    assert a.dtype == _U[elem_size]
    n = a.size
    threads, items, tile, vec = shape(n, elem_size)
    cur = forward(a, key_shift, key_bits, key_kind)
    out = []
    for d in schedule(n, elem_size, key_shift, key_bits, digit_bits):
        dig = pass_digit(cur, d)
        if only is None or d["p"] in only:
            rec, _, _ = analyse_pass(dig, n, d, threads, items, vec)
            rec["analysed"] = True
        else:
            rec = dict(analysed=False)
        rec["constant"] = bool(dig.min() == dig.max())           # one digit in the whole launch: every tile `single`
        identity = rec["constant"]
        if not identity:
            order = np.argsort(dig, kind="stable")
            identity = bool((order[1:] > order[:-1]).all())
        rec["identity"] = identity
        if not identity:
            cur = cur[order]
        out.append((d, rec))
    return out, inverse(cur, key_shift, key_bits, key_kind)


# ----------------------------------------------------------------------------------------------------------------------
# key families
# ----------------------------------------------------------------------------------------------------------------------

def two_runs_lengths(items, tile):
    return [1, 2, 3, 4, 5, 63, 64, 65, items - 1, items, items + 1, tile - 1]


def _tile_digits(family, t, count, R, items, tile, rng):
    """The digit at pass p* of the `count` elements of tile t, in input order."""
    if family == "one_digit_per_tile":
        return np.full(count, (7 * t) % R, np.int64)
    if family == "single_mixed":
        if t % 2 == 0 or count < tile:
            return np.full(count, (7 * t) % R, np.int64)
        return rng.integers(0, R, count)
    if family == "short_runs":
        # every digit r times, r = 1 .. 5 by digit and tile; one digit takes what is left; in a scrambled order
        filler = t % R
        reps = 1 + (np.arange(R) + t) % 5
        reps[filler] = 0
        d = np.repeat(np.arange(R), reps)
        if d.size >= count:
            d = d[:count]
        else:
            d = np.concatenate((d, np.full(count - d.size, filler, np.int64)))
        return rng.permutation(d)
    if family == "two_runs":
        a = (3 * t) % R
        b = (a + 1 + t % (R - 1)) % R
        cs = two_runs_lengths(items, tile)
        c = min(cs[t % len(cs)], count)
        d = np.full(count, b, np.int64)
        at = (t * (5 * items + 1)) % (count - c + 1)
        d[at:at + c] = a
        return d
    raise ValueError(family)


def make_keys(family, n, elem_size, key_shift, key_bits, digit_bits, pstar, seed, key_kind=0, tile=None, items=None, upper="random"):
    """Deterministic keys (raw element bits) of one family. The first four families write the digit of pass `pstar`
    tile by tile (tile, items: the tile of the launch, by default that of n elements of this size), leave the key bits
    below it zero and fill those above it (upper 'random': at random; 'grouped': the next pass's digit is one value
    per even digit of pass p* and for its highest digit, random for the others). sorted / reversed / skew90 speak of
    the whole key field. What is written is the key AFTER the forward transform; the element holds its inverse. The
    bits outside the field carry the element's index, low bits first."""
    ut = _U[elem_size]
    if tile is None:
        _, items, tile, _ = shape(n, elem_size)
    rng = np.random.default_rng(seed)
    idx = np.arange(n, dtype=np.uint64)
    fm = field_mask(key_bits)
    if family in ("sorted", "reversed"):
        if key_bits <= 32:
            T = (idx << np.uint64(key_bits)) // np.uint64(n)
        else:
            T = idx * np.uint64(fm // max(n - 1, 1))
        if family == "reversed":
            T = np.uint64(fm) - T
    elif family == "skew90":
        T = rng.integers(0, fm, n, dtype=np.uint64, endpoint=True)
        T[rng.random(n) < 0.9] = np.uint64(0x5A5A5A5A5A5A5A5A & fm)
    else:
        d = schedule(n, elem_size, key_shift, key_bits, digit_bits)[pstar]
        R = d["mask"] + 1
        assert R >= 2
        dig = np.concatenate([_tile_digits(family, t, min(tile, n - t * tile), R, items, tile, rng) for t in range((n + tile - 1) // tile)])
        below = d["shift"] - key_shift
        T = dig.astype(np.uint64) << np.uint64(below)
        above = d["next_shift"] - key_shift
        if above < key_bits:
            up = rng.integers(0, fm >> above, n, dtype=np.uint64, endpoint=True)
            if upper == "grouped":
                nd = np.uint64(min((1 << (d["LB"] + d["HB"])), (fm >> above) + 1))
                grouped = (dig % 2 == 0) | (dig == R - 1)
                up = np.where(grouped, ((up // nd) * nd) | ((dig.astype(np.uint64) * np.uint64(37) + np.uint64(11)) % nd), up)
            T |= up << np.uint64(above)
    a = (T & np.uint64(fm)) << np.uint64(key_shift)
    a = inverse(a, key_shift, key_bits, key_kind) if key_kind else a
    low = key_shift
    high = 8 * elem_size - key_shift - key_bits
    if low:
        a |= idx & np.uint64((1 << low) - 1)
    if high:
        a |= ((idx >> np.uint64(low)) & np.uint64((1 << high) - 1)) << np.uint64(key_shift + key_bits)
    return a.astype(ut)


def order_key(a, key_shift, key_bits, key_kind):
    """The key field as unsigned integers whose order is the sort's: the field itself, sign-flipped for two's
    complement keys, the IEEE total order for floating-point ones."""
    a = np.ascontiguousarray(a).astype(np.uint64)
    f = (a >> np.uint64(key_shift)) & np.uint64(field_mask(key_bits))
    sign = np.uint64(1 << (key_bits - 1))
    if key_kind == 1:
        return f ^ sign
    if key_kind == 2:
        return np.where((f & sign) != 0, ~f & np.uint64(field_mask(key_bits)), f ^ sign)
    return f


def stable_order(a, key_shift, key_bits, key_kind):
    k = order_key(a, key_shift, key_bits, key_kind)
    for ut in (np.uint8, np.uint16, np.uint32):
        if key_bits <= 8 * np.dtype(ut).itemsize:
            k = k.astype(ut)
            break
    return np.argsort(k, kind="stable")
