"""What CloSegScan's kernels (cl_ops_amd/csrc/hip/clo_hip_segscan.hip) do one level below the tile,
computed with numpy from segscan_model.merge_steps alone: nothing here calls the library. The rules are the kernel's,
restated:
  the tile        clo_seg_tile_range: tile t holds the merge steps [d0, d1) = [min(t T, m + n), min(t T + T, m + n)), cnt of
                  them; na of them close the ends [a0, a0 + na), nb = cnt - na take the rows [b0, b0 + nb), b0 = d0 - a0.
                  There are ceil((numel_seg + n) / T) tiles, whatever num_in leaves of the segments. SWEEP stores the
                  tile's rows below ct = min(total, n): nstore = max(min(b0 + nb, ct), b0) - b0.
  TAILS           the rows behind the tile's last close: [c, b0 + nb), c = that end clipped at n and clamped into
                  [b0, b0 + nb] (c = b0 where nothing closes), count = b0 + nb - c. They are read as head single elements
                  up to the first 16-byte boundary of values + c (at most count), nvec 16-byte vectors of PER elements,
                  and the elements behind the body; rest = head + those.
  SWEEP, a lane   lane l of 256 owns the steps [d, d + steps) of the tile, d = min(17 l, cnt), steps = min(17, cnt - d).
                  With e_k the position of the tile's end k among the tile's rows (clamped into [0, nb]), `a` = the ends
                  with e_k + k < d (the halving), b = d - a, ne = min(the next lane's a - a, steps), nr = steps - ne; end
                  a + j closes at step min(max(e_(a+j) - b, 0), nr) + j of the lane: bit that of the `closes` mask.
  SWEEP, a wave   64 lanes, 64 * 17 steps; its state's head count is the number of its closes.
  CARRY           thread i of 256 holds the states of the tiles [16 i, 16 i + 16) of a trip of 4096; it loads them with
                  16-byte loads where 16 i + 16 <= tiles and one by one otherwise.
The lane items and carry items are the kernel's CLO_SEG_ITEMS and CLO_SEG_CARRY_ITEMS; T comes from the library's getter and is
passed in."""
import numpy as np

from segscan_model import merge_steps

ITEMS = 17         # CLO_SEG_ITEMS: merge steps per lane
CARRY_ITEMS = 16   # CLO_SEG_CARRY_ITEMS: tile states per thread of the carry scan
WAVE = 64


class Lanes:
    """The fields are numpy arrays: one entry per tile (cnt, a0, na, nb, b0, nstore, c, count, head, nvec, rest,
    residue), one per lane of every tile (steps, ne, nr, closes), one per wave of every tile (wave_closes); for the carry
    scan tiles, vector (per thread that holds a tile: is it on the 16-byte path) and last_thread."""


def lanes(form, counts_or_offsets, n, T, num_in=None, value_size=4, align=0, items=ITEMS, carry_items=CARRY_ITEMS):
    """align: the byte address of values_in modulo 16."""
    assert T % items == 0 and value_size in (4, 8) and align % value_size == 0
    threads = T // items
    src = np.asarray(counts_or_offsets)
    m_h = src.size - (1 if form == "offsets" else 0)
    close, m, total = merge_steps(form, src, n, num_in)
    ends = close - np.arange(m, dtype=np.int64)                                # the clipped ends
    L = Lanes()
    L.T, L.threads, L.m, L.n, L.total = T, threads, m, n, total
    L.tiles = tiles = -(-(m_h + n) // T) if m_h else 0
    steps_all = m + n
    ct = min(total, n)
    t = np.arange(tiles, dtype=np.int64)
    d0, d1 = np.minimum(t * T, steps_all), np.minimum(t * T + T, steps_all)
    L.cnt = d1 - d0
    L.a0 = np.searchsorted(close, d0, "left")                                  # the closes among the first d0 steps
    L.na = np.searchsorted(close, d1, "left") - L.a0
    L.nb = L.cnt - L.na
    L.b0 = d0 - L.a0
    L.nstore = np.maximum(np.minimum(L.b0 + L.nb, ct), L.b0) - L.b0
    # TAILS
    last = ends[np.maximum(L.a0 + L.na - 1, 0)] if m else np.zeros(tiles, np.int64)
    L.c = np.where(L.na > 0, np.minimum(np.maximum(last, L.b0), L.b0 + L.nb), L.b0)
    L.count = L.b0 + L.nb - L.c
    per = 16 // value_size
    L.per = per
    L.residue = (align + L.c * value_size) % 16
    L.head = np.minimum(((16 - L.residue) % 16) // value_size, L.count)
    L.nvec = (L.count - L.head) // per
    L.rest = L.head + (L.count - L.head - L.nvec * per)
    # SWEEP
    L.steps = np.zeros((tiles, threads), np.int64)
    L.ne = np.zeros((tiles, threads), np.int64)
    L.nr = np.zeros((tiles, threads), np.int64)
    L.closes = np.zeros((tiles, threads), np.int64)
    lane = np.arange(threads + 1, dtype=np.int64)
    for k in range(tiles):
        cnt, na, nb, a0, b0 = (int(x[k]) for x in (L.cnt, L.na, L.nb, L.a0, L.b0))
        e = np.clip(ends[a0:a0 + na] - b0, 0, nb)                              # s_end
        d = np.minimum(lane * items, cnt)
        a = np.searchsorted(e + np.arange(na), d, "left")                      # the halving: ends with e_k <= d - 1 - k
        a[threads] = na                                                        # s_start[CLO_SEG_THREADS]
        a, d, nxt = a[:threads], d[:threads], a[1:]
        b = d - a
        steps = np.minimum(items, cnt - d)
        ne = np.minimum(np.maximum(nxt, a) - a, steps)
        nr = steps - ne
        L.steps[k], L.ne[k], L.nr[k] = steps, ne, nr
        own = np.repeat(lane[:threads], ne)                                    # the lane of every end it closes
        j = np.arange(own.size) - np.repeat(np.cumsum(ne) - ne, ne)
        if own.size:
            p = np.minimum(np.maximum(e[a[own] + j] - b[own], 0), nr[own]) + j
            np.bitwise_or.at(L.closes[k], own, np.int64(1) << p)
    L.wave_closes = L.ne.reshape(tiles, threads // WAVE, WAVE).sum(axis=2)
    # CARRY (the first trip: tiles <= 256 * 16 in everything aimed at threads)
    holders = -(-tiles // carry_items)
    L.vector = (np.arange(holders) + 1) * carry_items <= tiles
    L.last_thread = holders - 1
    return L


def close_steps(L):
    """The merge steps at which the lanes' masks say a segment closes, ascending: what merge_steps gives directly."""
    out = []
    for k in range(L.tiles):
        bits = (L.closes[k][:, None] >> np.arange(ITEMS)) & 1
        lane, bit = np.nonzero(bits)
        out.append(k * L.T + lane * ITEMS + bit)
    return np.concatenate(out) if out else np.zeros(0, np.int64)
