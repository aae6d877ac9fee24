"""numpy restatement of CloRng (test infrastructure): the six generators' seed conversion and step, the DEV_GID
hashes, the HOST_MT seed stream, and the fill's index rule. Every rule cites the upstream line it restates
(paths relative to the reference tree's src/cl_ops/). Vectorised over states; arithmetic wraps as the OpenCL
types do (numpy's fixed-width unsigned arrays)."""
import numpy as np

U32, U64 = np.uint32, np.uint64
NAMES = ["lcg", "xorshift64", "xorshift128", "mwc64x", "parkmiller", "tauslcg"]   # rng/clo_rng.c:60-68
SEED_SIZE = {"lcg": 8, "xorshift64": 8, "xorshift128": 16, "mwc64x": 8, "parkmiller": 4, "tauslcg": 16}
M32 = U64(0xFFFFFFFF)


def ulong2state(name, seed):
    """clo_ulong2statetype of an array of u64 seeds."""
    s = np.asarray(seed, dtype=U64)
    if name in ("lcg", "xorshift64"):       # rng/clo_rng_lcg.cl:32, clo_rng_xorshift64.cl:32: (seed)
        return s.copy()
    if name == "xorshift128":               # rng/clo_rng_xorshift128.cl:32: words from shifts 0, 16, 32, 46
        return np.stack([(s & M32), (s >> U64(16)) & M32, (s >> U64(32)) & M32, (s >> U64(46)) & M32], axis=-1).astype(U32)
    if name == "mwc64x":                    # rng/clo_rng_mwc64x.cl:33: as_uint2(seed) = (low, high)
        return np.stack([s & M32, s >> U64(32)], axis=-1).astype(U32)
    if name == "parkmiller":                # rng/clo_rng_parkmiller.cl:32: as_int((uint) (0xFFFFFFFF & seed))
        return (s & M32).astype(U32).view(np.int32)
    if name == "tauslcg":                   # rng/clo_rng_tauslcg.cl:32: as_uint4((ulong2) (seed, seed))
        lo, hi = s & M32, s >> U64(32)
        return np.stack([lo, hi, lo, hi], axis=-1).astype(U32)
    raise KeyError(name)


def _taus(z, s1, s2, s3, m):                # rng/clo_rng_tauslcg.cl:37-40
    b = ((z << U32(s1)) ^ z) >> U32(s2)
    return ((z & U32(m)) << U32(s3)) ^ b


def step(name, st):
    """One draw of every state: (new states, outputs as uint32)."""
    with np.errstate(over="ignore"):
        if name == "lcg":                   # rng/clo_rng_lcg.cl:44-53
            s = (st * U64(0x5DEECE66D) + U64(0xB)) & U64((1 << 48) - 1)
            return s, (s >> U64(16)).astype(U32)
        if name == "xorshift64":            # rng/clo_rng_xorshift64.cl:41-50
            s = st ^ (st << U64(21))
            s = s ^ (s >> U64(35))
            s = s ^ (s << U64(4))
            return s, (s & M32).astype(U32)
        if name == "xorshift128":           # rng/clo_rng_xorshift128.cl:41-51
            x, y, z, w = st[..., 0], st[..., 1], st[..., 2], st[..., 3]
            t = x ^ (x << U32(11))
            nw = w ^ (w >> U32(19)) ^ (t ^ (t >> U32(8)))
            return np.stack([y, z, w, nw], axis=-1), nw.copy()
        if name == "mwc64x":                # rng/clo_rng_mwc64x.cl:40-58
            A = U64(4294883355)
            x, c = st[..., 0].astype(U64), st[..., 1].astype(U64)
            res = (x ^ c).astype(U32)
            hi = (x * A) >> U64(32)
            nx = (x * A + c) & M32
            nc = (hi + (nx < c).astype(U64)) & M32
            return np.stack([nx, nc], axis=-1).astype(U32), res
        if name == "parkmiller":            # rng/clo_rng_parkmiller.cl:40-50: C's truncating remainder
            p = st.astype(np.int64) * 16807
            s = np.fmod(p, 2147483647).astype(np.int32)
            return s, s.view(U32) << U32(1)
        if name == "tauslcg":               # rng/clo_rng_tauslcg.cl:48-68
            x = st[..., 0]
            nx = _taus(st[..., 1], 13, 19, 12, 4294967294)
            ny = _taus(st[..., 2], 2, 25, 4, 4294967288)
            nz = _taus(st[..., 3], 3, 11, 17, 4294967294)
            nw = U32(1664525) * x + U32(1013904223)
            return np.stack([nx, ny, nz, nw], axis=-1), nx.copy()
    raise KeyError(name)


def knuth(x):                               # rng/clo_rng_init.cl:27: x = ((x*2654435761) % 0x100000000)
    with np.errstate(over="ignore"):
        return (np.asarray(x, dtype=U64) * U64(2654435761)) % U64(0x100000000)


def xs1(x):                                 # rng/clo_rng_init.cl:29-32
    x = np.asarray(x, dtype=U64)
    with np.errstate(over="ignore"):
        x = ((x >> U64(16)) ^ x) * U64(0x45d9f3b)
        x = ((x >> U64(16)) ^ x) * U64(0x45d9f3b)
        return (x >> U64(16)) ^ x


HASHES = {None: lambda x: x, "": lambda x: x, "KNUTH(x)": knuth, "XS1(x)": xs1,
          "(x * 3 + 1)": lambda x: x,                        # an expression statement: changes nothing
          "x = x << 2": lambda x: np.asarray(x, dtype=U64) << U64(2)}


def dev_gid_states(name, count, main_seed=0, hash=None):
    """rng/clo_rng_init.cl:45-57: seed = gid + main_seed; CLO_RNG_HASH(seed); seeds[gid] = clo_ulong2statetype(seed)."""
    with np.errstate(over="ignore"):
        seed = np.arange(count, dtype=U64) + U64(main_seed)
    return ulong2state(name, HASHES[hash](seed))


def host_mt_words(main_seed, nwords):
    """rng/clo_rng.c:158-186: g_rand_new_with_seed((guint32) main_seed), then g_rand_int per 4 bytes. GRand is
    MT19937 seeded by init_genrand, the core of numpy's legacy RandomState (tests/test_oracle.py)."""
    r = np.random.RandomState(int(main_seed) & 0xFFFFFFFF)
    return r.randint(0, 2 ** 32, size=nwords, dtype=np.uint64).astype(U32)


def state_from_bytes(name, raw, count):
    """States from their bytes in memory (EXT_HOST / HOST_MT seeds)."""
    raw = np.ascontiguousarray(raw).view(np.uint8)[:count * SEED_SIZE[name]]
    if name in ("lcg", "xorshift64"):
        return raw.view(U64).copy()
    if name == "parkmiller":
        return raw.view(np.int32).copy()
    return raw.view(U32).reshape(count, SEED_SIZE[name] // 4).copy()


def host_mt_states(name, count, main_seed):
    return state_from_bytes(name, host_mt_words(main_seed, count * SEED_SIZE[name] // 4), count)


def out_fn(x, bits=32, maxint=0):
    """benchmarks/clo_rng_bench.cl:37-41: clo_rng_next_int(seeds, maxint) = x % maxint, else x >> (32 - bits)."""
    return x % U32(maxint) if maxint else x >> U32(32 - bits)


def fill(name, states, numel, bits=32, maxint=0, keep=None):
    """clo_rng_fill: out[i] = f(draw i // S of state i % S), S = len(states); returns (out, final states). With
    `keep` (sorted indices), only out[keep] is returned (for fills too large to hold on the host)."""
    st = states.copy()
    S = st.shape[0]
    out = np.empty(numel if keep is None else len(keep), dtype=U32)
    d = 0
    while d * S < numel:
        m = min(S, numel - d * S)
        ns, x = step(name, st[:m])
        st[:m] = ns
        v = out_fn(x, bits, maxint)
        if keep is None:
            out[d * S:d * S + m] = v
        else:
            sel = (keep >= d * S) & (keep < d * S + m)
            out[sel] = v[keep[sel] - d * S]
        d += 1
    return out, st
