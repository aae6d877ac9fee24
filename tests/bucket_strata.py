"""The strata of tests/test_gpu_bucket_fuzz.py: a seeded, stratified set of CloBucket calls. Every value of every
dimension is dealt — key type, value form, count type, bin count (on both sides of the one-pass / two-pass border at 256
digits, the rest being one), row count (empty, and on both sides of multiples of the tile), lower, shift and the rows'
distribution — by walking the dimensions with strides that are coprime to their lengths, so that no two dimensions move
together. tests/test_bucket_cpu.py shows, through the model alone, that the strata reach what they are for."""
import numpy as np

SEED = 24101
NP = {"char": np.int8, "uchar": np.uint8, "short": np.int16, "ushort": np.uint16, "int": np.int32, "uint": np.uint32,
      "long": np.int64, "ulong": np.uint64}
KEY_TYPES = tuple(NP)
MODES = ("keys", "v4", "v8", "arg", "arg_only")
VALUE_SIZE = {"keys": 0, "v4": 4, "v8": 8, "arg": 4, "arg_only": 4}
COUNT_TYPES = ("uint", "ulong")
BIN_COUNTS = (1, 2, 16, 254, 255, 256, 257, 1000, 4096, 65535)          # 255 bins + the rest: the last one-pass call
SIZES = ("0", "1", "T-1", "T", "T+1", "2T-1", "2T", "3T+1", "random")
DISTS = ("uniform", "one bin", "rest only", "descending", "two bins", "skewed")
LOWERS = ("zero", "positive", "negative or min", "near max")
SHIFTS = ("0", "small", "B-1")
STRATA = 240


def size_of(name, T, rng):
    return {"0": 0, "1": 1, "T-1": T - 1, "T": T, "T+1": T + 1, "2T-1": 2 * T - 1, "2T": 2 * T, "3T+1": 3 * T + 1}.get(name) if name != "random" \
        else int(rng.integers(2, 4 * T))


def strata(T):
    """The list of strata for tiles of T rows: dicts with key_type, mode, count_type, num_bins, n, lower, shift, dist and
    keys (raw keys of the type; their bins are whatever the mapping gives them)."""
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(STRATA):
        kt = KEY_TYPES[i % 8]
        mode = MODES[(i // 8 + i) % 5]
        ct = COUNT_TYPES[(i // 3) % 2]
        num_bins = BIN_COUNTS[(7 * i + i // 10) % 10]
        size = SIZES[(4 * i + i // 9) % 9]
        dist = DISTS[(5 * i + i // 6) % 6]
        lower_kind = LOWERS[(3 * i + i // 4) % 4]
        shift_kind = SHIFTS[(2 * i + i // 3) % 3]
        info = np.iinfo(NP[kt])
        B = 8 * np.dtype(NP[kt]).itemsize
        n = size_of(size, T, rng)
        shift = {"0": 0, "small": int(rng.integers(1, 4)), "B-1": B - 1}[shift_kind]
        width = min(num_bins << shift, 1 << B)                          # the range's width, cut to the type's
        lower = {"zero": 0, "positive": int(rng.integers(1, 100)), "negative or min": int(-rng.integers(1, 100)) if info.min < 0 else 0,
                 "near max": info.max - min(width // 2, info.max)}[lower_kind]
        # offsets d from lower, by distribution; then raw keys lower + d, cut to the type's range
        bins_reached = max(1, min(num_bins, (info.max - lower) >> shift))
        if dist == "uniform":
            b = rng.integers(-2, bins_reached + 2, n)
        elif dist == "one bin":
            b = np.full(n, bins_reached // 2)
        elif dist == "rest only":
            b = np.where(rng.random(n) < 0.5, -1 - rng.integers(0, 5, n), num_bins + rng.integers(0, 5, n))
        elif dist == "descending":
            b = (n - 1 - np.arange(n)) * bins_reached // max(n, 1)
        elif dist == "two bins":
            b = np.where(np.arange(n) % 2 == 0, bins_reached - 1, 0)
        else:
            b = np.where(rng.random(n) < 0.9, bins_reached // 3, rng.integers(-2, bins_reached + 2, n))
        low = rng.integers(0, 1 << min(shift, 30), n) if shift else np.zeros(n, np.int64)
        d = np.asarray(b).astype(object) * (1 << shift) + low.astype(object) + lower          # Python integers: nothing wraps
        keys = np.maximum(np.minimum(d, info.max), info.min).astype(NP[kt]) if n else np.zeros(0, NP[kt])
        out.append(dict(key_type=kt, mode=mode, count_type=ct, num_bins=num_bins, size=size, n=n, lower=lower, lower_kind=lower_kind, shift=shift,
                        shift_kind=shift_kind, dist=dist, keys=keys))
    return out
