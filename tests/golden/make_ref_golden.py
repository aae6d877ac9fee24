"""Generates tests/golden/ref_exec_golden.npz: inputs and outputs OF UPSTREAM'S OWN KERNELS, executed on the CPU
(oracle/ref_build.py, tests/ref_exec.py), for a subset of tests/test_ref_pin.py small enough to commit. The file
holds arrays and short names only. tests/test_gpu_ref_golden.py holds the HIP library against it on the GPU, where
neither oracle/_ref nor the reference tree exists; tests/test_oracle.py holds the restatements against it anywhere.

Refuses to write if, on any of these inputs, the executed kernels disagree with the restatement that
tests/test_ref_pin.py compares them with (the oracle, the RNG model, the numpy cast), or if the file would outgrow
tests/golden/sortscan_golden.npz.

Run from the repository root, after build():  python tests/golden/make_ref_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import oracle_lib as O  # noqa: E402
import ref_exec as R  # noqa: E402
import rng_model as M  # noqa: E402
from numpy_ops import scan_cast_expected  # noqa: E402
from test_ref_pin import KIND, PAIR_KW, bits_of, keys_of, pairs_of, same_bits, state_bytes  # noqa: E402

U32, U64 = np.uint32, np.uint64
LIMIT = os.path.getsize(os.path.join(HERE, "sortscan_golden.npz"))       # the largest fixture tracked so far

# the seeding paths that end in a kernel: (tag, hash, main seed, bits recorded); "ext" = arbitrary state bytes
RNG_PATHS = [("nohash", "", 12345, 32), ("knuth", "KNUTH(x)", (1 << 64) - 1, 8), ("xs1", "XS1(x)", 0, 8), ("ext", "", 0, 8)]


def need(ok, what):
    if not ok:
        raise SystemExit("refusing to write: executed upstream and its restatement disagree on " + str(what))


def main():
    out = {}

    # --- comparison sorts of whole keys, both directions (N <= 4096). Sorted whole keys are one function of the input
    # up to where +0 / -0 land, so one output serves sbitonic, abitonic and (N <= 1024) gselect.
    for t, n in (("uint", 512), ("ulong", 256), ("int", 512), ("long", 256), ("ushort", 512), ("uchar", 512),
                 ("float", 512), ("double", 256)):
        a = keys_of(t, n, 1000 + n)
        out["keys_%s_in" % t] = a
        for desc, tag in ((False, "asc"), (True, "desc")):
            kw = dict(key_kind=KIND[t], descending=desc)
            got = R.sbitonic(a, descending=desc)
            need(same_bits(got, O.sbitonic(a, **kw)) and same_bits(R.abitonic(a, descending=desc)[0], O.abitonic(a, **kw)[0]), ("bitonic", t, tag))
            need(same_bits(got, R.abitonic(a, descending=desc)[0]), ("sbitonic vs abitonic", t, tag))
            if n <= 1024:
                g = R.gselect(a, descending=desc)
                need(same_bits(g, O.gselect(a, **kw)) and np.array_equal(g, got), ("gselect", t, tag))
                if not same_bits(g, got):
                    out["keys_%s_gselect_%s" % (t, tag)] = g          # differs from the network in where +0 / -0 land only
            out["keys_%s_%s" % (t, tag)] = got

    # --- tie order: (key, index) pairs, at most 50 distinct keys, key in the high word
    for key, n in (("uint", 512), ("float", 512)):
        p = pairs_of(n, 77, key)
        out["tie_%s_in" % key] = p
        for desc, tag in ((False, "asc"), (True, "desc")):
            kw = dict(PAIR_KW[key], descending=desc)
            got = R.sbitonic(p, key, desc)
            need(np.array_equal(got, O.sbitonic(p, **kw)) and np.array_equal(R.abitonic(p, key, desc)[0], got)
                 and np.array_equal(O.abitonic(p, **kw)[0], got), ("tie order", key, tag))
            out["tie_%s_bitonic_%s" % (key, tag)] = got
            g = R.gselect(p[:300], key, desc)
            need(np.array_equal(g, O.gselect(p[:300], **kw)), ("gselect pairs", key, tag))
            out["tie_%s_gselect_%s" % (key, tag)] = g                 # of the first 300 pairs: any numel
    p = out["tie_uint_in"]
    got = R.satradix(p, "uint", dev_max_lws=64)
    need(np.array_equal(got, O.satradix(p, dev_max_lws=64, key_size=4, key_shift=32)), "satradix pairs")
    out["tie_uint_satradix"] = got

    # --- satradix per radix (8 / 32 / 64 / 128 drop the partial last digit), other key types, one pass's aux arrays
    a = keys_of("uint", 256, 5)
    out["radix_uint_in"] = a
    for radix in (2, 4, 8, 16, 32, 64, 128, 256):
        got = R.satradix(a, radix=radix, dev_max_lws=64)
        need(np.array_equal(got, O.satradix(a, radix=radix, dev_max_lws=64)), ("satradix", radix))
        out["radix_uint_r%d" % radix] = got
    for t in ("int", "long", "ulong", "ushort", "uchar"):
        a = keys_of(t, 128, 6)
        got = R.satradix(a, dev_max_lws=64)
        need(same_bits(got, O.satradix(a, dev_max_lws=64, key_kind=KIND[t])), ("satradix", t))
        out["radix_%s_in" % t], out["radix_%s_r16" % t] = a, got
    a = keys_of("uint", 512, 8)
    got = R.satradix(a, radix=16, lws_max=64, dev_max_lws=64, debug=True)
    exp = O.satradix(a, radix=16, lws_max=64, dev_max_lws=64, debug=True)
    need(all(np.array_equal(g, e) for g, e in zip(got, exp)), "aux arrays")
    out["aux_in"] = a
    for g, what in zip(got, ("out", "offsets", "counters", "counters_sum")):
        out["aux_" + what] = g

    # --- scans: integer pairs (int -> long holds negative elements), float -> integer casts
    for et, st, n in (("uint", "uint", 512), ("uint", "ulong", 512), ("int", "long", 512), ("uchar", "uint", 512),
                      ("ushort", "ushort", 512), ("ulong", "ulong", 256), ("long", "short", 256), ("uint", "uchar", 512)):
        a = keys_of(et, n, 9)
        got = R.scan(a, R.NP_TYPES[st], 0, 64)
        need(same_bits(got, O.blelloch(a, R.NP_TYPES[st], 0, 64)) and same_bits(got, scan_cast_expected(a, R.NP_TYPES[st])), ("scan", et, st))
        out["scan_%s_%s_in" % (et, st)], out["scan_%s_%s_out" % (et, st)] = a, got
    for et, st in (("float", "uint"), ("double", "long"), ("float", "int"), ("double", "uchar"), ("float", "ulong")):
        edt, sdt = np.dtype(R.NP_TYPES[et]), np.dtype(R.NP_TYPES[st])
        si = np.iinfo(sdt)
        hi = min(300.0, float(si.max))
        lo = -min(300.0, float(-si.min)) if si.min < 0 else -0.999
        a = (np.random.default_rng(10).random(256) * (hi - lo) * 0.999 + lo).astype(edt)
        a[:8] = np.array([0.5, -0.5, 0.999, -0.999, 1.5, 2.999, -0.0, 0.0], edt)
        if si.min < 0:
            a[8:12] = np.array([-1.5, -2.999, -1.0, -127.5], edt)
        got = R.scan(a, sdt, 0, 64)
        need(same_bits(got, scan_cast_expected(a, sdt)), ("scan cast", et, st))
        out["scan_%s_%s_in" % (et, st)], out["scan_%s_%s_out" % (et, st)] = a, got

    # --- RNG: 64 states x 64 draws of every generator for each seeding path that ends in a kernel
    S, D = 64, 64
    for tag, h, ms, bits in RNG_PATHS:
        out["rng_%s_hash" % tag] = np.array(h)
        out["rng_%s_main_seed" % tag] = np.array(ms, U64)
        out["rng_%s_bits" % tag] = np.array(bits, U32)
    # (per path one array each: the generators' seed bytes, final state bytes (both concatenated in M.NAMES order) and
    # outputs [generator, draw, state], to spare the archive's per-array overhead)
    for tag, h, ms, bits in RNG_PATHS:
        all_seeds, all_out, all_fin = [], [], []
        for name in M.NAMES:
            if tag == "ext":
                seeds = np.random.default_rng(len(name)).integers(0, 256, S * M.SEED_SIZE[name], dtype=np.uint8)
                seeds[:M.SEED_SIZE[name]] = 0
                seeds[M.SEED_SIZE[name]:2 * M.SEED_SIZE[name]] = 0xFF
            else:
                seeds = R.rng_dev_gid_seeds(name, S, ms, h)
                need(np.array_equal(seeds, state_bytes(M.dev_gid_states(name, S, ms, h))), ("rng seeds", name, tag))
            got, fin = R.rng_bench(name, seeds, D, bits=bits)
            exp, efin = M.fill(name, M.state_from_bytes(name, seeds, S), S * D, bits)
            need(np.array_equal(got.reshape(-1), exp) and np.array_equal(fin, state_bytes(efin)), ("rng stream", name, tag))
            all_seeds.append(seeds), all_out.append(got.astype(np.uint8) if bits <= 8 else got), all_fin.append(fin)
        out["rng_%s_seeds" % tag] = np.concatenate(all_seeds)
        out["rng_%s_out" % tag] = np.stack(all_out)
        out["rng_%s_final" % tag] = np.concatenate(all_fin)
    # the maxint form (a power of two, another number, 1) from the knuth path's seeds, 64 states x 4 draws:
    # [generator, maxint, draw, state]
    out["rng_maxints"] = np.array([256, 251, 1], U32)
    off, rows = 0, []
    for name in M.NAMES:
        seeds = out["rng_knuth_seeds"][off:off + S * M.SEED_SIZE[name]]
        off += S * M.SEED_SIZE[name]
        row = []
        for maxint in out["rng_maxints"]:
            got, _ = R.rng_bench(name, seeds, 4, maxint=int(maxint))
            need(np.array_equal(got.reshape(-1), M.fill(name, M.state_from_bytes(name, seeds, S), S * 4, 32, int(maxint))[0]), ("rng maxint", name))
            row.append(got.astype(np.uint8))
        rows.append(np.stack(row))
    out["rng_maxint_out"] = np.stack(rows)

    path = os.path.join(HERE, "ref_exec_golden.npz")
    tmp = path + ".tmp.npz"
    np.savez_compressed(tmp, **out)
    size = os.path.getsize(tmp)
    if size > LIMIT:
        os.remove(tmp)
        raise SystemExit("refusing to write: %d bytes, more than sortscan_golden.npz's %d" % (size, LIMIT))
    os.replace(tmp, path)
    print("wrote", path, size, "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
