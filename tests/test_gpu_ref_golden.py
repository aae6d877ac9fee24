"""The HIP library against recorded outputs of upstream's own kernels (tests/golden/ref_exec_golden.npz, written by
tests/golden/make_ref_golden.py from the executed reference). Reads only the .npz: neither oracle/_ref nor the
reference tree exists on the GPU machine. Bit for bit through the C API, except where DESIGN §1 diverges on purpose;
each divergence is stated by the assertion that replaces the equality:

* +0 and -0 under the bitonic sorts: IEEE total order here, upstream's `>` leaves them where the network puts
  them. Compared as values, and bit for bit with the zeros' signs put in total order. (gselect compares them equal,
  as upstream: bit for bit.)
* satradix of signed keys: numeric order here; upstream orders raw bits (negatives after positives).
* satradix with a radix whose digit does not divide the key: every bit sorted here; upstream drops the partial
  last digit.
"""
import os

import numpy as np
import pytest

import rng_model as M

pytestmark = pytest.mark.gpu

G = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ref_exec_golden.npz"))
NAMES = {np.dtype(np.uint32): "uint", np.dtype(np.uint64): "ulong", np.dtype(np.int32): "int", np.dtype(np.int64): "long",
         np.dtype(np.uint16): "ushort", np.dtype(np.uint8): "uchar", np.dtype(np.float32): "float", np.dtype(np.float64): "double",
         np.dtype(np.int16): "short"}
DESC = "((a) < (b))"
PAIR = {"uint": dict(key_type="uint", get_key="(uint) ((x) >> 32)"),
        "float": dict(key_type="float", get_key="as_float((uint) ((x) >> 32))")}


def bits_of(a):
    return np.ascontiguousarray(a).view("u%d" % a.dtype.itemsize)


def zeros_in_total_order(sorted_vals, descending):
    """A sorted float array with the signs of its run of zeros rearranged as the IEEE total order wants them."""
    out = sorted_vals.copy()
    z = np.flatnonzero(out == 0)
    if z.size:
        assert np.array_equal(z, np.arange(z[0], z[0] + z.size))
        neg = int(np.signbit(out[z]).sum())
        signs = np.zeros(z.size, out.dtype)
        signs[(z.size - neg if descending else 0):(z.size if descending else neg)] = -0.0
        out[z] = signs
    return out


def test_recorded_upstream_outputs_through_the_hip_path(gpu):
    import cl_ops_amd as clo
    ctx, q = gpu
    bad = []                      # every mismatch is collected, so one run shows them all; any of them fails the test

    def check(ok, what):
        if not ok:
            bad.append(what)
        return 1

    checked = 0

    def sort(alg, a, **kw):
        s = clo.Sorter(alg, ctx, NAMES[a.dtype], **kw)
        try:
            return s.with_host_data(a, q)
        finally:
            s.close()

    # whole keys, both directions
    for t in ("uint", "ulong", "int", "long", "ushort", "uchar", "float", "double"):
        a = G["keys_%s_in" % t]
        for tag, kw in (("asc", {}), ("desc", dict(compare=DESC))):
            exp = G["keys_%s_%s" % (t, tag)]
            for alg in ("sbitonic", "abitonic", "gselect"):
                got = sort(alg, a, **kw)
                if alg == "gselect":          # the kernel compares -0 == +0 as upstream's does: equal keys stay in input order
                    rec = G["keys_%s_gselect_%s" % (t, tag)] if "keys_%s_gselect_%s" % (t, tag) in G.files else exp
                    check(np.array_equal(bits_of(got), bits_of(rec)), (t, tag, alg))
                elif a.dtype.kind == "f":
                    check(np.array_equal(got, exp), (t, tag, alg))                  # as values
                    check(np.array_equal(bits_of(got), bits_of(zeros_in_total_order(exp, tag == "desc"))), (t, tag, alg))
                else:
                    check(np.array_equal(got, exp), (t, tag, alg))
                checked += 1

    # tie order of the bitonic network, stable order of gselect and satradix, on (key, index) pairs
    for key in ("uint", "float"):
        p = G["tie_%s_in" % key]
        for tag, kw in (("asc", {}), ("desc", dict(compare=DESC))):
            for alg in ("sbitonic", "abitonic"):
                got = sort(alg, p, **PAIR[key], **kw)
                exp = G["tie_%s_bitonic_%s" % (key, tag)]
                if key == "float":
                    # the keys +0 and -0 tie upstream and are ordered here: everything but the zero-key pairs, in place
                    nz = (exp >> np.uint64(32)) & np.uint64(0x7FFFFFFF) != 0
                    check(np.array_equal((got >> np.uint64(32)) & np.uint64(0x7FFFFFFF) != 0, nz), (key, tag, alg))
                    check(np.array_equal(got[nz], exp[nz]) and np.array_equal(np.sort(got[~nz]), np.sort(exp[~nz])), (key, tag, alg))
                else:
                    check(np.array_equal(got, exp), (key, tag, alg))
                checked += 1
            exp = G["tie_%s_gselect_%s" % (key, tag)]
            got = sort("gselect", p[:exp.size], **PAIR[key], **kw)
            check(np.array_equal(got, exp), (key, tag))          # zero keys of either sign tie here as upstream, by index
            checked += 1
    check(np.array_equal(sort("satradix", G["tie_uint_in"], **PAIR["uint"]), G["tie_uint_satradix"]), "satradix pairs")
    checked += 1

    # satradix: every radix; where upstream drops the partial last digit, its output sorted on by the dropped bits
    a = G["radix_uint_in"]
    for radix in (2, 4, 8, 16, 32, 64, 128, 256):
        bits = radix.bit_length() - 1
        rec = G["radix_uint_r%d" % radix]
        done = (32 // bits) * bits
        assert np.array_equal(rec, a[np.argsort(a & np.uint32((1 << done) - 1), kind="stable")])
        got = sort("satradix", a, options="radix=%d" % radix)
        check(np.array_equal(got, rec[np.argsort(rec >> np.uint32(done), kind="stable")] if done < 32 else rec), radix)
        checked += 1
    for t in ("int", "long", "ulong", "ushort", "uchar"):
        a, rec = G["radix_%s_in" % t], G["radix_%s_r16" % t]
        got = sort("satradix", a)
        if a.dtype.kind == "i":
            assert np.all(rec[:int((rec >= 0).sum())] >= 0) and (rec < 0).any()             # upstream: negatives last
            rec = np.concatenate((rec[rec < 0], rec[rec >= 0]))
        check(np.array_equal(got, rec), t)
        checked += 1
    check(np.array_equal(sort("satradix", G["aux_in"]), G["aux_out"]), "satradix aux_in")
    checked += 1

    # scans: integer pairs (negative elements into a wider sum among them) and float -> integer casts
    for name in G.files:
        if name.startswith("scan_") and name.endswith("_in"):
            a, exp = G[name], G[name[:-3] + "_out"]
            sc = clo.Scanner("blelloch", ctx, NAMES[a.dtype], NAMES[exp.dtype])
            got = sc.with_host_data(a, q)
            sc.close()
            check(got.dtype == exp.dtype and np.array_equal(got, exp), name)
            checked += 1

    # RNG: seeds of the DEV_GID path per hash, 64 states x 64 draws, final states; the maxint form
    S, D = 64, 64
    for tag in ("nohash", "knuth", "xs1", "ext"):
        h, ms, bits = str(G["rng_%s_hash" % tag]) or None, int(G["rng_%s_main_seed" % tag]), int(G["rng_%s_bits" % tag])
        off = 0
        for gi, name in enumerate(M.NAMES):
            nb = S * M.SEED_SIZE[name]
            seeds, fin = G["rng_%s_seeds" % tag][off:off + nb], G["rng_%s_final" % tag][off:off + nb]
            off += nb
            if tag == "ext":
                r = clo.Rng(name, ctx, q, "ext_host", seeds.view(np.uint32).copy(), S)
            else:
                r = clo.Rng(name, ctx, q, "dev_gid", None, S, ms, h)
            check(np.array_equal(r.states(q), M.state_from_bytes(name, seeds, S)), (name, tag, "seeds"))
            out = clo.Buffer(ctx, 4 * S * D)
            r.fill(q, out, S * D, bits)
            check(np.array_equal(out.read(q, np.uint32, S * D), G["rng_%s_out" % tag][gi].reshape(-1).astype(np.uint32)), (name, tag))
            check(np.array_equal(r.states(q), M.state_from_bytes(name, fin, S)), (name, tag, "final"))
            r.close()
            checked += 1
            if tag == "knuth":
                for mi, maxint in enumerate(G["rng_maxints"]):
                    r = clo.Rng(name, ctx, q, "dev_gid", None, S, ms, h)
                    r.fill(q, out, S * 4, 32, int(maxint))
                    check(np.array_equal(out.read(q, np.uint32, S * 4), G["rng_maxint_out"][gi, mi].reshape(-1).astype(np.uint32)), (name, maxint))
                    r.close()
                    checked += 1
            out.close()
    # 48 sorts of whole keys, 13 on pairs, 14 radix sorts, 13 scans, 24 + 18 RNG fills: an empty or cut fixture fails here
    assert not bad, bad
    assert checked >= 130, checked
