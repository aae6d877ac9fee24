"""Measurement probe (not part of the bench contract): CloBucket against what a caller has today, on the same GPU in one
process.

Baselines, on code the bucket partition does not touch:
  (a) this library's sort of the same rows — clo_sort_* for keys alone, clo_sort_by_key_* with values and for the
      argsort — plus Histogram plus the blelloch scan for the offsets;
  (b) torch.sort(bins, stable=True) (+ a gather of the values) + torch.bincount + cumsum.
The keys ARE their bins (lower 0, shift 0, every key below num_bins), so that a sort by key is the same permutation.
Legs: 2^28 and 2^24 uint32 keys x 16, 255, 256, 4096 and 65 535 bins, uniform, keys only; the key patterns (all equal,
8 distinct, 90 % in one bin) at 255 and 4096 bins; the forms (uint32 values, arg, uint64 keys) at 255 and 4096 bins; and
one pipeline leg, bucket -> SegReduce("offsets") against sort by key -> reduce by key.
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for --reps rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the bytes its schedule
moves (per pass: the keys read twice, the keys and values read by the scatter written once; two passes above 255 bins,
plus one more read of the keys for the histogram), those bytes per second as a fraction of the 8 TB/s peak, and its time
over each baseline's; LOSES where it is slower than a baseline. Then one pass with the library's per-kernel events:
where the time goes. Every output is compared with torch's before anything is timed.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/bucket_probe.py [--log2n 28,24] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
BINS = (16, 255, 256, 4096, 65535)
LABELS = ("bucket_count", "bucket_scan", "bucket_scatter", "bucket_offsets", "histogram")


def stats(ms):
    t = sorted(ms)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}


def schedule_bytes(n, ks, valued, arg, passes):
    """What the launches move: per pass the keys read by the count and by the scatter, the values or the first pass's
    indices read by the scatter, the rows written (the last pass of the arg form writes no keys); with two passes the
    histogram's read of the keys. The counters (12 bytes per tile and digit) are left out."""
    total = 0
    for p in range(passes):
        last = p == passes - 1
        reads_values = 4 if valued or (arg and p > 0) else 0
        writes = (0 if arg and last else ks) + (4 if valued or arg else 0)
        total += n * (2 * ks + reads_values + writes)
    return total + (n * ks if passes == 2 else 0)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", default="28,24")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "bucket_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": clo.bucket_tile(4, 0), "legs": []}

    legs = []   # (n, bins, pattern, form)
    for lg in [int(x) for x in args.log2n.split(",")]:
        n = 1 << lg
        legs += [(n, b, "uniform", "keys") for b in BINS]
        legs += [(n, b, p, "keys") for b in (255, 4096) for p in ("all equal", "8 distinct", "90 % in one bin")]
        legs += [(n, b, "uniform", f) for b in (255, 4096) for f in ("values", "arg", "ulong keys", "pipeline")]

    def keys_of(n, bins, pattern, dtype, g):
        if pattern == "uniform":
            return torch.randint(0, bins, (n,), device="cuda", dtype=dtype, generator=g)
        if pattern == "all equal":
            return torch.full((n,), bins // 2, device="cuda", dtype=dtype)
        if pattern == "8 distinct":
            return torch.randint(0, 8, (n,), device="cuda", dtype=dtype, generator=g) * (bins // 8)
        k = torch.randint(0, bins, (n,), device="cuda", dtype=dtype, generator=g)
        return torch.where(torch.rand(n, device="cuda", generator=g) < 0.9, torch.full_like(k, bins // 3), k)

    for n, bins, pattern, form in legs:
        torch.cuda.empty_cache()
        g = torch.Generator(device="cuda").manual_seed(n % 1000 + bins)
        kt, ks, dtype = ("ulong", 8, torch.int64) if form == "ulong keys" else ("uint", 4, torch.int32)
        keys = keys_of(n, bins, pattern, dtype, g)
        valued, arg = form in ("values", "pipeline"), form == "arg"
        vs = 4 if valued or arg else 0
        values = torch.randint(0, 1 << 20, (n,), device="cuda", dtype=torch.int32, generator=g) if valued else None
        ko, vo = torch.empty_like(keys), torch.empty(n, device="cuda", dtype=torch.int32)
        ko2, vo2 = torch.empty_like(keys), torch.empty(n, device="cuda", dtype=torch.int32)
        off, off2 = torch.zeros(bins + 1, device="cuda", dtype=torch.int32), torch.zeros(bins + 1, device="cuda", dtype=torch.int32)
        hist = torch.zeros(bins + 1, device="cuda", dtype=torch.int32)
        sums = torch.zeros(bins, device="cuda", dtype=torch.int64)
        rows2 = n if form == "pipeline" else 2                            # reduce by key sizes its outputs by numel rows
        sums2, rk = torch.zeros(rows2, device="cuda", dtype=torch.int64), torch.empty(rows2, device="cuda", dtype=torch.int32)
        num = torch.zeros(4, device="cuda", dtype=torch.int64)
        bk, bv, bko, bvo, bko2, bvo2, boff, boff2, bhist, bsums, bsums2, brk, bnum = (B(t) if t is not None else None for t in
                                                                                       (keys, values, ko, vo, ko2, vo2, off, off2, hist, sums, sums2, rk, num))
        bkt = clo.Bucket(ctx, kt, vs)
        srt = clo.Sorter("satradix", ctx, kt)
        hst = clo.Histogram(ctx, kt)
        scn = clo.Scanner("blelloch", ctx, "uint", "uint")
        red = clo.SegReduce("sum", "offsets", ctx, "uint", "ulong")
        rbk = clo.ReduceByKey(ctx, "uint", "uint", "ulong")
        keep = {}

        def ours():
            bkt.with_device_data(q, bk, bv, None if arg else bko, bvo if vs else None, boff, n, 0, 0, bins)
            if form == "pipeline":
                red.with_device_data(q, boff, None, bvo, bsums, bnum, bins, n)

        def sort_a():
            if vs:
                srt.by_key_with_device_data(q, bk, bv, None if arg else bko2, bvo2, n)
            else:
                srt.with_device_data(q, bk, bko2, n)
            if form == "pipeline":
                rbk.with_device_data(q, bko2, bvo2, brk, bsums2, bnum, n)
            else:
                hst.with_device_data(q, bk, None, bhist, n, 0, 0, bins)
                scn.with_device_data(q, bhist, boff2, bins + 1)           # the exclusive scan of the counts and a zero: the offsets

        def torch_b():
            s, i = torch.sort(keys, stable=True)
            keep["k"], keep["i"] = s, i
            if valued:
                keep["v"] = values[i]
            c = torch.bincount(keys, minlength=bins)
            keep["off"] = torch.cumsum(c, 0)
            if form == "pipeline":
                keep["sums"] = torch.zeros(bins, device="cuda", dtype=torch.int64).index_add_(0, keys.to(torch.int64), values.to(torch.int64))

        run = {"bucket": ours, "sort (a)": sort_a, "torch (b)": torch_b}
        variants = tuple(run)
        for v in variants:   # warm-up: code objects, the objects' workspaces, torch's allocator
            for _ in range(2):
                run[v]()
        torch.cuda.synchronize()
        # every output against torch before anything is timed
        agrees = bool(torch.equal(off[1:].to(torch.int64), keep["off"])) and int(off[0]) == 0
        if not arg:
            agrees = agrees and bool(torch.equal(ko, keep["k"]))
        if arg:
            agrees = agrees and bool(torch.equal(vo.to(torch.int64) & 0xFFFFFFFF, keep["i"]))
        if valued:
            agrees = agrees and bool(torch.equal(vo, keep["v"]))
        if form == "pipeline":
            agrees = agrees and bool(torch.equal(sums, keep["sums"]))
        else:
            agrees = agrees and bool(torch.equal(off2, off))              # baseline (a) computes the same offsets
        ms = {v: [] for v in variants}
        for r in range(args.reps):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                timer.start()
                run[v]()
                timer.stop()
                ms[v].append(timer.elapsed_ms())
        torch.cuda.synchronize()
        _hip.lib.clo_hip_timing_enable(1)
        _hip.lib.clo_hip_timing_reset()
        for _ in range(3):
            bkt.with_device_data(q, bk, bv, None if arg else bko, bvo if vs else None, boff, n, 0, 0, bins)
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        passes = 1 if bins + 1 <= 256 else 2
        by = schedule_bytes(n, ks, valued, arg, passes)
        V = {v: stats(ms[v]) for v in variants}
        med = V["bucket"]["median_ms"]
        entry = {"n": n, "bins": bins, "pattern": pattern, "form": form, "passes": passes, "reps": args.reps, "agrees_with_torch": agrees,
                 "bytes": by, "kernel_ms": kernel_ms, "variants": V, "bytes_per_s": round(by / (med * 1e-3)),
                 "fraction_of_peak": round(by / (med * 1e-3) / PEAK, 3),
                 "time_over_sort_a": round(med / V["sort (a)"]["median_ms"], 3), "time_over_torch_b": round(med / V["torch (b)"]["median_ms"], 3)}
        loses = [name for name, key in (("(a)", "time_over_sort_a"), ("(b)", "time_over_torch_b")) if entry[key] > 1.0]
        entry["verdict"] = "LOSES to " + " and ".join("%s by %.2fx" % (x, entry["time_over_sort_a" if x == "(a)" else "time_over_torch_b"]) for x in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in (bkt, srt, hst, scn, red, rbk, bk, bv, bko, bvo, bko2, bvo2, boff, boff2, bhist, bsums, bsums2, brk, bnum):
            if x is not None:
                x.close()
        keep.clear()
        del keys, values, ko, vo, ko2, vo2

    rec["legs_that_lose"] = [[e["n"], e["bins"], e["pattern"], e["form"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["agrees_with_torch"] for e in rec["legs"])
    timer.close()
    q.close()
    ctx.close()
    text = json.dumps(rec)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
