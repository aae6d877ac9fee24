"""Measurement probe (not part of the bench contract): CloSegScan against two baselines on the same inputs, on the same
GPU, in one process:
  (a) this library's own composition: CloExpand's segment ids, then CloScanByKey on them.
  (b) torch with the same result, for sums only: torch.cumsum minus the cumsum gathered at each row's segment start, the
      starts spread over the rows by torch.repeat_interleave (output_size given, so that torch pays no host
      synchronisation).

Legs, at 2^28 uint32 rows unless noted, uint32 counts, values below 2^31 so that torch's signed types hold them:
  exclusive sum at mean segment lengths 1, 16 and 4096, and a single segment; at mean length 16: half of the segments
  empty, min, max, uint64 sums, inclusive, the offsets form, in place; 2^24 rows
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for 10 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the model's bytes
n (value_size + sum_size) + m count_size, the workspace traffic on top (counts form: the counts read twice more, the ends
written and read; 32 bytes per tile; the rows behind every tile's last close, read once more, are not counted: the
per-kernel time of the tails launch shows them), both as a fraction of the 8 TB/s peak, and its time over the baselines';
LOSES where it is slower than one. Every output is compared with the baselines'. Each leg ends with one pass with the
library's per-kernel events: where the time goes.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/segscan_probe.py [--log2n 28] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("segscan_sums", "segscan_sums_scan", "segscan_ends", "segscan_partition", "segscan_tails", "segscan_carry", "segscan_sweep")


def stats(ms):
    t = sorted(ms)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    N = 1 << args.log2n
    T = clo.segscan_tile(4, 4)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "segscan_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": T, "legs": []}
    g = torch.Generator(device="cuda").manual_seed(23)

    def counts_for(kind, n):
        """int32 counts whose sum is n."""
        if kind == "single":
            return torch.tensor([n], dtype=torch.int32, device="cuda")
        mean = int(kind.split()[-1])
        if mean == 1:
            return torch.ones(n, dtype=torch.int32, device="cuda")
        m = n // mean // (2 if kind.startswith("half empty") else 1)
        cuts = torch.sort(torch.randperm(n - 1, device="cuda", generator=g)[:m - 1] + 1)[0]      # distinct: no segment is empty
        edge = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), cuts, torch.tensor([n], dtype=torch.int64, device="cuda")))
        c = (edge[1:] - edge[:-1]).to(torch.int32)
        if kind.startswith("half empty"):
            both = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
            both[1::2] = c
            return both
        return c

    # (name, rows, counts kind, op, sum size, form, inclusive, in place)
    legs = [("exclusive sum, mean length %d" % ln, N, "mean %d" % ln, "sum", 4, "counts", False, False) for ln in (1, 16, 4096) if ln < N]
    legs += [("exclusive sum, a single segment", N, "single", "sum", 4, "counts", False, False),
             ("exclusive sum, half of the segments empty, mean length 16", N, "half empty mean 16", "sum", 4, "counts", False, False),
             ("exclusive min, mean length 16", N, "mean 16", "min", 4, "counts", False, False),
             ("exclusive max, mean length 16", N, "mean 16", "max", 4, "counts", False, False),
             ("exclusive uint64 sums, mean length 16", N, "mean 16", "sum", 8, "counts", False, False),
             ("inclusive sum, mean length 16", N, "mean 16", "sum", 4, "counts", True, False),
             ("exclusive sum, the offsets form, mean length 16", N, "mean 16", "sum", 4, "offsets", False, False),
             ("exclusive sum in place, mean length 16", N, "mean 16", "sum", 4, "counts", False, True)]
    if args.log2n > 24:
        legs.append(("exclusive sum, 2^24 rows, mean length 16", 1 << 24, "mean 16", "sum", 4, "counts", False, False))

    for name, n, kind, op, ss, form, incl, in_place in legs:
        torch.cuda.empty_cache()
        counts = counts_for(kind, n)
        m = counts.numel()
        assert int(counts.sum(dtype=torch.int64)) == n
        sdt = torch.int64 if ss == 8 else torch.int32
        values = torch.randint(0, 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        saved = values.clone() if in_place else None
        off64 = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts, 0, dtype=torch.int64)))
        offsets = off64.to(torch.int32)
        src = offsets if form == "offsets" else counts
        out = values if in_place else torch.empty(n, device="cuda", dtype=sdt)
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        seg, out2 = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=sdt)
        st = "ulong" if ss == 8 else "uint"
        sc = clo.SegScan(op, form, ctx, "uint", st, "uint", inclusive=incl)
        ex, sbk = clo.Expand("counts", ctx, None, "uint"), clo.ScanByKey(ctx, "uint", "uint", st, op, incl)
        bufs = {k: B(t) for k, t in (("src", src), ("values", values), ("out", out), ("num", num), ("counts", counts), ("seg", seg), ("out2", out2))}
        keep = {}

        def torch_leg():
            run = torch.cat((torch.zeros(1, dtype=sdt, device="cuda"), torch.cumsum(values, 0, dtype=sdt)))     # wraps modulo 2^bits
            start = torch.repeat_interleave(off64[:-1], counts, output_size=n)
            keep["a"] = (run[1:] if incl else run[:-1]) - run[start]

        def composition():
            ex.with_device_data(q, bufs["counts"], None, None, None, bufs["seg"], None, bufs["num"], m, n)
            sbk.with_device_data(q, bufs["seg"], bufs["values"], bufs["out2"], n)

        run = {"segscan": lambda: sc.with_device_data(q, bufs["src"], None, bufs["values"], bufs["out"], bufs["num"], m, n), "composition": composition}
        if op == "sum":
            run["torch"] = torch_leg
        variants = tuple(run)
        for v in variants:   # warm-up: code objects, the objects' scratch, torch's allocator
            for _ in range(2):
                run[v]()
        torch.cuda.synchronize()
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
            run["segscan"]()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        num.fill_(-1)
        if in_place:   # the values again: the baselines first, from the values; the scan last, onto them
            values.copy_(saved)
        for v in variants[::-1]:
            run[v]()
        torch.cuda.synchronize()
        agrees = bool(torch.equal(out, keep["a"].to(sdt))) if op == "sum" else None
        composition_agrees = bool(torch.equal(out2, out.to(sdt))) and int(num[0].item()) == n
        by = n * (4 + ss) + m * 4
        tiles = -(-(m + n) // T)
        ws = ((2 * 4 + 2 * 8) * m if form == "counts" else 0) + 32 * tiles
        V = {v: stats(ms[v]) for v in variants}
        med = V["segscan"]["median_ms"]
        entry = {"leg": name, "rows": n, "segments": m, "op": op, "sum_size": ss, "form": form, "inclusive": incl, "in_place": in_place, "reps": args.reps,
                 "agrees_with_torch": agrees, "composition_agrees": composition_agrees, "model_bytes": by, "workspace_bytes": ws,
                 "kernel_ms": kernel_ms, "variants": V, "fraction_of_peak_model": round(by / (med * 1e-3) / PEAK, 3),
                 "fraction_of_peak_with_workspace": round((by + ws) / (med * 1e-3) / PEAK, 3),
                 "time_over": {w: round(med / V[w]["median_ms"], 3) for w in variants if w != "segscan"}}
        loses = [w for w in variants if w != "segscan" and med > V[w]["median_ms"]]
        entry["verdict"] = "LOSES to " + " and to ".join("the composition (%.2fx)" % entry["time_over"][w] if w == "composition" else "%s (%.2fx)" % (w, entry["time_over"][w])
                                                         for w in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in list(bufs.values()) + [sc, ex, sbk]:
            x.close()
        keep.clear()
        del counts, values, saved, off64, offsets, src, out, seg, out2

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["agrees_with_torch"] is not False and e["composition_agrees"] is not False for e in rec["legs"])
    rec["not_measured"] = ["ulong counts", "64-bit values", "num_in", "totals above or below the rows", "min and max at other lengths than 16",
                           "the bytes of the open tails"]
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
