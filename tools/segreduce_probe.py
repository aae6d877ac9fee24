"""Measurement probe (not part of the bench contract): CloSegReduce against two baselines on the same inputs, on the
same GPU, in one process:
  (a) this library's own composition: CloExpand's segment ids, then CloReduceByKey on them. It drops empty segments, so
      it runs only on the legs that have none.
  (b) torch with the same result: for sums torch.cumsum gathered at the offsets; for min and max scatter_reduce_ on
      torch.repeat_interleave ids (output_size given, so that torch pays no host synchronisation); torch.segment_reduce
      where it accepts the dtype (reported as not accepted otherwise).

Legs, at 2^28 uint32 rows unless noted, uint32 counts, values below 2^31 so that torch's signed types hold them:
  sum at mean segment lengths 1, 16 and 4096, and a single segment; half of the segments empty; min and max; uint64 sums;
  the offsets form; 2^24 rows
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for 10 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the model's bytes
n value_size + m (count_size + sum_size), the workspace traffic on top (counts form: the counts read twice more, the ends
written and read; 20 bytes per tile), both as a fraction of the 8 TB/s peak, and its time over the baselines'; LOSES where
it is slower than one. Every output is compared with torch's. Then one pass with the library's per-kernel events: where
the time goes.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/segreduce_probe.py [--log2n 28] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("segreduce_sums", "segreduce_sums_scan", "segreduce_ends", "segreduce_partition", "segreduce_sweep", "segreduce_carry", "segreduce_fixup")


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
    T = clo.segreduce_tile(4, 4)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "segreduce_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": T, "legs": []}
    g = torch.Generator(device="cuda").manual_seed(21)

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

    # (name, rows, counts kind, op, sum size, form)
    legs = [("sum, mean length %d" % ln, N, "mean %d" % ln, "sum", 4, "counts") for ln in (1, 16, 4096) if ln < N]
    legs += [("sum, a single segment", N, "single", "sum", 4, "counts"),
             ("sum, half of the segments empty, mean length 16", N, "half empty mean 16", "sum", 4, "counts"),
             ("min, mean length 16", N, "mean 16", "min", 4, "counts"),
             ("max, mean length 16", N, "mean 16", "max", 4, "counts"),
             ("uint64 sums, mean length 16", N, "mean 16", "sum", 8, "counts"),
             ("sum, the offsets form, mean length 16", N, "mean 16", "sum", 4, "offsets")]
    if args.log2n > 24:
        legs.append(("sum, 2^24 rows, mean length 16", 1 << 24, "mean 16", "sum", 4, "counts"))

    for name, n, kind, op, ss, form in legs:
        torch.cuda.empty_cache()
        counts = counts_for(kind, n)
        m = counts.numel()
        assert int(counts.sum(dtype=torch.int64)) == n
        empties = bool((counts == 0).any())
        sdt = torch.int64 if ss == 8 else torch.int32
        values = torch.randint(0, 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        off64 = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts, 0, dtype=torch.int64)))
        offsets = off64.to(torch.int32)
        src = offsets if form == "offsets" else counts
        ao = torch.empty(m, device="cuda", dtype=sdt)
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        seg, ao2, runs = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n if not empties else 2, device="cuda", dtype=sdt), torch.zeros(2, device="cuda", dtype=torch.int64)
        ids = torch.arange(m, device="cuda", dtype=torch.int64)
        st = "ulong" if ss == 8 else "uint"
        sr = clo.SegReduce(op, form, ctx, "uint", st, "uint")
        ex, rbk = clo.Expand("counts", ctx, None, "uint"), clo.ReduceByKey(ctx, "uint", "uint", st, op)
        bufs = {k: B(t) for k, t in (("src", src), ("values", values), ("ao", ao), ("num", num), ("counts", counts), ("seg", seg), ("ao2", ao2), ("runs", runs))}
        keep = {}

        def torch_leg():
            if op == "sum":
                run = torch.cat((torch.zeros(1, dtype=sdt, device="cuda"), torch.cumsum(values, 0, dtype=sdt)))     # wraps modulo 2^bits
                keep["a"] = run[off64[1:]] - run[off64[:-1]]
            else:
                rows = torch.repeat_interleave(ids, counts, output_size=n)
                out = torch.full((m,), (1 << 31) - 1 if op == "min" else 0, dtype=torch.int32, device="cuda")
                keep["a"] = out.scatter_reduce_(0, rows, values, "amin" if op == "min" else "amax", include_self=True)

        def composition():
            ex.with_device_data(q, bufs["counts"], None, None, None, bufs["seg"], None, bufs["num"], m, n)
            rbk.with_device_data(q, bufs["seg"], bufs["values"], None, bufs["ao2"], bufs["runs"], n)

        def segment_reduce():
            keep["s"] = torch.segment_reduce(values, op, lengths=counts.to(torch.int64), unsafe=True)

        run = {"segreduce": lambda: sr.with_device_data(q, bufs["src"], None, bufs["values"], bufs["ao"], bufs["num"], m, n), "torch": torch_leg}
        if not empties:
            run["composition"] = composition
        try:
            torch_leg()
            torch.cuda.synchronize()
            torch_runs = True
        except Exception as e:   # noqa: BLE001  (a torch build without this reduction for int32: the leg goes without it, and says so)
            torch_runs = type(e).__name__
            del run["torch"]
        try:
            segment_reduce()
            torch.cuda.synchronize()
            run["torch.segment_reduce"] = segment_reduce
            accepted = True
        except Exception as e:   # noqa: BLE001  (whatever torch raises for a dtype it does not take)
            accepted = type(e).__name__
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
            run["segreduce"]()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        num.fill_(-1)
        for v in variants:
            run[v]()
        torch.cuda.synchronize()
        # the identity of an empty segment: torch's cumsum difference gives 0 as well; the legs with empties are sums
        agrees = int(num[0].item()) == n and bool(torch.equal(ao, keep["a"].to(sdt))) if torch_runs is True else None
        composition_agrees = bool(torch.equal(ao2[:m], ao)) and int(runs[0].item()) == m if not empties else None
        by = 4 * n + m * (4 + ss)
        tiles = -(-(m + n) // T)
        ws = ((2 * 4 + 2 * 8) * m if form == "counts" else 0) + 20 * tiles
        V = {v: stats(ms[v]) for v in variants}
        med = V["segreduce"]["median_ms"]
        entry = {"leg": name, "rows": n, "segments": m, "op": op, "sum_size": ss, "form": form, "reps": args.reps, "agrees_with_torch": agrees, "torch_runs": torch_runs,
                 "composition_agrees": composition_agrees, "torch_segment_reduce_accepts_int32": accepted, "model_bytes": by, "workspace_bytes": ws,
                 "kernel_ms": kernel_ms, "variants": V, "fraction_of_peak_model": round(by / (med * 1e-3) / PEAK, 3),
                 "fraction_of_peak_with_workspace": round((by + ws) / (med * 1e-3) / PEAK, 3),
                 "time_over": {w: round(med / V[w]["median_ms"], 3) for w in variants if w != "segreduce"}}
        loses = [w for w in variants if w != "segreduce" and med > V[w]["median_ms"]]
        entry["verdict"] = "LOSES to " + " and to ".join("the composition (%.2fx)" % entry["time_over"][w] if w == "composition" else "%s (%.2fx)" % (w, entry["time_over"][w])
                                                         for w in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in list(bufs.values()) + [sr, ex, rbk]:
            x.close()
        keep.clear()
        del counts, values, off64, offsets, src, ao, seg, ao2, ids

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["agrees_with_torch"] is not False and e["composition_agrees"] is not False for e in rec["legs"])
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
