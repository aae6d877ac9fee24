"""Measurement probe (not part of the bench contract): CloExpand against torch.repeat_interleave with output_size given
(so that torch pays no host synchronisation) and against this library's own composition — clo_scan_* of the counts, then
CloSearch with UPPER | NEEDLES_SORTED on an iota array of needles, which yields the segment ids (plus one) alone and
gathers no values — on the same inputs, on the same GPU, in one process.

Legs, at 2^28 output rows unless noted, uint32 counts:
  uint32 values and seg_out at mean segment lengths 1, 16, 4096 and 2^20; a single segment; half of the segments empty
  seg_out alone; all three outputs; uint64 values
  the offsets form against the counts form on the same data
  2^24 rows
  tiles with exactly L and L + 1 segment ends (2^26 rows): the LDS marks against the per-row search in global memory
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for 10 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports its floor's bytes (the
outputs asked for written once, 8 (m + 1) bytes of ends and value_size m bytes of values read once; the counts form also
its scan: the counts read twice, the ends written), those bytes per second as a fraction of the 8 TB/s peak, and its time
over both baselines'; LOSES where it is slower than either. Every output is compared with torch's. Then one pass with
the library's per-kernel events: where the time goes.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/expand_probe.py [--log2n 28] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("expand_sums", "expand_sums_scan", "expand_ends", "expand_partition", "expand")


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
    T, L = clo.expand_tile(4), clo.expand_lds_segments()
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "expand_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": T, "lds_segments": L, "legs": []}
    g = torch.Generator(device="cuda").manual_seed(20)

    def counts_for(kind, n):
        """int32 counts whose sum is n."""
        if kind == "single":
            return torch.tensor([n], dtype=torch.int32, device="cuda")
        if kind.startswith("ends per tile "):                                 # every tile: K ends, T of them of segments of one row
            k = int(kind.split()[-1])
            mid = torch.cat((torch.ones(T - 2, dtype=torch.int32, device="cuda"), torch.zeros(k - T, dtype=torch.int32, device="cuda")))
            mid = mid[torch.randperm(mid.numel(), device="cuda", generator=g)]
            one = torch.ones(1, dtype=torch.int32, device="cuda")
            return torch.cat((one, mid, one)).repeat(n // T)
        mean = int(kind.split()[-1])
        if mean == 1:
            return torch.ones(n, dtype=torch.int32, device="cuda")
        m = n // mean // (2 if kind.startswith("half empty") else 1)
        cuts = torch.sort(torch.randint(0, n, (m - 1,), device="cuda", generator=g))[0]
        edge = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), cuts, torch.tensor([n], dtype=torch.int64, device="cuda")))
        c = (edge[1:] - edge[:-1]).to(torch.int32)
        if kind.startswith("half empty"):
            both = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
            both[1::2] = c
            return both
        return c

    # (name, rows, counts kind, value size, outputs (values, seg, rank), form)
    legs = [("uint32 values and seg_out, mean length %d" % ln, N, "mean %d" % ln, 4, (1, 1, 0), "counts") for ln in (1, 16, 4096, 1 << 20) if ln < N]
    legs += [("a single segment", N, "single", 4, (1, 1, 0), "counts"),
             ("half of the segments empty, mean length 16", N, "half empty mean 16", 4, (1, 1, 0), "counts"),
             ("seg_out alone, mean length 16", N, "mean 16", 0, (0, 1, 0), "counts"),
             ("all three outputs, mean length 16", N, "mean 16", 4, (1, 1, 1), "counts"),
             ("uint64 values and seg_out, mean length 16", N, "mean 16", 8, (1, 1, 0), "counts"),
             ("the offsets form, mean length 16", N, "mean 16", 4, (1, 1, 0), "offsets")]
    if args.log2n > 24:
        legs.append(("2^24 rows, mean length 16", 1 << 24, "mean 16", 4, (1, 1, 0), "counts"))
    edge_n = min(N, 1 << 26)
    legs += [("%d ends in every tile (%s)" % (k, how), edge_n, "ends per tile %d" % k, 4, (1, 1, 0), "counts")
             for k, how in ((L, "LDS marks"), (L + 1, "per-row search in global memory"))]

    for name, n, kind, vs, outs, form in legs:
        torch.cuda.empty_cache()
        counts = counts_for(kind, n)
        m = counts.numel()
        assert int(counts.sum(dtype=torch.int64)) == n
        vdt = torch.int64 if vs == 8 else torch.int32
        values = torch.randint(-(1 << 31), 1 << 31, (m,), device="cuda", dtype=vdt, generator=g) if outs[0] else None
        offsets = torch.cat((torch.zeros(1, dtype=torch.int32, device="cuda"), torch.cumsum(counts, 0, dtype=torch.int64).to(torch.int32)))
        src = offsets if form == "offsets" else counts
        vo = torch.empty(n, device="cuda", dtype=vdt) if outs[0] else None
        so = torch.empty(n, device="cuda", dtype=torch.int32) if outs[1] else None
        ro = torch.empty(n, device="cuda", dtype=torch.int32) if outs[2] else None
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        # the composition: starts = exclusive scan of the counts; pos = upper bound of row j among the starts = r(j) + 1
        starts, iota, pos = torch.empty_like(counts), torch.arange(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.int32)
        ids = torch.arange(m, device="cuda", dtype=torch.int32)
        ex = clo.Expand(form, ctx, "ulong" if vs == 8 else "uint", "uint")
        scan, search = clo.Scanner("blelloch", ctx, "uint", "uint"), clo.Search(ctx, "uint")
        bufs = {k: (B(t) if t is not None else None) for k, t in (("src", src), ("values", values), ("vo", vo), ("so", so), ("ro", ro), ("num", num),
                                                                    ("counts", counts), ("starts", starts), ("iota", iota), ("pos", pos))}
        keep = {}

        def torch_leg():
            if outs[0]:
                keep["v"] = torch.repeat_interleave(values, counts, output_size=n)
            if outs[1] or outs[2]:
                keep["s"] = torch.repeat_interleave(ids, counts, output_size=n)
            if outs[2]:
                keep["r"] = iota - offsets[:-1][keep["s"]]

        def composition():
            scan.with_device_data(q, bufs["counts"], bufs["starts"], m)
            search.with_device_data(q, bufs["starts"], m, bufs["iota"], n, bufs["pos"], upper=True, needles_sorted=True)

        run = {"expand": lambda: ex.with_device_data(q, bufs["src"], None, bufs["values"], bufs["vo"], bufs["so"], bufs["ro"], bufs["num"], m, n),
               "torch": torch_leg, "composition": composition}
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
            run["expand"]()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        for v in variants:
            run[v]()
        torch.cuda.synchronize()
        agrees = int(num[0].item()) == n
        if outs[0]:
            agrees = agrees and bool(torch.equal(vo, keep["v"]))
        if outs[1]:
            agrees = agrees and bool(torch.equal(so, keep["s"]))
        if outs[2]:
            agrees = agrees and bool(torch.equal(ro, keep["r"]))
        composition_agrees = bool(torch.equal(pos - 1, keep["s"])) if "s" in keep else None
        by = n * (vs * outs[0] + 4 * outs[1] + 4 * outs[2]) + 8 * (m + 1) + vs * m * outs[0] + ((2 * 4 + 8) * m if form == "counts" else 0)
        V = {v: stats(ms[v]) for v in variants}
        med = V["expand"]["median_ms"]
        entry = {"leg": name, "rows": n, "segments": m, "value_size": vs, "outputs": "+".join(w for w, o in zip(("values", "seg", "rank"), outs) if o),
                 "form": form, "reps": args.reps, "agrees_with_torch": agrees, "composition_agrees_with_torch": composition_agrees,
                 "floor_bytes": by, "kernel_ms": kernel_ms, "variants": V, "fraction_of_peak": round(by / (med * 1e-3) / PEAK, 3),
                 "time_over_torch": round(med / V["torch"]["median_ms"], 3), "time_over_composition": round(med / V["composition"]["median_ms"], 3)}
        loses = [w for w in ("torch", "composition") if med > V[w]["median_ms"]]
        entry["verdict"] = "LOSES to " + " and to ".join("the " + w if w == "composition" else w for w in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in list(bufs.values()) + [ex, scan, search]:
            if x is not None:
                x.close()
        keep.clear()
        del counts, values, offsets, src, vo, so, ro, starts, iota, pos, ids

    by_name = {e["leg"]: e for e in rec["legs"]}
    lds, glob = (by_name.get("%d ends in every tile (%s)" % (k, how)) for k, how in ((L, "LDS marks"), (L + 1, "per-row search in global memory")))
    rec["fallback_stays_a_fallback"] = lds["variants"]["expand"]["median_ms"] <= glob["variants"]["expand"]["median_ms"]
    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["agrees_with_torch"] and e["composition_agrees_with_torch"] is not False for e in rec["legs"])
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
