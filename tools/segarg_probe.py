"""Measurement probe (not part of the bench contract): CloSegArg against two baselines on the same inputs, on the same
GPU, in one process:
  (a) CloSegReduce min of the same values (their bits as uint or ulong): the value without the index, the floor for the
      same bytes read.
  (b) for uint values, the composition that was the only route to an index inside this library: torch packs
      (value << 32) | row into 64-bit words, CloSegReduce min reduces them as ulong, torch unpacks. It gives the same idx
      for tie "first" where a segment has a row; that is verified before timing.

Legs, at 2^28 uint32 rows unless noted, uint32 counts, argmin, tie first, val_out written; the values' bits are below
2^31, so that every type orders them as unsigned numbers and (a) checks val_out for all of them:
  mean segment lengths 1, 16 and 4096, and a single segment; half of the segments empty; tie last; val_out off; float,
  ulong and double values; the offsets form; 2^24 rows
Every variant of every leg is warmed up first; then the variants alternate, timed with device events on one stream, for
10 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the model's bytes (the rows
read once, the counts, idx_out and val_out) as a fraction of the 8 TB/s peak, and its time over the baselines'; LOSES
where it is slower than one. Then one pass with the library's per-kernel events: where the time goes.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/segarg_probe.py [--log2n 28] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("segarg_sums", "segarg_sums_scan", "segarg_ends", "segarg_partition", "segarg_sweep", "segarg_carry", "segarg_fixup")


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
    T = clo.segarg_tile(4)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "segarg_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": T, "carry_tiles": clo.segarg_carry_tiles(), "legs": []}
    g = torch.Generator(device="cuda").manual_seed(25)

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

    # (name, rows, counts kind, value type, tie, val_out, form)
    legs = [("mean length %d" % ln, N, "mean %d" % ln, "uint", "first", True, "counts") for ln in (1, 16, 4096) if ln < N]
    legs += [("a single segment", N, "single", "uint", "first", True, "counts"),
             ("half of the segments empty, mean length 16", N, "half empty mean 16", "uint", "first", True, "counts"),
             ("tie last, mean length 16", N, "mean 16", "uint", "last", True, "counts"),
             ("val_out off, mean length 16", N, "mean 16", "uint", "first", False, "counts"),
             ("float, mean length 16", N, "mean 16", "float", "first", True, "counts"),
             ("ulong, mean length 16", N, "mean 16", "ulong", "first", True, "counts"),
             ("double, mean length 16", N, "mean 16", "double", "first", True, "counts"),
             ("the offsets form, mean length 16", N, "mean 16", "uint", "first", True, "offsets")]
    if args.log2n > 24:
        legs.append(("2^24 rows, mean length 16", 1 << 24, "mean 16", "uint", "first", True, "counts"))

    for name, n, kind, vt, tie, with_val, form in legs:
        torch.cuda.empty_cache()
        counts = counts_for(kind, n)
        m = counts.numel()
        assert int(counts.sum(dtype=torch.int64)) == n
        vs = 8 if vt in ("ulong", "double") else 4
        vdt = torch.int64 if vs == 8 else torch.int32
        # few distinct values in the upper bits, so that ties are decided by the index; the bits stay below 2^31 (2^63)
        values = torch.randint(0, 1 << 10, (n,), device="cuda", dtype=torch.int32, generator=g).to(vdt) << (50 if vs == 8 else 20)
        off64 = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts, 0, dtype=torch.int64)))
        src = off64.to(torch.int32) if form == "offsets" else counts
        full = counts > 0
        io, vo = torch.empty(m, device="cuda", dtype=torch.int32), torch.empty(m, device="cuda", dtype=vdt)
        ao, num, num2 = torch.empty(m, device="cuda", dtype=vdt), torch.zeros(2, device="cuda", dtype=torch.int64), torch.zeros(2, device="cuda", dtype=torch.int64)
        ut = "ulong" if vs == 8 else "uint"
        sa = clo.SegArg("argmin", tie, form, ctx, vt, "uint")
        sr = clo.SegReduce("min", form, ctx, ut, ut, "uint")
        bufs = {k: B(t) for k, t in (("src", src), ("values", values), ("io", io), ("vo", vo), ("ao", ao), ("num", num), ("num2", num2))}
        run = {"segarg": lambda: sa.with_device_data(q, bufs["src"], None, bufs["values"], bufs["io"], bufs["vo"] if with_val else None, bufs["num"], m, n),
               "segreduce min": lambda: sr.with_device_data(q, bufs["src"], None, bufs["values"], bufs["ao"], bufs["num2"], m, n)}
        keep = {}
        objs = [sa, sr]
        if vt == "uint":
            packed, po = torch.empty(n, device="cuda", dtype=torch.int64), torch.empty(m, device="cuda", dtype=torch.int64)
            rows = torch.arange(n, device="cuda", dtype=torch.int64)
            sr8 = clo.SegReduce("min", form, ctx, "ulong", "ulong", "uint")
            bufs["packed"], bufs["po"] = B(packed), B(po)
            objs.append(sr8)

            def composition():
                torch.bitwise_or(values.to(torch.int64) << 32, rows, out=packed)
                sr8.with_device_data(q, bufs["src"], None, bufs["packed"], bufs["po"], bufs["num2"], m, n)
                keep["idx"], keep["val"] = (po & 0xffffffff).to(torch.int32), (po >> 32).to(torch.int32)

            run["pack + segreduce + unpack"] = composition
        variants = tuple(run)
        for v in variants:   # warm-up: code objects, the objects' scratch, torch's allocator
            for _ in range(2):
                run[v]()
        torch.cuda.synchronize()
        # the results, before anything is timed
        agrees_a = bool(torch.equal(vo[full], ao[full])) if with_val else None
        agrees_b = None
        if vt == "uint" and tie == "first":
            agrees_b = bool(torch.equal(io[full], keep["idx"][full])) and (not with_val or bool(torch.equal(vo[full], keep["val"][full])))
        none_ok = bool((io[~full] == -1).all()) and int(num[0].item()) == n
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
            run["segarg"]()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        by = vs * n + m * (4 + 4 + (vs if with_val else 0))
        V = {v: stats(ms[v]) for v in variants}
        med = V["segarg"]["median_ms"]
        entry = {"leg": name, "rows": n, "segments": m, "value_type": vt, "tie": tie, "val_out": with_val, "form": form, "reps": args.reps,
                 "val_out_equals_segreduce_min": agrees_a, "idx_out_equals_the_composition": agrees_b, "empty_segments_and_total_ok": none_ok,
                 "model_bytes": by, "kernel_ms": kernel_ms, "variants": V, "fraction_of_peak_model": round(by / (med * 1e-3) / PEAK, 3),
                 "time_over": {w: round(med / V[w]["median_ms"], 3) for w in variants if w != "segarg"}}
        loses = [w for w in variants if w != "segarg" and med > V[w]["median_ms"]]
        entry["verdict"] = "LOSES to " + " and to ".join("%s (%.2fx)" % (w, entry["time_over"][w]) for w in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in list(bufs.values()) + objs:
            x.close()
        keep.clear()
        del counts, values, off64, src, io, vo, ao
        if vt == "uint":
            del packed, po, rows

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["val_out_equals_segreduce_min"] is not False and e["idx_out_equals_the_composition"] is not False
                                     and e["empty_segments_and_total_ok"] for e in rec["legs"])
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
