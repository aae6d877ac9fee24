"""Measurement probe (not part of the bench contract): CloSegSort against three baselines on the same inputs, on the same
GPU, in one process:
  (a) the composition a caller had before: CloExpand's segment ids, packed with the key into 64 bits by torch
      ((id << 32) | key), this library's satradix sort of the ulong elements, unpacked by torch; the whole chain is timed.
      It exists for 4-byte keys without values.
  (b) torch alone: a stable sort of the packed int64 (4-byte keys; with values or in the arg form the gather by the
      sort's indices is part of it). 8-byte keys do not pack: two stable argsorts, by key and then by segment id.
  (c) on the legs with a few huge segments: clo_sort_* (satradix) once per segment, which is what clo_segsort.h tells
      such a caller to do. (The segments of the 2^20 leg all have exactly 2^20 rows, so that they are slices.)

Legs, at 2^28 uint32 rows unless noted, uint32 counts, keys below 2^31 so that torch's signed types order them alike:
  mean segment length 1, 16, 256, T / 2, 4 T and 2^20, a single segment, half of the segments empty, uint32 values, the
  arg form, uint64 keys, the offsets form, 2^24 rows
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for 10 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the model's bytes
2 n (key_size + value_size) + m count_size as a fraction of the 8 TB/s peak, and its time over the baselines'; LOSES
where it is slower than one. Every output is compared with baseline (b)'s. Then one pass with the library's per-kernel
events: where the time goes.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/segsort_probe.py [--log2n 28] [--reps 10] [--out FILE] [--legs a,b]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("segsort_sums", "segsort_sums_scan", "segsort_ends", "segsort_zero", "segsort_heads", "segsort_tile", "segsort_merge")


def stats(ms):
    t = sorted(ms)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--legs", default="", help="comma-separated leg numbers (all when empty)")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    N = 1 << args.log2n
    T = clo.segsort_tile(4, 0)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "segsort_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": T, "legs": []}
    g = torch.Generator(device="cuda").manual_seed(22)

    def counts_for(kind, n):
        """int32 counts whose sum is n."""
        if kind == "single":
            return torch.tensor([n], dtype=torch.int32, device="cuda")
        if kind.startswith("equal"):
            ln = int(kind.split()[-1])
            return torch.full((n // ln,), ln, dtype=torch.int32, device="cuda")
        mean = int(kind.split()[-1])
        if mean == 1:
            return torch.ones(n, dtype=torch.int32, device="cuda")
        m = max(n // mean // (2 if kind.startswith("half empty") else 1), 2)
        cuts = torch.sort(torch.randperm(n - 1, device="cuda", generator=g)[:m - 1] + 1)[0]      # distinct: no segment is empty
        edge = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), cuts, torch.tensor([n], dtype=torch.int64, device="cuda")))
        c = (edge[1:] - edge[:-1]).to(torch.int32)
        if kind.startswith("half empty"):
            both = torch.zeros(2 * m, dtype=torch.int32, device="cuda")
            both[1::2] = c
            return both
        return c

    big = 1 << 20
    # (name, rows, counts kind, key size, mode, form); mode: keys, v4 or arg
    legs = [("mean length %d" % ln, N, "mean %d" % ln, 4, "keys", "counts") for ln in (1, 16, 256, T // 2, 4 * T) if ln < N]
    if big < N:
        legs.append(("2^20 rows in every segment", N, "equal %d" % big, 4, "keys", "counts"))
    legs += [("a single segment", N, "single", 4, "keys", "counts"),
             ("half of the segments empty, mean length 16", N, "half empty mean 16", 4, "keys", "counts"),
             ("uint32 values, mean length 16", N, "mean 16", 4, "v4", "counts"),
             ("the arg form, mean length 16", N, "mean 16", 4, "arg", "counts"),
             ("uint64 keys, mean length 16", N, "mean 16", 8, "keys", "counts"),
             ("the offsets form, mean length 16", N, "mean 16", 4, "keys", "offsets")]
    if args.log2n > 24:
        legs.append(("2^24 rows, mean length 16", 1 << 24, "mean 16", 4, "keys", "counts"))
    want = {int(x) for x in args.legs.split(",") if x} if args.legs else None

    for number, (name, n, kind, ks, mode, form) in enumerate(legs):
        if want is not None and number not in want:
            continue
        torch.cuda.empty_cache()
        counts = counts_for(kind, n)
        m = counts.numel()
        assert int(counts.sum(dtype=torch.int64)) == n
        kdt = torch.int64 if ks == 8 else torch.int32
        keys = torch.randint(0, 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g).to(kdt)
        if ks == 8:
            keys = keys * 2654435761 + 12345                                                    # above 2^32, still positive
        vs = 0 if mode == "keys" else 4
        values = torch.randint(0, 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g) if mode == "v4" else None
        off64 = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts, 0, dtype=torch.int64)))
        src = off64.to(torch.int32) if form == "offsets" else counts
        ko = torch.empty(n, device="cuda", dtype=kdt)
        vo = torch.empty(n if vs else 2, device="cuda", dtype=torch.int32)
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        ss = clo.SegSort(form, ctx, "ulong" if ks == 8 else "uint", vs, "uint")
        bufs = {k: B(t) for k, t in (("src", src), ("keys", keys), ("ko", ko), ("vo", vo), ("num", num), ("counts", counts))}
        if values is not None:
            bufs["values"] = B(values)
        keep = {}
        closing = [ss]

        def segsort():
            ss.with_device_data(q, bufs["src"], None, bufs["keys"], bufs.get("values"), bufs["ko"], bufs["vo"] if vs else None, bufs["num"], m, n)

        def torch_leg():
            ids = torch.repeat_interleave(torch.arange(m, device="cuda", dtype=torch.int64), counts, output_size=n)
            if ks == 4:
                s, idx = torch.sort((ids << 32) | keys.to(torch.int64), stable=True)
                keep["k"] = (s & 0xffffffff).to(torch.int32)
            else:
                i1 = torch.sort(keys, stable=True)[1]
                idx = i1[torch.sort(ids[i1], stable=True)[1]]
                keep["k"] = keys[idx]
            if mode == "v4":
                keep["v"] = values[idx]
            elif mode == "arg":
                keep["v"] = idx.to(torch.int32)

        run = {"segsort": segsort, "torch": torch_leg}
        if ks == 4 and mode == "keys":
            seg = torch.empty(n, device="cuda", dtype=torch.int32)
            packed, sorted_ = torch.empty(n, device="cuda", dtype=torch.int64), torch.empty(n, device="cuda", dtype=torch.int64)
            ex, sorter = clo.Expand("counts", ctx, None, "uint"), clo.Sorter("satradix", ctx, "ulong")
            bufs.update(seg=B(seg), packed=B(packed), sorted=B(sorted_), num2=B(torch.zeros(2, device="cuda", dtype=torch.int64)))
            closing += [ex, sorter]

            def composition():
                ex.with_device_data(q, bufs["counts"], None, None, None, bufs["seg"], None, bufs["num2"], m, n)
                torch.add(seg.to(torch.int64) << 32, keys, out=packed)
                sorter.with_device_data(q, bufs["packed"], bufs["sorted"], n)
                keep["c"] = (sorted_ & 0xffffffff).to(torch.int32)
            run["composition"] = composition
        if kind == "single" or kind.startswith("equal"):
            ln = n if kind == "single" else int(kind.split()[-1])
            plain = clo.Sorter("satradix", ctx, "uint")
            po = torch.empty(n, device="cuda", dtype=torch.int32)
            parts = [(B(keys[a:a + ln]), B(po[a:a + ln])) for a in range(0, n, ln)]
            closing += [plain] + [b for pair in parts for b in pair]

            def per_segment():
                for a, b in parts:
                    plain.with_device_data(q, a, b, ln)
                keep["p"] = po
            run["clo_sort per segment"] = per_segment

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
            segsort()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        num.fill_(-1)
        ko.fill_(-1)
        for v in variants:
            run[v]()
        torch.cuda.synchronize()
        agrees = int(num[0].item()) == n and bool(torch.equal(ko, keep["k"])) and (not vs or bool(torch.equal(vo, keep["v"])))
        others = {w: bool(torch.equal(ko, keep[k])) for w, k in (("composition", "c"), ("clo_sort per segment", "p")) if k in keep}
        by = 2 * n * (ks + vs) + 4 * m
        V = {v: stats(ms[v]) for v in variants}
        med = V["segsort"]["median_ms"]
        entry = {"leg": name, "number": number, "rows": n, "segments": m, "key_size": ks, "mode": mode, "form": form, "reps": args.reps,
                 "agrees_with_torch": agrees, "baselines_agree": others, "model_bytes": by, "kernel_ms": kernel_ms, "variants": V,
                 "fraction_of_peak_model": round(by / (med * 1e-3) / PEAK, 4),
                 "time_over": {w: round(med / V[w]["median_ms"], 3) for w in variants if w != "segsort"}}
        loses = [w for w in variants if w != "segsort" and med > V[w]["median_ms"]]
        entry["verdict"] = "LOSES to " + " and to ".join("%s (%.2fx)" % (w, entry["time_over"][w]) for w in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in list(bufs.values()) + closing:
            x.close()
        keep.clear()
        del counts, keys, values, off64, src, ko, vo, run

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["agrees_with_torch"] and all(e["baselines_agree"].values()) for e in rec["legs"])
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
