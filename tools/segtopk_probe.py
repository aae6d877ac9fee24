"""Measurement probe (not part of the bench contract): CloSegTopK against what a caller had before, on the same inputs,
on the same GPU, in one process:
  (a) the composition: CloSegSort of all rows, CloExpand's ranks, CloSelect on rank < k with the sorted keys as values;
      the whole chain is timed. Its output is compacted (CSR), which is the dense output's written slots in order.
  (b) CloSegArg ("first") on the k = 1 leg.
  (c) CloTopK (order "sorted") on the single-segment leg.
  (d) torch alone, on one leg: a stable sort of the packed (id << 32 | key) and the slicing by rank < k.

Legs, at 2^28 uint32 rows unless noted, uint32 counts, "smallest", keys below 2^31:
  mean length 16 with k 2, 4 and 16; mean length 256 with k 16; 2^20 rows per segment with k 16 and 1024; a single segment
  with k 64; mean length 1 with k 1; half of the segments empty; uint32 values; the arg form; uint64 keys; the offsets
  form; 2^24 rows
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for 10 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the model's bytes
n key_size + m count_size + written rows (key_size + value_size) + 4 m as a fraction of the 8 TB/s peak, and its time
over the baselines'; LOSES where it is slower than one. Every output is compared with the baselines'. Then one pass with
the library's per-kernel events: where the time goes.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/segtopk_probe.py [--log2n 28] [--reps 10] [--out FILE] [--legs a,b]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("segtopk_sums", "segtopk_sums_scan", "segtopk_ends", "segtopk_zero", "segtopk_heads", "segtopk_tile", "segtopk_combine")


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
    T, cap = clo.segtopk_tile(4, 0), clo.segtopk_k_max(4, 0)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "segtopk_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": T, "k_max": cap, "legs": []}
    g = torch.Generator(device="cuda").manual_seed(28)

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

    big = min(1 << 20, N // 4)
    # (name, rows, counts kind, k, key size, mode, form, the torch baseline too); mode: keys, v4 or arg
    legs = [("mean length 16, k = %d" % k, N, "mean 16", k, 4, "keys", "counts", k == 4) for k in (2, 4, 16)]
    legs += [("mean length 256, k = 16", N, "mean 256", 16, 4, "keys", "counts", False),
             ("%d rows in every segment, k = 16" % big, N, "equal %d" % big, 16, 4, "keys", "counts", False),
             ("%d rows in every segment, k = %d" % (big, cap), N, "equal %d" % big, cap, 4, "keys", "counts", False),
             ("a single segment, k = 64", N, "single", 64, 4, "keys", "counts", False),
             ("mean length 1, k = 1", N, "mean 1", 1, 4, "arg", "counts", False),
             ("half of the segments empty, mean length 16, k = 4", N, "half empty mean 16", 4, 4, "keys", "counts", False),
             ("uint32 values, mean length 16, k = 4", N, "mean 16", 4, 4, "v4", "counts", False),
             ("the arg form, mean length 16, k = 4", N, "mean 16", 4, 4, "arg", "counts", False),
             ("uint64 keys, mean length 16, k = 4", N, "mean 16", 4, 8, "keys", "counts", False),
             ("the offsets form, mean length 16, k = 4", N, "mean 16", 4, 4, "keys", "offsets", False)]
    if args.log2n > 24:
        legs.append(("2^24 rows, mean length 16, k = 4", 1 << 24, "mean 16", 4, 4, "keys", "counts", False))
    want = {int(x) for x in args.legs.split(",") if x} if args.legs else None

    for number, (name, n, kind, k, ks, mode, form, with_torch) in enumerate(legs):
        if want is not None and number not in want:
            continue
        torch.cuda.empty_cache()
        counts = counts_for(kind, n)
        m = counts.numel()
        assert int(counts.sum(dtype=torch.int64)) == n
        kdt = torch.int64 if ks == 8 else torch.int32
        kt = "ulong" if ks == 8 else "uint"
        keys = torch.randint(0, 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g).to(kdt)
        if ks == 8:
            keys = keys * 2654435761 + 12345                                                    # above 2^32, still positive
        vs = 0 if mode == "keys" else 4
        values = torch.randint(0, 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g) if mode == "v4" else None
        off64 = torch.cat((torch.zeros(1, dtype=torch.int64, device="cuda"), torch.cumsum(counts, 0, dtype=torch.int64)))
        src = off64.to(torch.int32) if form == "offsets" else counts
        ko = torch.full((m * k,), -1, device="cuda", dtype=kdt)
        vo = torch.full((m * k if vs else 2,), -1, device="cuda", dtype=torch.int32)
        co = torch.zeros(m, device="cuda", dtype=torch.int32)
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        st = clo.SegTopK("smallest", form, ctx, kt, vs, "uint")
        bufs = {x: B(t) for x, t in (("src", src), ("keys", keys), ("ko", ko), ("vo", vo), ("co", co), ("num", num), ("counts", counts))}
        if values is not None:
            bufs["values"] = B(values)
        keep = {}
        closing = [st]

        def segtopk():
            st.with_device_data(q, bufs["src"], None, bufs["keys"], bufs.get("values"), bufs["ko"], bufs["vo"] if vs else None, bufs["co"], bufs["num"],
                                m, n, k)

        # (a) sort every segment, rank every row, keep rank < k; the sorted keys travel as the select's values. With
        # values or in the arg form the select carries those instead (the keys would take a second select).
        ss, ex, sel = clo.SegSort(form, ctx, kt, vs, "uint"), clo.Expand("counts", ctx, None, "uint"), clo.Select("select", "lt", ctx, "uint", 4 if ks == 4 else 8)
        sk = torch.empty(n, device="cuda", dtype=kdt)
        sv = torch.empty(n if vs else 2, device="cuda", dtype=torch.int32)
        rank, rank_o = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.int32)
        picked = torch.empty(n, device="cuda", dtype=kdt if not vs else torch.int32)
        thr = torch.tensor([k, 0], dtype=torch.int32, device="cuda")
        nums = torch.zeros(6, device="cuda", dtype=torch.int64)
        bufs.update(sk=B(sk), sv=B(sv), rank=B(rank), rank_o=B(rank_o), picked=B(picked), thr=B(thr), n1=B(nums[0:2]), n2=B(nums[2:4]), n3=B(nums[4:6]))
        closing += [ss, ex, sel]

        def composition():
            ss.with_device_data(q, bufs["src"], None, bufs["keys"], bufs.get("values"), bufs["sk"], bufs["sv"] if vs else None, bufs["n1"], m, n)
            ex.with_device_data(q, bufs["counts"], None, None, None, None, bufs["rank"], bufs["n2"], m, n)
            sel.with_device_data(q, bufs["rank"], bufs["sv"] if vs else bufs["sk"], bufs["thr"], bufs["rank_o"], bufs["picked"], bufs["n3"], n)

        run = {"segtopk": segtopk, "composition": composition}
        if k == 1:
            sa = clo.SegArg("argmin", "first", "counts", ctx, kt, "uint")
            ai, av = torch.empty(m, device="cuda", dtype=torch.int32), torch.empty(m, device="cuda", dtype=kdt)
            bufs.update(ai=B(ai), av=B(av), n4=B(torch.zeros(2, device="cuda", dtype=torch.int64)))
            closing.append(sa)
            run["segarg"] = lambda: sa.with_device_data(q, bufs["counts"], None, bufs["keys"], bufs["ai"], bufs["av"], bufs["n4"], m, n)
        if kind == "single":
            tp = clo.TopK("smallest", "sorted", ctx, kt, 0)
            tk = torch.empty(k, device="cuda", dtype=kdt)
            bufs.update(tk=B(tk))
            closing.append(tp)
            run["topk"] = lambda: tp.with_device_data(q, bufs["keys"], None, bufs["tk"], None, None, n, k)
        if with_torch:
            def torch_leg():
                ids = torch.repeat_interleave(torch.arange(m, device="cuda", dtype=torch.int64), counts, output_size=n)
                s = torch.sort((ids << 32) | keys.to(torch.int64), stable=True)[0]
                r = torch.arange(n, device="cuda", dtype=torch.int64) - off64[:-1][ids]
                keep["t"] = (s[r < k] & 0xffffffff).to(torch.int32)
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
            segtopk()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        num.fill_(-1)
        ko.fill_(-1)
        for v in variants:
            run[v]()
        torch.cuda.synchronize()
        written = torch.arange(k, device="cuda", dtype=torch.int32)[None, :] < co[:, None]     # the slots the call wrote, in order
        rows = int(co.sum(dtype=torch.int64))
        mine = (vo if vs else ko).view(m, k)[written]
        agrees = {"num_out": int(num[0].item()) == n, "counts_out": bool(torch.equal(co, torch.clamp(counts, max=k))),
                  "composition": int(nums[4].item()) == rows and bool(torch.equal(mine, picked[:rows]))}
        if "segarg" in run:
            agrees["segarg"] = bool(torch.equal(vo.view(m, k)[:, 0][counts > 0], ai[counts > 0]))
        if "topk" in run:
            agrees["topk"] = bool(torch.equal(ko[:k], tk))
        if "t" in keep:
            agrees["torch"] = bool(torch.equal(ko.view(m, k)[written], keep["t"]))
        by = n * ks + 4 * m + rows * (ks + vs) + 4 * m
        V = {v: stats(ms[v]) for v in variants}
        med = V["segtopk"]["median_ms"]
        entry = {"leg": name, "number": number, "rows": n, "segments": m, "k": k, "key_size": ks, "mode": mode, "form": form, "reps": args.reps,
                 "rows_written": rows, "agrees": agrees, "model_bytes": by, "kernel_ms": kernel_ms, "variants": V,
                 "fraction_of_peak_model": round(by / (med * 1e-3) / PEAK, 4),
                 "time_over": {w: round(med / V[w]["median_ms"], 3) for w in variants if w != "segtopk"}}
        loses = [w for w in variants if w != "segtopk" and med > V[w]["median_ms"]]
        entry["verdict"] = "LOSES to " + " and to ".join("%s (%.2fx)" % (w, entry["time_over"][w]) for w in loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in list(bufs.values()) + closing:
            x.close()
        keep.clear()
        del counts, keys, values, off64, src, ko, vo, co, run, sk, sv, rank, rank_o, picked, written, mine

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(all(e["agrees"].values()) for e in rec["legs"])
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
