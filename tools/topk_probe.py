"""Measurement probe (not part of the bench contract): top-k against the two things a caller had before it — this
library's argsort (clo_sort_by_key_*) followed by taking the first m rows, and torch.topk — on the same GPU, in one
process, on the same inputs.

Legs, at 2^28 uint32 keys unless noted ("smallest", "input" order, keys and k-th key written, unless noted):
  k in {1, 64, 1024, 2^16, 2^20, 2^24, 2^27} on uniform keys
  all keys equal, 8 distinct keys, ascending and descending keys, at k = 1024 and 2^20
  "largest" at k = 1024; "sorted" order, both directions, at k = 1024
  the arg form (indices alone) and uint32 values at k = 1024
  uint64 keys at k = 1024 and 2^20 (the library has no argsort for them)
  2^24 keys at k = 1024
Every variant of every leg is warmed up first; then the variants alternate, timed with device events on one stream, for
--reps rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the bytes its launches
move (each of the key_size digit sweeps, the count sweep and the apply sweep reads all n keys; the apply sweep reads the
values too and writes the m rows), those bytes per second as a fraction of the 8 TB/s peak, its time over the
sort-and-take's and over torch.topk's, and LOSES where it is slower than either. Then one pass with the library's
per-kernel events: where the time goes. The chosen keys are compared with torch's (as sorted multisets: ties make
torch's choice of rows differ) where m <= 2^20, the k-th key alone above that.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/topk_probe.py [--log2n 28] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("topk_digit", "topk_pick", "topk_count", "topk_scan", "topk_apply", "topk_sort")


def stats(ms):
    t = sorted(ms)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    N = 1 << args.log2n
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "topk_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "digit_bits": 8,
           "tile": {"uint": clo.topk_tile(4, 0), "uint + values": clo.topk_tile(4, 4), "ulong": clo.topk_tile(8, 0)},
           "sorted_max": clo.topk_sorted_max(4, 0), "legs": []}

    # (name, key type, n, distribution, which, order, form, k)
    legs = [("uniform, k=%d" % k, "uint", N, "uniform", "smallest", "input", "keys", k)
            for k in (1, 64, 1024, 1 << 16, 1 << 20, 1 << 24, 1 << 27) if k < N]
    for dist in ("all equal", "8 distinct", "ascending", "descending"):
        legs += [("%s, k=%d" % (dist, k), "uint", N, dist, "smallest", "input", "keys", k) for k in (1024, 1 << 20) if k < N]
    legs += [("largest, k=1024", "uint", N, "uniform", "largest", "input", "keys", 1024),
             ("smallest sorted, k=1024", "uint", N, "uniform", "smallest", "sorted", "keys", 1024),
             ("largest sorted, k=1024", "uint", N, "uniform", "largest", "sorted", "keys", 1024),
             ("arg form, k=1024", "uint", N, "uniform", "smallest", "input", "arg", 1024),
             ("uint32 values, k=1024", "uint", N, "uniform", "smallest", "input", "values", 1024),
             ("uint64 keys, k=1024", "ulong", N, "uniform", "smallest", "input", "keys", 1024)]
    if (1 << 20) < N:
        legs.append(("uint64 keys, k=2^20", "ulong", N, "uniform", "smallest", "input", "keys", 1 << 20))
    if args.log2n > 24:
        legs.append(("2^24 keys, k=1024", "uint", 1 << 24, "uniform", "smallest", "input", "keys", 1024))

    made = {}

    def arrays(kt, n, dist):
        """The leg's input, made once per (key type, n, distribution); non-negative, so that torch's signed order is
        the unsigned one."""
        if (kt, n, dist) not in made:
            made.clear()
            torch.cuda.empty_cache()
            dtype = torch.int32 if kt == "uint" else torch.int64
            g = torch.Generator(device="cuda").manual_seed(n + len(kt))
            top = (1 << 31) if kt == "uint" else (1 << 62)
            if dist == "all equal":
                keys = torch.full((n,), 12345, device="cuda", dtype=dtype)
            elif dist == "8 distinct":
                keys = torch.randint(0, 8, (n,), device="cuda", dtype=dtype, generator=g) * 1000003
            else:
                keys = torch.randint(0, top, (n,), device="cuda", dtype=dtype, generator=g)
                if dist != "uniform":
                    keys = torch.sort(keys, descending=dist == "descending")[0]
            made[(kt, n, dist)] = {"keys": keys, "values": torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)}
        return made[(kt, n, dist)]

    for name, kt, n, dist, which, order, form, k in legs:
        a = arrays(kt, n, dist)
        keys = a["keys"]
        ks = 4 if kt == "uint" else 8
        vs = 0 if form == "keys" else 4
        ko = torch.empty(k, device="cuda", dtype=keys.dtype)
        vo = torch.empty(k, device="cuda", dtype=torch.int32)
        kth = torch.zeros(2, device="cuda", dtype=keys.dtype)
        t = clo.TopK(which, order, ctx, kt, vs)
        bk, bv, bko, bvo, bkth = B(keys), B(a["values"]), B(ko), B(vo), B(kth)
        keep, closing = {}, [t, bk, bv, bko, bvo, bkth]
        run = {"topk": lambda: t.with_device_data(q, bk, bv if form == "values" else None, None if form == "arg" else bko, bvo if vs else None, bkth, n, k)}
        if kt == "uint":   # the argsort exists for keys of up to 4 bytes
            sk, sv = torch.empty_like(keys), torch.empty(n, device="cuda", dtype=torch.int32)
            s, bsk, bsv = clo.Sorter("satradix", ctx, "uint"), B(sk), B(sv)
            closing += [s, bsk, bsv]

            def sort_and_take():
                s.by_key_with_device_data(q, bk, None, bsk, bsv, n)
                keep["s"] = (sk[:k].clone(), sv[:k].clone())
            run["sort and take"] = sort_and_take
        run["torch.topk"] = lambda: keep.__setitem__("t", torch.topk(keys, k, largest=which == "largest", sorted=order == "sorted"))
        variants = tuple(run)
        failed = {}
        for v in variants:   # warm-up: code objects, the objects' scratch, torch's allocator
            try:
                for _ in range(2):
                    run[v]()
                torch.cuda.synchronize()
            except RuntimeError as e:   # torch.topk out of memory at a large k: the leg goes on without it
                failed[v] = str(e).split("\n")[0][:200]
                keep.clear()
                torch.cuda.empty_cache()
        variants = tuple(v for v in variants if v not in failed)
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
            run["topk"]()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        run["topk"]()
        torch.cuda.synchronize()
        agrees = None
        if "torch.topk" in variants:
            tv = keep["t"][0]
            edge = tv.max() if which == "smallest" else tv.min()
            agrees = bool(edge == kth[0])
            if form != "arg" and k <= (1 << 20):
                agrees = agrees and bool(torch.equal(torch.sort(ko)[0], torch.sort(tv)[0]))
            if order == "sorted" and form != "arg":
                agrees = agrees and bool(torch.equal(ko, tv))
        if "sort and take" in variants and which == "smallest":
            same = bool(torch.equal(torch.sort(vo)[0] if order == "input" else vo, torch.sort(keep["s"][1])[0] if order == "input" else keep["s"][1])) if form == "arg" \
                else bool(torch.equal(torch.sort(ko)[0], keep["s"][0]))
            agrees = same if agrees is None else agrees and same
        launches = {"digit sweeps": ks * ks * n, "count": ks * n, "apply": ks * n + (4 * n if form == "values" else 0) + (0 if form == "arg" else ks * k) + vs * k}
        by = sum(launches.values())
        V = {v: stats(ms[v]) for v in variants}
        med = V["topk"]["median_ms"]
        entry = {"leg": name, "keys": kt, "n": n, "distribution": dist, "which": which, "order": order, "form": form, "k": k, "reps": args.reps,
                 "agrees": agrees, "bytes": by, "bytes_per_launch_kind": launches, "kernel_ms": kernel_ms, "variants": V, "not_run": failed,
                 "bytes_per_s": round(by / (med * 1e-3)), "fraction_of_peak": round(by / (med * 1e-3) / PEAK, 3)}
        loses = []
        for other, key in (("sort and take", "time_over_sort_and_take"), ("torch.topk", "time_over_torch_topk")):
            if other in V:
                entry[key] = round(med / V[other]["median_ms"], 3)
                if med > V[other]["median_ms"]:
                    loses.append("to " + other)
        entry["verdict"] = "LOSES " + " and ".join(loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in closing:
            x.close()
        keep.clear()

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
    rec["every_result_agrees"] = all(e["agrees"] is not False for e in rec["legs"])
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
