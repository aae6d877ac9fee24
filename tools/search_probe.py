"""Measurement probe (not part of the bench contract): lower bounds of many needles in a sorted haystack, this
library's two paths against torch.searchsorted on the same data, on the same GPU in one process.

Legs: a haystack of 2^28 uniform uint32 keys with 2^20, 2^24 and 2^27 uniform needles; the same haystack all equal
(2^24 needles); 2^24 needles of which 90 % are one key; 2^27 uint64 keys with 2^24 needles. Every leg times,
alternating and with device events on one stream, after warming up every shape:
  general_unsorted   clo_search_with_device_data, no flag, the needles as drawn
  general_sorted     the same call on the needles sorted beforehand (still no flag)
  flag_sorted        CLO_SEARCH_NEEDLES_SORTED on the sorted needles
  torch_unsorted     torch.searchsorted(haystack, needles, out_int32=True)
  torch_sorted       the same on the sorted needles
Keys are non-negative and handed to torch as int32 / int64, so that its signed order is the unsigned one. For each
variant it reports the median and the minimum; for this library's also the bytes of the form's floor (needles read,
positions written, and the haystack keys a search can touch, each once: min(numel_h, numel_n * ceil(log2 numel_h))
keys; 2 ceil(log2 numel_h) for the all-equal haystack, where every search goes all the way left or all the way right)
as a share of 8 TB/s at the median, and the ratio to torch on the same needles. Every output is compared with
torch's. Prints one JSON record per leg and one for all (also written to --out).
Usage on the GPU machine: python tools/search_probe.py [--log2h 28] [--reps 10] [--out FILE]"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402

PEAK = 8e12


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2h", type=int, default=28)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    H = 1 << args.log2h
    small, mid, large = 1 << max(args.log2h - 8, 4), 1 << max(args.log2h - 4, 4), 1 << (args.log2h - 1)
    legs = [("uint", "uniform", H, n, "uniform") for n in (small, mid, large)]
    legs += [("uint", "equal", H, mid, "uniform"), ("uint", "uniform", H, mid, "90% one key"), ("ulong", "uniform", H >> 1, mid, "uniform")]
    rec = {"what": "search_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK,
           "tile": clo.search_tile(4), "lds_keys": clo.search_lds_keys(4), "pivots": clo.search_pivots(4), "legs": []}
    B = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())

    for kt, hdist, nh, nn, ndist in legs:
        dtype, ks = (torch.int32, 4) if kt == "uint" else (torch.int64, 8)
        top = (1 << 31) - 1 if ks == 4 else (1 << 62)
        g = torch.Generator(device="cuda").manual_seed(nh + nn)
        if hdist == "uniform":
            hay = torch.sort(torch.randint(0, top, (nh,), device="cuda", dtype=dtype, generator=g)).values
        else:
            hay = torch.full((nh,), top // 2, device="cuda", dtype=dtype)
        ndl = torch.randint(0, top, (nn,), device="cuda", dtype=dtype, generator=g)
        if ndist != "uniform":
            ndl[torch.rand(nn, device="cuda", generator=g) < 0.9] = hay[nh // 3]
        ndl_sorted = torch.sort(ndl).values
        pos = {v: torch.empty(nn, device="cuda", dtype=torch.int32) for v in ("general_unsorted", "general_sorted", "flag_sorted")}
        bh, bn, bs = B(hay), B(ndl), B(ndl_sorted)
        bp = {v: B(t) for v, t in pos.items()}
        s = clo.Search(ctx, kt)
        keep = {}

        def torch_run(name, x):
            def run():
                keep[name] = torch.searchsorted(hay, x, out_int32=True)
            return run

        run = {"general_unsorted": lambda: s.with_device_data(q, bh, nh, bn, nn, bp["general_unsorted"]),
               "general_sorted": lambda: s.with_device_data(q, bh, nh, bs, nn, bp["general_sorted"]),
               "flag_sorted": lambda: s.with_device_data(q, bh, nh, bs, nn, bp["flag_sorted"], needles_sorted=True),
               "torch_unsorted": torch_run("torch_unsorted", ndl), "torch_sorted": torch_run("torch_sorted", ndl_sorted)}
        variants = tuple(run)
        for v in variants:   # warm-up: code objects, the object's workspace, torch's allocator
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
        agree = (bool(torch.equal(pos["general_unsorted"], keep["torch_unsorted"])) and bool(torch.equal(pos["general_sorted"], keep["torch_sorted"]))
                 and bool(torch.equal(pos["flag_sorted"], keep["torch_sorted"])))
        steps = max(1, math.ceil(math.log2(nh)))
        touched = 2 * steps if hdist == "equal" else min(nh, nn * steps)
        by = nn * ks + nn * 4 + touched * ks
        entry = {"keys": kt, "haystack": hdist, "needles": ndist, "numel_h": nh, "numel_n": nn, "reps": args.reps,
                 "result_agrees": agree, "floor_bytes": by, "variants": {}}
        for v in variants:
            t = sorted(ms[v])
            entry["variants"][v] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4)}
        V = entry["variants"]
        for v, ref in (("general_unsorted", "torch_unsorted"), ("general_sorted", "torch_sorted"), ("flag_sorted", "torch_sorted")):
            V[v]["share_of_peak"] = round(by / (V[v]["median_ms"] * 1e-3) / PEAK, 4)
            V[v]["ratio_to_torch"] = round(V[v]["median_ms"] / V[ref]["median_ms"], 3)
        entry["flag_over_general_on_sorted"] = round(V["flag_sorted"]["median_ms"] / V["general_sorted"]["median_ms"], 3)
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        s.close()
        keep.clear()
        for x in [bh, bn, bs] + list(bp.values()):
            x.close()
        del hay, ndl, ndl_sorted, pos
        torch.cuda.empty_cache()

    rec["every_result_agrees"] = all(e["result_agrees"] for e in rec["legs"])
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
