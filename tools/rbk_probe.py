"""Measurement probe (not part of the bench contract): reduce by key against torch on the same GPU, in one process.

At 2^24, 2^26 and 2^28 uint32 keys with mean run lengths of 1, 16 and 4096 it times, alternating and with device
events on one stream, after warming up every shape:
  sum           clo_reduce_by_key_with_device_data: uint values summed in uint, keys_out and aggr_out written
  rle           values NULL: the run lengths (uint), keys_out written
  unique        keys_out alone
  torch_rle     torch.unique_consecutive(keys, return_counts=True)
  torch_sum     torch.unique_consecutive(keys, return_inverse=True) and index_add_ of the values
For each it reports the median and the minimum; for the library's variants also the bytes the three-launch schedule
moves (two reads of the inputs, the rows written, the tile states written, scanned in place and read again) and
the share of 8 TB/s those bytes take at the median. The library's results are compared with torch's. Prints one
JSON record (and writes it to --out).
Usage on the GPU machine: python tools/rbk_probe.py [--sizes 24,26,28] [--runs 1,16,4096] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402

PEAK = 8e12
VARIANTS = ("sum", "rle", "unique", "torch_rle", "torch_sum")


def schedule_bytes(n, m, variant, tile):
    ks = 4
    vs = 4 if variant == "sum" else 0
    ss = 0 if variant == "unique" else 4
    tiles = (n + tile - 1) // tile
    state = 4 + (4 if ss else 0)
    return 2 * (ks + vs) * n + (ks + ss) * m + 4 * state * tiles


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="24,26,28")
    ap.add_argument("--runs", default="1,16,4096")
    ap.add_argument("--reps", type=int, default=0, help="timed rounds per shape (0: by size)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for both
    r_sum = clo.ReduceByKey(ctx, "uint", "uint", "uint")
    r_rle = clo.ReduceByKey(ctx, "uint", None, "uint")
    timer = clo.HipEventTimer(q)
    rec = {"what": "rbk_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "shapes": []}

    for logn in [int(x) for x in args.sizes.split(",")]:
        n = 1 << logn
        for mean in [int(x) for x in args.runs.split(",")]:
            g = torch.Generator(device="cuda").manual_seed(logn * 100003 + mean)
            if mean == 1:
                keys = torch.arange(n, device="cuda", dtype=torch.int32)
            else:
                heads = torch.rand(n, device="cuda", generator=g) < 1.0 / mean
                keys = torch.cumsum(heads, 0, dtype=torch.int32)
                del heads
            values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
            ko, ao = torch.empty_like(keys), torch.empty_like(values)
            cnt = torch.zeros(1, device="cuda", dtype=torch.int64)
            torch.cuda.synchronize()
            B = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
            bk, bv, bko, bao, bc = B(keys), B(values), B(ko), B(ao), B(cnt)
            keep = {}

            def torch_rle():
                keep["rle"] = torch.unique_consecutive(keys, return_counts=True)

            def torch_sum():
                u, inv = torch.unique_consecutive(keys, return_inverse=True)
                keep["sum"] = (u, torch.zeros(u.numel(), device="cuda", dtype=torch.int32).index_add_(0, inv, values))

            run = {
                "sum": lambda: r_sum.with_device_data(q, bk, bv, bko, bao, bc, n),
                "rle": lambda: r_rle.with_device_data(q, bk, None, bko, bao, bc, n),
                "unique": lambda: r_rle.with_device_data(q, bk, None, bko, None, bc, n),
                "torch_rle": torch_rle,
                "torch_sum": torch_sum,
            }
            for v in VARIANTS:   # warm-up: code objects, the objects' scratch, torch's allocator
                for _ in range(2):
                    run[v]()
            torch.cuda.synchronize()
            reps = args.reps or max(5, min(40, (1 << 30) // n))
            ms = {v: [] for v in VARIANTS}
            for r in range(reps):
                for v in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
                    timer.start()
                    run[v]()
                    timer.stop()
                    ms[v].append(timer.elapsed_ms())
            torch.cuda.synchronize()
            # the results agree with torch's
            run["torch_rle"]()
            run["torch_sum"]()
            run["rle"]()
            torch.cuda.synchronize()
            m = int(cnt.item())
            u, c = keep["rle"]
            agree = bool(m == u.numel() and torch.equal(ko[:m], u) and torch.equal(ao[:m], c.to(torch.int32)))
            run["sum"]()
            torch.cuda.synchronize()
            agree = agree and bool(int(cnt.item()) == m and torch.equal(ko[:m], keep["sum"][0]) and torch.equal(ao[:m], keep["sum"][1]))
            tile = clo.reduce_by_key_tile(4, 4)
            entry = {"log2n": logn, "n": n, "mean_run": mean, "runs": m, "reps": reps, "results_agree": agree, "variants": {}}
            for v in VARIANTS:
                t = sorted(ms[v])
                med = t[len(t) // 2]
                e = {"median_ms": round(med, 4), "min_ms": round(t[0], 4)}
                if not v.startswith("torch"):
                    by = schedule_bytes(n, m, v, clo.reduce_by_key_tile(4, 4 if v == "sum" else 0))
                    e["bytes"] = by
                    e["share_of_peak"] = round(by / (med * 1e-3) / PEAK, 3)
                entry["variants"][v] = e
            entry["variants"]["rle"]["ratio_to_torch"] = round(entry["variants"]["rle"]["median_ms"] / entry["variants"]["torch_rle"]["median_ms"], 3)
            entry["variants"]["sum"]["ratio_to_torch"] = round(entry["variants"]["sum"]["median_ms"] / entry["variants"]["torch_sum"]["median_ms"], 3)
            entry["tile"] = tile
            rec["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
            for b in (bk, bv, bko, bao, bc):
                b.close()
            keep.clear()
            del keys, values, ko, ao, cnt, u, c
            torch.cuda.empty_cache()

    timer.close()
    r_sum.close()
    r_rle.close()
    q.close()
    ctx.close()
    text = json.dumps(rec)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
