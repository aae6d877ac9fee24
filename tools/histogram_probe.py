"""Measurement probe (not part of the bench contract): the histogram against torch.bincount and against this library's
own sort-then-reduce route on the same GPU, in one process.

At 2^24, 2^26 and 2^28 uint32 keys, with 256, 4096, L (clo_hip_histogram_lds_bins(4)) and 2^20 bins and four key
distributions (uniform over the bins, all keys equal, 8 distinct keys, 90 % of the keys in one bin) it times,
alternating and with device events on one stream, after warming up every shape:
  count              clo_histogram_with_device_data, values NULL: counts in uint
  sum                the same with uint values summed in uint
  torch_bincount     torch.bincount(keys, minlength=num_bins) (counts only)
  sort_reduce_count  clo_sort_with_device_data (satradix) then clo_reduce_by_key_with_device_data run lengths
  sort_reduce_sum    clo_sort_by_key_with_device_data then clo_reduce_by_key_with_device_data sums
For each it reports the median and the minimum; for the histogram also the bytes it has to read (ks n, plus vs n)
and the share of 8 TB/s they take at the median, the ratios to the other routes and, with 256 bins, the ratio to the
0.222 ms clo_hip_radixw.hip records for the sort's tile histogram of 2^28 keys, scaled to n. The counts are compared with
torch.bincount, the sums with torch's index_add_. Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/histogram_probe.py [--sizes 24,26,28] [--bins 256,4096,L,1048576] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402

PEAK = 8e12
# the sort's private tile histogram: 8-bit digits of 2^28 uint32 keys (clo_hip_radixw.hip), the read-only-stream yardstick
TILEHIST_MS_2P28 = 0.222
VARIANTS = ("count", "sum", "torch_bincount", "sort_reduce_count", "sort_reduce_sum")
DISTRIBUTIONS = ("uniform", "equal", "distinct8", "skew90")


def make_keys(torch, dist, n, nb, g):
    if dist == "uniform":
        return torch.randint(0, nb, (n,), device="cuda", dtype=torch.int32, generator=g)
    if dist == "equal":
        return torch.full((n,), nb // 2, device="cuda", dtype=torch.int32)
    if dist == "distinct8":
        return torch.randint(0, 8, (n,), device="cuda", dtype=torch.int32, generator=g) * (nb // 8)
    if dist == "skew90":
        k = torch.randint(0, nb, (n,), device="cuda", dtype=torch.int32, generator=g)
        k[torch.rand(n, device="cuda", generator=g) < 0.9] = nb // 3
        return k
    raise KeyError(dist)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="24,26,28")
    ap.add_argument("--bins", default="256,4096,L,1048576")
    ap.add_argument("--dists", default=",".join(DISTRIBUTIONS))
    ap.add_argument("--reps", type=int, default=0, help="timed rounds per shape (0: by size)")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for both
    L = clo.histogram_lds_bins(4)
    h_cnt = clo.Histogram(ctx, "uint", None, "uint")
    h_sum = clo.Histogram(ctx, "uint", "uint", "uint")
    sorter = clo.Sorter("satradix", ctx, "uint")
    r_rle = clo.ReduceByKey(ctx, "uint", None, "uint")
    r_sum = clo.ReduceByKey(ctx, "uint", "uint", "uint")
    timer = clo.HipEventTimer(q)
    rec = {"what": "histogram_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "lds_bins": L, "sort_tile_histogram_ms_2p28": TILEHIST_MS_2P28,
           "tile": {"count": clo.histogram_tile(4, 0), "sum": clo.histogram_tile(4, 4)}, "shapes": []}

    for logn in [int(x) for x in args.sizes.split(",")]:
        n = 1 << logn
        B = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
        g = torch.Generator(device="cuda").manual_seed(logn)
        values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        ks, vs, ko, ao = (torch.empty(n, device="cuda", dtype=torch.int32) for _ in range(4))
        cnt = torch.zeros(1, device="cuda", dtype=torch.int64)
        bv, bks, bvs, bko, bao, bc = B(values), B(ks), B(vs), B(ko), B(ao), B(cnt)
        for nb in [L if x == "L" else int(x) for x in args.bins.split(",")]:
            hist = torch.empty(nb, device="cuda", dtype=torch.int32)
            bh = B(hist)
            for dist in args.dists.split(","):
                keys = make_keys(torch, dist, n, nb, g)
                bk = B(keys)
                keep = {}

                def torch_bincount():
                    keep["bc"] = torch.bincount(keys, minlength=nb)

                def sort_reduce_count():
                    sorter.with_device_data(q, bk, bks, n)
                    r_rle.with_device_data(q, bks, None, bko, bao, bc, n)

                def sort_reduce_sum():
                    sorter.by_key_with_device_data(q, bk, bv, bks, bvs, n)
                    r_sum.with_device_data(q, bks, bvs, bko, bao, bc, n)

                run = {
                    "count": lambda: h_cnt.with_device_data(q, bk, None, bh, n, num_bins=nb),
                    "sum": lambda: h_sum.with_device_data(q, bk, bv, bh, n, num_bins=nb),
                    "torch_bincount": torch_bincount,
                    "sort_reduce_count": sort_reduce_count,
                    "sort_reduce_sum": sort_reduce_sum,
                }
                for v in VARIANTS:   # warm-up: code objects, the objects' scratch, torch's allocator
                    for _ in range(2):
                        run[v]()
                torch.cuda.synchronize()
                reps = args.reps or max(5, min(30, (1 << 30) // n))
                ms = {v: [] for v in VARIANTS}
                for r in range(reps):
                    for v in (VARIANTS if r % 2 == 0 else VARIANTS[::-1]):
                        timer.start()
                        run[v]()
                        timer.stop()
                        ms[v].append(timer.elapsed_ms())
                torch.cuda.synchronize()
                # the results agree with torch's
                run["torch_bincount"]()
                run["count"]()
                torch.cuda.synchronize()
                agree = bool(torch.equal(hist.to(torch.int64), keep["bc"]))
                run["sum"]()
                want = torch.zeros(nb, device="cuda", dtype=torch.int64).index_add_(0, keys.to(torch.int64), values.to(torch.int64))
                torch.cuda.synchronize()
                agree = agree and bool(torch.equal(hist.to(torch.int64) & 0xffffffff, want & 0xffffffff))
                del want
                entry = {"log2n": logn, "n": n, "num_bins": nb, "distribution": dist, "reps": reps, "results_agree": agree, "variants": {}}
                for v in VARIANTS:
                    t = sorted(ms[v])
                    med = t[len(t) // 2]
                    e = {"median_ms": round(med, 4), "min_ms": round(t[0], 4)}
                    if v in ("count", "sum"):
                        by = (4 + (4 if v == "sum" else 0)) * n
                        e["bytes"] = by
                        e["share_of_peak"] = round(by / (med * 1e-3) / PEAK, 3)
                    entry["variants"][v] = e
                V = entry["variants"]
                V["count"]["ratio_to_torch_bincount"] = round(V["count"]["median_ms"] / V["torch_bincount"]["median_ms"], 3)
                V["count"]["ratio_to_sort_reduce"] = round(V["count"]["median_ms"] / V["sort_reduce_count"]["median_ms"], 3)
                V["sum"]["ratio_to_sort_reduce"] = round(V["sum"]["median_ms"] / V["sort_reduce_sum"]["median_ms"], 3)
                if nb == 256:   # against the yardstick scaled to n (it streams: time ~ bytes)
                    V["count"]["ratio_to_sort_tile_histogram"] = round(V["count"]["median_ms"] / (TILEHIST_MS_2P28 * n / (1 << 28)), 3)
                entry["faster_than_sort_reduce"] = bool(V["count"]["median_ms"] < V["sort_reduce_count"]["median_ms"]
                                                        and V["sum"]["median_ms"] < V["sort_reduce_sum"]["median_ms"])
                rec["shapes"].append(entry)
                print(json.dumps(entry), flush=True)
                bk.close()
                keep.clear()
                del keys
            bh.close()
            del hist
        for b in (bv, bks, bvs, bko, bao, bc):
            b.close()
        del values, ks, vs, ko, ao, cnt
        torch.cuda.empty_cache()

    rec["every_shape_faster_than_sort_reduce"] = all(s["faster_than_sort_reduce"] for s in rec["shapes"])
    rec["every_result_agrees"] = all(s["results_agree"] for s in rec["shapes"])
    timer.close()
    for o in (h_cnt, h_sum, sorter, r_rle, r_sum):
        o.close()
    q.close()
    ctx.close()
    text = json.dumps(rec)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
