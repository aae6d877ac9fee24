"""Measurement probe (not part of the bench contract): scan by key against reduce by key and torch on the same GPU,
on the same input, in one process.

At 2^24, 2^26 and 2^28 uint32 keys with mean run lengths of 1, 16 and 4096 it times, alternating and with device
events on one stream, after warming up every shape:
  sum           clo_scan_by_key_with_device_data: exclusive sum of uint values in uint
  rank          values NULL: the exclusive sum of ones, the element's rank in its run (uint)
  max           inclusive max of uint values in uint
  rbk_sum       clo_reduce_by_key_with_device_data: uint values summed in uint, keys_out and aggr_out written (the same
                two reads of the inputs; it writes (ks + ss) m bytes where the scan by key writes ss n)
  torch_sum     torch.cumsum of the values (int32, and in int64 for comparison) minus the gathered cumsum at each run's
                head, the heads from torch.unique_consecutive(return_inverse=True)
For each it reports the median and the minimum; for the library's variants also the bytes the three-launch schedule
moves (two reads of the inputs, the results written, the tile states written, scanned in place and read again) and
the share of 8 TB/s those bytes take at the median. Neither yardstick is the code under test. The library's exclusive
sum is compared with torch's. Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/sbk_probe.py [--sizes 24,26,28] [--runs 1,16,4096] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402

PEAK = 8e12
VARIANTS = ("sum", "rank", "max", "rbk_sum", "torch_sum", "torch_sum64")


def schedule_bytes(n, m, variant, tile):
    """What the three launches move: both sweeps read keys (and values); scan by key writes a result per element,
    reduce by key a row per run; a tile state is 4 + 4 bytes, written, read and written by the state scan, and read."""
    ks, ss = 4, 4
    vs = 0 if variant == "rank" else 4
    tiles = (n + tile - 1) // tile
    out = (ks + ss) * m if variant == "rbk_sum" else ss * n
    return 2 * (ks + vs) * n + out + 4 * 8 * tiles


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
    s_sum = clo.ScanByKey(ctx, "uint", "uint", "uint")
    s_rank = clo.ScanByKey(ctx, "uint", None, "uint")
    s_max = clo.ScanByKey(ctx, "uint", "uint", "uint", op="max", inclusive=True)
    r_sum = clo.ReduceByKey(ctx, "uint", "uint", "uint")
    timer = clo.HipEventTimer(q)
    rec = {"what": "sbk_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "shapes": []}

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
            out, ko, ao = torch.empty_like(values), torch.empty_like(keys), torch.empty_like(values)
            cnt = torch.zeros(1, device="cuda", dtype=torch.int64)
            torch.cuda.synchronize()
            B = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
            bk, bv, bo, bko, bao, bc = B(keys), B(values), B(out), B(ko), B(ao), B(cnt)
            keep = {}

            def torch_sum(dtype):
                # exclusive: the inclusive cumsum minus the value, minus what the cumsum held before the run's head
                u, inv = torch.unique_consecutive(keys, return_inverse=True)
                c = torch.cumsum(values, 0, dtype=dtype)
                head = torch.ones(n, device="cuda", dtype=torch.bool)
                head[1:] = inv[1:] != inv[:-1]
                at = torch.nonzero(head).squeeze(1)
                base = (c[at] - values[at].to(dtype))
                keep[dtype] = c - values.to(dtype) - base[inv]

            run = {
                "sum": lambda: s_sum.with_device_data(q, bk, bv, bo, n),
                "rank": lambda: s_rank.with_device_data(q, bk, None, bo, n),
                "max": lambda: s_max.with_device_data(q, bk, bv, bo, n),
                "rbk_sum": lambda: r_sum.with_device_data(q, bk, bv, bko, bao, bc, n),
                "torch_sum": lambda: torch_sum(torch.int32),
                "torch_sum64": lambda: torch_sum(torch.int64),
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
            # the exclusive sums agree with torch's (both wrap in 32 bits; the 64-bit one in its low word)
            run["torch_sum"]()
            run["torch_sum64"]()
            run["rbk_sum"]()
            run["sum"]()
            torch.cuda.synchronize()
            m = int(cnt.item())
            agree = bool(torch.equal(out, keep[torch.int32]) and torch.equal(out, keep[torch.int64].to(torch.int32)))
            tile = clo.scan_by_key_tile(4, 4)
            entry = {"log2n": logn, "n": n, "mean_run": mean, "runs": m, "reps": reps, "results_agree": agree, "tile": tile, "variants": {}}
            for v in VARIANTS:
                t = sorted(ms[v])
                med = t[len(t) // 2]
                e = {"median_ms": round(med, 4), "min_ms": round(t[0], 4)}
                if not v.startswith("torch"):
                    by = schedule_bytes(n, m, v, clo.scan_by_key_tile(4, 0 if v == "rank" else 4))
                    e["bytes"] = by
                    e["share_of_peak"] = round(by / (med * 1e-3) / PEAK, 3)
                entry["variants"][v] = e
            V = entry["variants"]
            V["sum"]["ratio_to_rbk_sum"] = round(V["sum"]["median_ms"] / V["rbk_sum"]["median_ms"], 3)
            # the expectation from bytes alone: reduce by key's time plus ss n bytes at the 3.4 TB/s its apply sweep reached
            V["sum"]["expected_from_bytes_ms"] = round(V["rbk_sum"]["median_ms"] + 4 * n / 3.4e12 * 1e3, 4)
            V["sum"]["ratio_to_torch"] = round(V["sum"]["median_ms"] / V["torch_sum"]["median_ms"], 3)
            rec["shapes"].append(entry)
            print(json.dumps(entry), flush=True)
            for b in (bk, bv, bo, bko, bao, bc):
                b.close()
            keep.clear()
            del keys, values, out, ko, ao, cnt
            torch.cuda.empty_cache()

    timer.close()
    for x in (s_sum, s_rank, s_max, r_sum):
        x.close()
    q.close()
    ctx.close()
    text = json.dumps(rec)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
