"""Measurement probe (not part of the bench contract): the merge of two sorted arrays against sorting their
concatenation again, with this library's own sort and with torch's, on the same GPU in one process.

Legs: 2^27 + 2^27 uint32 keys with the inputs uniform, all equal, and A entirely below B, each as keys only, with uint32
values and as argmerge; 2^27 + 2^20 (a small batch into a large table) in the same three modes; 2^27 + 2^27 uint64 keys,
keys only. Every leg times, alternating and with device events on one stream, after warming up every shape:
  merge        clo_merge_with_device_data
  resort       clo_sort_by_key_with_device_data (satradix) on the concatenation, built beforehand: values given, or NULL
               (index) for the argmerge and the keys-only legs; not for uint64 keys, which the by-key sort does not take
  plain_sort   clo_sort_with_device_data on the concatenation (keys-only legs)
  torch_sort   torch.sort(torch.cat((a, b)), stable=True) (keys and indices)
For each it reports the median and the minimum; for the merge also the bytes it has to move (every key read and
written once, values likewise, the permutation written) and the share of 8 TB/s they take at the median, and the ratios
merge / resort, merge / plain_sort and merge / torch_sort. The merge's output is compared with the re-sort's. Prints one
JSON record (and writes it to --out).
Usage on the GPU machine: python tools/merge_probe.py [--log2n 27] [--log2small 20] [--reps 10] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402

PEAK = 8e12
MODES = ("keys", "values", "argmerge")


def make_inputs(torch, dist, na, nb, dtype, g):
    """Two ascending arrays of non-negative keys (so that torch's signed order is the unsigned one)."""
    top = (1 << 31) - 1 if dtype == torch.int32 else (1 << 62)
    if dist == "uniform":
        a = torch.sort(torch.randint(0, top, (na,), device="cuda", dtype=dtype, generator=g)).values
        b = torch.sort(torch.randint(0, top, (nb,), device="cuda", dtype=dtype, generator=g)).values
    elif dist == "equal":
        a, b = torch.full((na,), 12345, device="cuda", dtype=dtype), torch.full((nb,), 12345, device="cuda", dtype=dtype)
    elif dist == "a_below_b":
        a = torch.arange(na, device="cuda", dtype=dtype)
        b = torch.arange(nb, device="cuda", dtype=dtype) + na
    else:
        raise KeyError(dist)
    return a, b


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--log2small", type=int, default=20)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    N, S = 1 << args.log2n, 1 << args.log2small
    legs = [("uint", dist, N, N, MODES) for dist in ("uniform", "equal", "a_below_b")]
    legs += [("uint", "uniform", N, S, MODES), ("ulong", "uniform", N, N, ("keys",))]
    rec = {"what": "merge_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK,
           "tile": {"uint": clo.merge_tile(4, 4), "ulong": clo.merge_tile(8, 0)}, "legs": []}
    B = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())

    for kt, dist, na, nb, modes in legs:
        dtype, ks = (torch.int32, 4) if kt == "uint" else (torch.int64, 8)
        n = na + nb
        g = torch.Generator(device="cuda").manual_seed(na + nb)
        a, b = make_inputs(torch, dist, na, nb, dtype, g)
        values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        cat = torch.cat((a, b))
        mk, sk = torch.empty(n, device="cuda", dtype=dtype), torch.empty(n, device="cuda", dtype=dtype)
        mv, sv = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.int32)
        ba, bb, bcat, bmk, bsk, bmv, bsv = B(a), B(b), B(cat), B(mk), B(sk), B(mv), B(sv)
        bva, bvb, bval = B(values[:na]), B(values[na:]), B(values)
        sorter = clo.Sorter("satradix", ctx, kt)
        for mode in modes:
            vs = 0 if mode == "keys" else 4
            merger = clo.Merge(ctx, kt, vs)
            valued = mode == "values"
            keep = {}

            def torch_sort():
                keep["t"] = torch.sort(torch.cat((a, b)), stable=True)

            run = {"merge": lambda: merger.with_device_data(q, ba, bva if valued else None, na, bb, bvb if valued else None, nb,
                                                            bmk, bmv if vs else None),
                   "torch_sort": torch_sort}
            if ks == 4:
                run["resort"] = lambda: sorter.by_key_with_device_data(q, bcat, bval if valued else None, bsk, bsv, n)
            if mode == "keys":
                run["plain_sort"] = lambda: sorter.with_device_data(q, bcat, bsk, n)
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
            # the merge gives what sorting the concatenation gives
            run["resort" if ks == 4 else "plain_sort"]()
            run["merge"]()
            torch.cuda.synchronize()
            agree = bool(torch.equal(mk, sk)) and (vs == 0 or bool(torch.equal(mv, sv)))
            by = 2 * n * ks + (2 * n * 4 if valued else n * 4 if vs else 0)
            entry = {"keys": kt, "distribution": dist, "numel_a": na, "numel_b": nb, "mode": mode, "reps": args.reps,
                     "result_agrees": agree, "bytes": by, "variants": {}}
            for v in variants:
                t = sorted(ms[v])
                entry["variants"][v] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4)}
            V = entry["variants"]
            med = V["merge"]["median_ms"]
            V["merge"]["share_of_peak"] = round(by / (med * 1e-3) / PEAK, 3)
            for v in variants[1:]:
                V["merge"]["ratio_to_" + v] = round(med / V[v]["median_ms"], 3)
            entry["faster_than_resort"] = all(med < V[v]["median_ms"] for v in variants if v in ("resort", "plain_sort"))
            rec["legs"].append(entry)
            print(json.dumps(entry), flush=True)
            merger.close()
            keep.clear()
        sorter.close()
        for x in (ba, bb, bcat, bmk, bsk, bmv, bsv, bva, bvb, bval):
            x.close()
        del a, b, values, cat, mk, sk, mv, sv
        torch.cuda.empty_cache()

    rec["every_leg_faster_than_resort"] = all(e["faster_than_resort"] for e in rec["legs"])
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
