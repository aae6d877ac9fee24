"""Measurement probe (not part of the bench contract): the set operations on two sorted arrays against the merge of
the same inputs and against what a user would write in torch today, on the same GPU in one process.

Legs: 2^27 + 2^27 uint32 keys with the inputs uniform (strictly ascending with random gaps of 1 to 15, so duplicate-free
and about one key in eight shared), all equal, disjoint (A entirely below B) and A == B: every op keys only, and the
union also with uint32 values and in the arg form; a batch of 2^20 against a table of 2^27 (A is the batch), every op;
2^27 + 2^27 uint64 keys, every op. Every leg times, alternating and with device events on one stream, after warming up:
  setop   clo_setop_with_device_data
  merge   clo_merge_with_device_data on the same inputs in the same mode
  torch   on duplicate-free inputs only: torch.unique_consecutive(torch.sort(torch.cat((a, b))).values) for the union,
          a[torch.isin(a, b)] for the intersection, a[~torch.isin(a, b)] for the difference
For each it reports the median, the minimum and the spread (max - min) / median; the bytes the schedule moves (keys
read twice: once to count, once to apply; values read once; k rows written) over the merge's (everything read once, n
rows written); the time over the merge's; whether the time ratio exceeds the byte ratio by more than the leg's spread;
LOSES where the leg is slower than the torch composition; and the time of each kernel of both (the library's per-kernel
events, a pass of its own). k is compared with torch's where torch ran.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/setop_probe.py [--log2n 27] [--log2small 20] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

OPS = ("union", "intersection", "difference", "symmetric_difference")


def ascending(torch, n, dtype, g, first=0):
    """n strictly ascending keys with gaps of 1 to 15."""
    return torch.cumsum(torch.randint(1, 16, (n,), device="cuda", dtype=dtype, generator=g), 0, dtype=dtype) + first


def make_inputs(torch, dist, na, nb, dtype, g):
    """Two ascending arrays of non-negative keys (so that torch's signed order is the unsigned one)."""
    if dist == "uniform":
        return ascending(torch, na, dtype, g), ascending(torch, nb, dtype, g)
    if dist == "batch":   # the batch's keys span the table's range
        b = ascending(torch, nb, dtype, g)
        return torch.sort(torch.randint(0, 8 * nb, (na,), device="cuda", dtype=dtype, generator=g).unique()).values, b
    if dist == "equal":
        return torch.full((na,), 12345, device="cuda", dtype=dtype), torch.full((nb,), 12345, device="cuda", dtype=dtype)
    if dist == "disjoint":
        return torch.arange(na, device="cuda", dtype=dtype), torch.arange(nb, device="cuda", dtype=dtype) + na
    if dist == "same":
        a = ascending(torch, na, dtype, g)
        return a, a.clone()
    raise KeyError(dist)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=27)
    ap.add_argument("--log2small", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    N, S = 1 << args.log2n, 1 << args.log2small
    every = [(op, "keys") for op in OPS]
    legs = [("uint", dist, N, N, every + [("union", "values"), ("union", "arg")]) for dist in ("uniform", "equal", "disjoint", "same")]
    legs += [("uint", "batch", S, N, every), ("ulong", "uniform", N, N, every)]
    rec = {"what": "setop_probe", "device": ctx.device_name, "tile": {"uint": clo.setop_tile(4, 4), "ulong": clo.setop_tile(8, 0)}, "legs": []}
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())

    for kt, dist, na, nb, cases in legs:
        dtype, ks = (torch.int32, 4) if kt == "uint" else (torch.int64, 8)
        g = torch.Generator(device="cuda").manual_seed(na + nb)
        a, b = make_inputs(torch, dist, na, nb, dtype, g)
        na, nb = a.numel(), b.numel()
        n = na + nb
        values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        ok, mk = torch.empty(n, device="cuda", dtype=dtype), torch.empty(n, device="cuda", dtype=dtype)
        ov, mv = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(n, device="cuda", dtype=torch.int32)
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        ba, bb, bok, bmk, bov, bmv, bnum = B(a), B(b), B(ok), B(mk), B(ov), B(mv), B(num)
        bva, bvb = B(values[:na]), B(values[na:])
        duplicate_free = dist != "equal"
        for op, mode in cases:
            vs = 0 if mode == "keys" else 4
            valued = mode == "values"
            so, merger = clo.SetOp(op, ctx, kt, vs), clo.Merge(ctx, kt, vs)
            keep = {}
            run = {"setop": lambda: so.with_device_data(q, ba, bva if valued else None, na, bb, bvb if valued else None, nb,
                                                        bok, bov if vs else None, bnum),
                   "merge": lambda: merger.with_device_data(q, ba, bva if valued else None, na, bb, bvb if valued else None, nb,
                                                            bmk, bmv if vs else None)}
            if duplicate_free and mode == "keys" and op != "symmetric_difference":
                def torch_way():
                    if op == "union":
                        keep["t"] = torch.unique_consecutive(torch.sort(torch.cat((a, b))).values)
                    elif op == "intersection":
                        keep["t"] = a[torch.isin(a, b)]
                    else:
                        keep["t"] = a[~torch.isin(a, b)]
                run["torch"] = torch_way
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
            # one more pass with the library's per-kernel events: where the time goes
            labels = ("setop_partition", "setop_count", "setop_scan", "setop_apply", "merge_partition", "merge")
            _hip.lib.clo_hip_timing_enable(1)
            _hip.lib.clo_hip_timing_reset()
            for _ in range(3):
                run["setop"]()
                run["merge"]()
            torch.cuda.synchronize()
            kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in labels}
            _hip.lib.clo_hip_timing_enable(0)
            k = int(num[0].item())
            agrees = None
            if "torch" in run:
                t = keep["t"]
                agrees = t.numel() == k and bool(torch.equal(t, ok[:k]))
            keeps_b = op in ("union", "symmetric_difference")
            by = 2 * n * ks + k * ks + ((na + (nb if keeps_b else 0) + k) * 4 if valued else k * 4 if vs else 0)
            by_merge = 2 * n * ks + (2 * n * 4 if valued else n * 4 if vs else 0)
            entry = {"keys": kt, "distribution": dist, "numel_a": na, "numel_b": nb, "op": op, "mode": mode, "reps": args.reps,
                     "num_out": k, "agrees_with_torch": agrees, "bytes": by, "merge_bytes": by_merge, "kernel_ms": kernel_ms, "variants": {}}
            for v in variants:
                t = sorted(ms[v])
                entry["variants"][v] = {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4),
                                        "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}
            V = entry["variants"]
            med = V["setop"]["median_ms"]
            entry["bytes_over_merge"] = round(by / by_merge, 3)
            entry["time_over_merge"] = round(med / V["merge"]["median_ms"], 3)
            spread = max(V["setop"]["spread"], V["merge"]["spread"])
            entry["time_exceeds_bytes"] = entry["time_over_merge"] > entry["bytes_over_merge"] * (1 + spread)
            entry["bytes_per_s"] = round(by / (med * 1e-3))
            if "torch" in V:
                entry["time_over_torch"] = round(med / V["torch"]["median_ms"], 3)
                entry["verdict"] = "LOSES" if med > V["torch"]["median_ms"] else "wins"
            rec["legs"].append(entry)
            print(json.dumps(entry), flush=True)
            so.close()
            merger.close()
            keep.clear()
        for x in (ba, bb, bok, bmk, bov, bmv, bnum, bva, bvb):
            x.close()
        del a, b, values, ok, mk, ov, mv, num
        torch.cuda.empty_cache()

    rec["legs_that_lose_to_torch"] = [[e["distribution"], e["keys"], e["op"]] for e in rec["legs"] if e.get("verdict") == "LOSES"]
    rec["legs_whose_time_exceeds_their_bytes"] = [[e["distribution"], e["keys"], e["op"], e["mode"]] for e in rec["legs"] if e["time_exceeds_bytes"]]
    rec["every_result_agrees"] = all(e["agrees_with_torch"] is not False for e in rec["legs"])
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
