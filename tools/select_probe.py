"""Measurement probe (not part of the bench contract): selection and partition against what a user would write in torch
today and against this library's reduce by key in its "distinct keys alone" form (the sibling: the same three-launch
shape — a sweep, a one-group scan, a compacting sweep — on the same number of keys), on the same GPU in one process.

Legs, at 2^28 uint32 keys unless noted:
  flagged select at p = 0.01 / 0.5 / 0.99        torch: keys[mask]
  "lt" select with the threshold at the median   torch: keys[keys < t]
  partition, by flags (p = 0.5) and by "lt"      torch: none
  flagged select with uint32 values              torch: none
  the indices of the set flags (the arg form, no keys)   torch: torch.nonzero(mask)
  uint64 keys, "lt" select                       torch: none
  2^20 and 2^24 keys, flagged select p = 0.5     torch: none
Every variant of every shape is warmed up first; then the variants alternate, timed with device events on one stream,
for 7 rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the bytes its schedule
moves (the decision's input read twice: once to count, once to apply; keys and values read once more where the decision
does not read them; the rows written), those bytes per second as a fraction of the 8 TB/s peak, its time over torch's,
and its time per byte over the sibling's; LOSES where it is slower than torch, or more than the measured spread slower
per byte than the sibling. Then one pass with the library's per-kernel events: where the time goes. k and the rows are
compared with torch's where torch ran.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/select_probe.py [--log2n 28] [--reps 7] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12


def stats(ms):
    t = sorted(ms)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=28)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    N = 1 << args.log2n
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "select_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK,
           "tile": {"uint": clo.select_tile(4, 0), "uint + values": clo.select_tile(4, 4), "ulong": clo.select_tile(8, 0)}, "legs": []}

    # (name, key type, n, op, pred, p or None, form, torch form)
    legs = [("flagged select p=%g" % p, "uint", N, "select", "flagged", p, "keys", "keys[mask]") for p in (0.01, 0.5, 0.99)]
    legs += [("lt select at the median", "uint", N, "select", "lt", None, "keys", "keys[keys < t]"),
             ("flagged partition p=0.5", "uint", N, "partition", "flagged", 0.5, "keys", None),
             ("lt partition at the median", "uint", N, "partition", "lt", None, "keys", None),
             ("flagged select p=0.5 with uint32 values", "uint", N, "select", "flagged", 0.5, "values", None),
             ("indices of the set flags p=0.5", "uint", N, "select", "flagged", 0.5, "arg", "torch.nonzero(mask)"),
             ("uint64 keys, lt select at the median", "ulong", N, "select", "lt", None, "keys", None)]
    legs += [("flagged select p=0.5, 2^%d keys" % lg, "uint", 1 << lg, "select", "flagged", 0.5, "keys", None) for lg in (20, 24) if lg < args.log2n]

    made = {}

    def arrays(kt, n):
        """The shape's inputs and outputs, made once per (key type, n)."""
        if (kt, n) not in made:
            made.clear()
            torch.cuda.empty_cache()
            dtype = torch.int32 if kt == "uint" else torch.int64
            g = torch.Generator(device="cuda").manual_seed(n + len(kt))
            top = (1 << 31) if kt == "uint" else (1 << 62)                 # non-negative: torch's signed order is the unsigned one
            keys = torch.randint(0, top, (n,), device="cuda", dtype=dtype, generator=g)
            a = {"keys": keys, "values": torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g),
                 "uniform": torch.rand(n, device="cuda", generator=g), "thr": torch.tensor([top // 2], device="cuda", dtype=dtype),
                 "ko": torch.empty_like(keys), "vo": torch.empty(n, device="cuda", dtype=torch.int32), "num": torch.zeros(2, device="cuda", dtype=torch.int64),
                 # the sibling's input: runs of 16 on average, as in tools/rbk_probe.py
                 "runs": torch.cumsum(torch.rand(n, device="cuda", generator=g) < 1.0 / 16, 0, dtype=torch.int32)}
            made[(kt, n)] = a
        return made[(kt, n)]

    for name, kt, n, op, pred, p, form, torch_form in legs:
        a = arrays(kt, n)
        ks = 4 if kt == "uint" else 8
        keys, thr, ko, vo, num = a["keys"], a["thr"], a["ko"], a["vo"], a["num"]
        flags = ((a["uniform"] < p).to(torch.uint8) * 3) if pred == "flagged" else None       # flags of 0 and 3
        mask = flags != 0 if flags is not None else None
        vs = 0 if form == "keys" else 4
        sel = clo.Select(op, pred, ctx, kt, vs)
        sib = clo.ReduceByKey(ctx, "uint", None, "uint")
        bk, bv, bfot, bko, bvo, bnum, bruns = B(keys), B(a["values"]), B(flags if flags is not None else thr), B(ko), B(vo), B(num), B(a["runs"])
        bsib_out = B(a["vo"])
        keep = {}
        run = {"select": lambda: sel.with_device_data(q, None if form == "arg" else bk, bv if form == "values" else None, bfot,
                                                      None if form == "arg" else bko, bvo if vs else None, bnum, n),
               "sibling": lambda: sib.with_device_data(q, bruns, None, bsib_out, None, bnum_sib, n)}
        num_sib = torch.zeros(2, device="cuda", dtype=torch.int64)
        bnum_sib = B(num_sib)
        if torch_form == "keys[mask]":
            run["torch"] = lambda: keep.__setitem__("t", keys[mask])
        elif torch_form == "keys[keys < t]":
            run["torch"] = lambda: keep.__setitem__("t", keys[keys < thr])
        elif torch_form == "torch.nonzero(mask)":
            run["torch"] = lambda: keep.__setitem__("t", torch.nonzero(mask))
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
        labels = ("select_count", "select_scan", "select_apply")
        _hip.lib.clo_hip_timing_enable(1)
        _hip.lib.clo_hip_timing_reset()
        for _ in range(3):
            run["select"]()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in labels}
        _hip.lib.clo_hip_timing_enable(0)
        run["sibling"]()
        run["select"]()
        torch.cuda.synchronize()
        k, m = int(num[0].item()), int(num_sib[0].item())
        agrees = None
        if "torch" in run:
            run["torch"]()
            t = keep["t"].flatten()
            agrees = t.numel() == k and bool(torch.equal(t, vo[:k].to(torch.int64) if form == "arg" else ko[:k]))
        rows = n if op == "partition" else k
        decision = n if pred == "flagged" else ks * n                      # read by both sweeps
        by = 2 * decision + (ks * n if pred == "flagged" and form != "arg" else 0) + (0 if form == "arg" else ks * rows) \
            + (4 * n + 4 * rows if form == "values" else 4 * rows if form == "arg" else 0)
        by_sib = 2 * 4 * n + 4 * m
        V = {v: stats(ms[v]) for v in variants}
        med, med_sib = V["select"]["median_ms"], V["sibling"]["median_ms"]
        spread = max(V["select"]["spread"], V["sibling"]["spread"])
        entry = {"leg": name, "keys": kt, "n": n, "op": op, "pred": pred, "p": p, "form": form, "torch_form": torch_form, "reps": args.reps,
                 "num_out": k, "agrees_with_torch": agrees, "bytes": by, "kernel_ms": kernel_ms, "variants": V,
                 "bytes_per_s": round(by / (med * 1e-3)), "fraction_of_peak": round(by / (med * 1e-3) / PEAK, 3),
                 "sibling": {"what": "reduce by key, distinct keys alone, runs of 16", "runs": m, "bytes": by_sib,
                             "fraction_of_peak": round(by_sib / (med_sib * 1e-3) / PEAK, 3)},
                 "time_per_byte_over_sibling": round((med / by) / (med_sib / by_sib), 3)}
        loses = []
        if entry["time_per_byte_over_sibling"] > 1 + spread:
            loses.append("to the sibling per byte")
        if "torch" in V:
            entry["time_over_torch"] = round(med / V["torch"]["median_ms"], 3)
            if med > V["torch"]["median_ms"]:
                loses.append("to torch")
        entry["verdict"] = "LOSES " + " and ".join(loses) if loses else "holds"
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in (sel, sib, bk, bv, bfot, bko, bvo, bnum, bruns, bsib_out, bnum_sib):
            x.close()
        keep.clear()
        del flags, mask

    rec["legs_that_lose"] = [[e["leg"], e["verdict"]] for e in rec["legs"] if e["verdict"] != "holds"]
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
