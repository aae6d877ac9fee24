"""Measurement probe (not part of the bench contract): CloJoin against what a caller has today, on the same GPU in one
process.

Baselines, on the same inputs (inner joins only: neither has an outer form; a left join's torch baseline clamps the
counts to 1 and masks the indices):
  (a) the composition from this library: CloSearch lower + upper bounds of A in B with sorted needles, a torch
      subtraction for the counts, CloExpand("counts") for the ids and ranks (its three ends launches are the scan), and a
      torch gather-add for idx_b;
  (b) torch: searchsorted twice, repeat_interleave, cumsum and arange arithmetic.
Legs (uint keys unless said, 2^27 keys a side unless said): inner, left and full joins of duplicate-free inputs with one
key in eight shared; a 1 : 16 fan-out (A unique, B runs of 16); 16 x 16 runs at 2^23 keys a side (K = 2^27); one key
2^14 x 2^14 (K = 2^28); disjoint inputs; A == B; the count form alone; ulong keys; 2^20 keys against 2^27; 2^24 keys a
side. The join writes idx_a_out and idx_b_out into a capacity of exactly K, which the count form found.
Every variant of every leg is warmed up first; then the variants alternate, timed with device events on one stream, for
--reps rounds; each reports its median, minimum and spread (max - min) / median. A leg reports the bytes its schedule
moves (the keys read once by the count; unless only the count is wanted, the 16-byte table entry of every EMITTER —
an element that emits at least one row, counted here with torch from the run bounds — written once and read once, and
8 bytes per row written), those bytes per second as a fraction of the 8 TB/s peak, and its time over each baseline's;
LOSES where it is slower than a baseline. Then one pass with the library's per-kernel events: where the time goes. Every inner result is compared with torch's before anything is timed.
Prints one JSON record (and writes it to --out).
Usage on the GPU machine: python tools/join_probe.py [--shift 0] [--reps 5] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8.0e12
LABELS = ("join_partition", "join_count", "join_scan", "join_first", "join_write")


def stats(ms):
    t = sorted(ms)
    return {"median_ms": round(t[len(t) // 2], 4), "min_ms": round(t[0], 4), "spread": round((t[-1] - t[0]) / t[len(t) // 2], 3)}


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--shift", type=int, default=0, help="every size divided by 2^shift (a quick look)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx, stream=torch.cuda.current_stream().cuda_stream)   # torch's stream: one timer for everything
    timer = clo.HipEventTimer(q)
    B = lambda t: clo.Buffer(ctx, max(t.numel(), 2) * t.element_size(), device_ptr=t.data_ptr())
    rec = {"what": "join_probe", "device": ctx.device_name, "peak_bytes_per_s": PEAK, "tile": clo.join_tile(4), "out_tile": clo.join_out_tile(), "legs": []}
    N = 1 << (27 - args.shift)
    ar = lambda n, dt=torch.int32: torch.arange(n, device="cuda", dtype=dt)

    def one_in_eight(n, dt=torch.int32):
        a = ar(n, dt) * 2
        return a, torch.where(ar(n, dt) % 8 == 0, a, a + 1)

    # (name, kind, keys_a, keys_b as thunks, count form only)
    legs = [
        ("one key in eight shared", "inner", lambda: one_in_eight(N), False),
        ("one key in eight shared", "left", lambda: one_in_eight(N), False),
        ("one key in eight shared", "full", lambda: one_in_eight(N), False),
        ("1 : 16 fan-out", "inner", lambda: (ar(N), ar(N) // 16), False),
        ("16 x 16 runs, 2^23 a side", "inner", lambda: (ar(N >> 4) // 16, ar(N >> 4) // 16), False),
        ("one key 2^14 x 2^14", "inner", lambda: (torch.full((1 << (14 - args.shift // 2),), 7, device="cuda", dtype=torch.int32),) * 2, False),
        ("disjoint", "inner", lambda: (ar(N) * 2, ar(N) * 2 + 1), False),
        ("A == B", "inner", lambda: (ar(N), ar(N)), False),
        ("the count form alone", "inner", lambda: one_in_eight(N), True),
        ("ulong keys", "inner", lambda: one_in_eight(N, torch.int64), False),
        ("2^20 against 2^27", "inner", lambda: (ar(N >> 7) * 128, ar(N)), False),
        ("2^24 a side", "inner", lambda: one_in_eight(N >> 3), False),
    ]

    for name, kind, make, count_only in legs:
        torch.cuda.empty_cache()
        ka, kb = make()
        ka, kb = ka.contiguous(), kb.clone().contiguous()
        na, nb = ka.numel(), kb.numel()
        kt, ks = ("ulong", 8) if ka.dtype == torch.int64 else ("uint", 4)
        num = torch.zeros(2, device="cuda", dtype=torch.int64)
        bka, bkb, bnum = B(ka), B(kb), B(num)
        jn = clo.Join(kind, ctx, kt)
        jn.with_device_data(q, bka, na, bkb, nb, None, None, None, 0, bnum)
        torch.cuda.synchronize()
        K = int(num[0])
        cap = 0 if count_only else K
        # the emitters: rows of A with a partner, those without where the kind keeps them, and B's likewise
        with_partner = int((torch.searchsorted(kb, ka, right=True) > torch.searchsorted(kb, ka)).sum())
        b_alone = nb - int((torch.searchsorted(ka, kb, right=True) > torch.searchsorted(ka, kb)).sum())
        emitters = with_partner + (na - with_partner if kind in ("left", "full") else 0) + (b_alone if kind in ("right", "full") else 0)
        ia, ib = torch.empty(max(cap, 1), device="cuda", dtype=torch.int32), torch.empty(max(cap, 1), device="cuda", dtype=torch.int32)
        bia, bib = B(ia), B(ib)
        lo, hi = torch.empty(na, device="cuda", dtype=torch.int32), torch.empty(na, device="cuda", dtype=torch.int32)
        ids, rank = torch.empty(max(K, 1), device="cuda", dtype=torch.int32), torch.empty(max(K, 1), device="cuda", dtype=torch.int32)
        num2 = torch.zeros(2, device="cuda", dtype=torch.int64)
        blo, bhi, bids, brank, bnum2 = B(lo), B(hi), B(ids), B(rank), B(num2)
        srch, exp = clo.Search(ctx, kt), clo.Expand("counts", ctx, None, "uint")
        keep = {}
        baselines = kind in ("inner", "left") and not count_only and K < (1 << 31)

        def ours():
            jn.with_device_data(q, bka, na, bkb, nb, None if count_only else bia, None if count_only else bib, None, cap, bnum)

        def composition():
            srch.with_device_data(q, bkb, nb, bka, na, blo, upper=False, needles_sorted=True)
            srch.with_device_data(q, bkb, nb, bka, na, bhi, upper=True, needles_sorted=True)
            cnt = hi - lo
            keep["cnt"] = cnt
            bc = B(cnt)
            exp.with_device_data(q, bc, None, None, None, bids, brank, bnum2, na, K)
            bc.close()
            keep["ib_a"] = lo[ids.long()] + rank if K else rank[:0]

        def torch_b():
            l, h = torch.searchsorted(kb, ka), torch.searchsorted(kb, ka, right=True)
            cnt = h - l
            emit = cnt.clamp(min=1) if kind == "left" else cnt
            i = torch.repeat_interleave(ar(na, torch.int64), emit)
            start = torch.cumsum(emit, 0) - emit
            j = ar(i.numel(), torch.int64) - start[i] + l[i]
            if kind == "left":
                j = torch.where(cnt[i] > 0, j, torch.full_like(j, 0xFFFFFFFF))
            keep["ia_b"], keep["ib_b"] = i, j

        run = {"join": ours}
        if baselines and kind == "inner":
            run["composition (a)"] = composition
        if baselines:
            run["torch (b)"] = torch_b
        variants = tuple(run)
        for v in variants:   # warm-up: code objects, the objects' workspaces, torch's allocator
            for _ in range(2):
                run[v]()
        torch.cuda.synchronize()
        agrees = int(num[0]) == K
        if baselines:        # every output against torch before anything is timed
            agrees = agrees and keep["ia_b"].numel() == K
            agrees = agrees and bool(torch.equal(ia[:K].long() & 0xFFFFFFFF, keep["ia_b"])) and bool(torch.equal(ib[:K].long() & 0xFFFFFFFF, keep["ib_b"]))
            if kind == "inner":
                agrees = agrees and int(num2[0]) == K and bool(torch.equal(ids[:K], ia[:K])) and bool(torch.equal(keep["ib_a"][:K], ib[:K]))
        keep.clear()
        ms = {v: [] for v in variants}
        for r in range(args.reps):
            for v in (variants if r % 2 == 0 else variants[::-1]):
                timer.start()
                run[v]()
                timer.stop()
                ms[v].append(timer.elapsed_ms())
            keep.clear()
        torch.cuda.synchronize()
        _hip.lib.clo_hip_timing_enable(1)
        _hip.lib.clo_hip_timing_reset()
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        kernel_ms = {lab: round(_hip.timing_read(lab)[1] / 3, 4) for lab in LABELS}
        _hip.lib.clo_hip_timing_enable(0)
        n = na + nb
        by = n * ks + (0 if count_only else 32 * emitters + 8 * K)
        V = {v: stats(ms[v]) for v in variants}
        med = V["join"]["median_ms"]
        entry = {"leg": name, "kind": kind, "key_type": kt, "numel_a": na, "numel_b": nb, "K": K, "emitters": emitters, "capacity": cap, "reps": args.reps,
                 "agrees_with_baselines": agrees, "bytes": by, "kernel_ms": kernel_ms, "variants": V,
                 "bytes_per_s": round(by / (med * 1e-3)), "fraction_of_peak": round(by / (med * 1e-3) / PEAK, 3)}
        loses = []
        for v, key in (("composition (a)", "time_over_composition_a"), ("torch (b)", "time_over_torch_b")):
            if v in V:
                entry[key] = round(med / V[v]["median_ms"], 3)
                if entry[key] > 1.0:
                    loses.append("%s by %.2fx" % (v, entry[key]))
        entry["verdict"] = ("LOSES to " + " and ".join(loses)) if loses else ("holds" if len(V) > 1 else "no baseline has this form")
        rec["legs"].append(entry)
        print(json.dumps(entry), flush=True)
        for x in (jn, srch, exp, bka, bkb, bnum, bia, bib, blo, bhi, bids, brank, bnum2):
            x.close()
        del ka, kb, ia, ib, lo, hi, ids, rank

    rec["legs_that_lose"] = [[e["leg"], e["kind"], e["verdict"]] for e in rec["legs"] if e["verdict"].startswith("LOSES")]
    rec["every_result_agrees"] = all(e["agrees_with_baselines"] for e in rec["legs"])
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
