"""Measurement probe (not part of the bench contract): sorting by key against the AoS pair sort, in one process.

At 2^20 .. 2^28 pairs of uint32 keys and uint32 values (radix 16) it times, alternating and with device events, four
variants of the same sort:
  aos           the pair sort of BASELINE config 4: ulong elements (key << 32 | value), get_key "(uint) ((x) >> 32)"
  kv            clo_sort_by_key_with_device_data: keys and values in two arrays, both written
  argsort       values NULL (the indices), keys_out given
  argsort_only  values NULL, keys_out NULL
after warming up every shape it times. For each it reports the median and the minimum, the bytes its schedule moves
(histograms, passes, digit stream) and the share of 8 TB/s those bytes take at the median. A second section reports
what the pack and unpack kernels cost where the by-key sort goes through them (the one-launch kernel, the
single-sweep passes), from the library's per-kernel timing. Prints one JSON record.
Usage on the GPU machine: python tools/kv_probe.py [--sizes 20,22,24,26,28] [--reps R]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cl_ops_amd as clo  # noqa: E402
from cl_ops_amd import _hip  # noqa: E402

PEAK = 8e12
VARIANTS = ("aos", "kv", "argsort", "argsort_only")


def schedule_bytes(n, variant, passes=4, digit_stream=True):
    """Bytes the radix-16 chain-free schedule moves for n 32-bit keys + 32-bit values (8-byte pairs)."""
    dig = 2 * n * (passes - 1) if digit_stream else 8 * n * (passes - 1)   # stream written + histogram read / element re-read
    mid = 16 * n * (passes - 2)                                             # middle passes: 8 in + 8 out
    if variant == "aos":
        return 8 * n + 16 * n + mid + 16 * n + dig
    first_in = 8 * n if variant == "kv" else 4 * n                          # keys (+ values) read by the first pass
    last_out = 4 * n if variant == "argsort_only" else 8 * n                # (keys +) values written by the last pass
    return 4 * n + first_in + 8 * n + mid + 8 * n + last_out + dig


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="20,22,24,26,28")
    ap.add_argument("--reps", type=int, default=0, help="timed rounds per size (0: enough for ~0.3 s of sorting per variant)")
    args = ap.parse_args()
    ctx = clo.Context(0)
    q = clo.Queue(ctx)
    s_aos = clo.Sorter("satradix", ctx, "ulong", key_type="uint", get_key="(uint) ((x) >> 32)")
    s_kv = clo.Sorter("satradix", ctx, "uint")
    timer = clo.HipEventTimer(q)
    rec = {"what": "kv_probe", "device": ctx.device_name, "radix": 16, "peak_bytes_per_s": PEAK, "sizes": []}

    for logn in [int(x) for x in args.sizes.split(",")]:
        n = 1 << logn
        g = torch.Generator(device="cuda").manual_seed(logn)
        keys = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32, generator=g)
        pairs = (keys.to(torch.int64) << 32) | (values.to(torch.int64) & 0xffffffff)
        pairs_out = torch.empty_like(pairs)
        ko, vo = torch.empty_like(keys), torch.empty_like(values)
        torch.cuda.synchronize()
        B = lambda t: clo.Buffer(ctx, t.numel() * t.element_size(), device_ptr=t.data_ptr())
        bp, bpo, bk, bv, bko, bvo = B(pairs), B(pairs_out), B(keys), B(values), B(ko), B(vo)
        run = {
            "aos": lambda: s_aos.with_device_data(q, bp, bpo, n),
            "kv": lambda: s_kv.by_key_with_device_data(q, bk, bv, bko, bvo, n),
            "argsort": lambda: s_kv.by_key_with_device_data(q, bk, None, bko, bvo, n),
            "argsort_only": lambda: s_kv.by_key_with_device_data(q, bk, None, None, bvo, n),
        }
        for v in VARIANTS:   # warm-up: code objects, cached buffers of this size
            for _ in range(3):
                run[v]()
        q.finish()
        reps = args.reps or max(10, min(400, int(0.3e3 / (4.2 * n / (1 << 28)))))
        ms = {v: [] for v in VARIANTS}
        for r in range(reps):
            order = VARIANTS if r % 2 == 0 else VARIANTS[::-1]
            for v in order:
                timer.start()
                run[v]()
                timer.stop()
                ms[v].append(timer.elapsed_ms())
        q.finish()
        # the results agree (the pairs' halves are the two arrays)
        run["aos"]()
        run["kv"]()
        q.finish()
        agree = bool(torch.equal((pairs_out >> 32).to(torch.int32), ko) and torch.equal(pairs_out.to(torch.int32), vo))
        entry = {"log2n": logn, "n": n, "reps": reps, "results_agree": agree, "variants": {}}
        big = n * 8 >= (32 << 20)
        for v in VARIANTS:
            t = sorted(ms[v])
            med = t[len(t) // 2]
            by = schedule_bytes(n, v, digit_stream=big)
            entry["variants"][v] = {"median_ms": round(med, 4), "min_ms": round(t[0], 4), "bytes": by,
                                    "share_of_peak": round(by / (med * 1e-3) / PEAK, 3)}
        base = entry["variants"]["aos"]["median_ms"]
        for v in VARIANTS[1:]:
            entry["variants"][v]["ratio_to_aos"] = round(entry["variants"][v]["median_ms"] / base, 3)
        rec["sizes"].append(entry)
        for b in (bp, bpo, bk, bv, bko, bvo):
            b.close()
        del keys, values, pairs, pairs_out, ko, vo
        torch.cuda.empty_cache()

    # pack / unpack around the pair sort: the one-launch kernel (<= 8192 pairs) and the single-sweep passes
    rec["pack_unpack"] = []
    labels = ("radix_kv_pack", "radix_kv_unpack", "radix_small", "radix_hist", "radix_offsets", "radix_pass", "radix_sweep", "radix_ghist")
    for n in (4096, 8192, 1 << 16, 1 << 20):
        keys = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32)
        values = torch.randint(-(1 << 31), 1 << 31, (n,), device="cuda", dtype=torch.int32)
        ko, vo = torch.empty_like(keys), torch.empty_like(values)
        torch.cuda.synchronize()
        B = lambda t: clo.Buffer(ctx, t.numel() * 4, device_ptr=t.data_ptr())
        bk, bv, bko, bvo = B(keys), B(values), B(ko), B(vo)
        for _ in range(3):
            s_kv.by_key_with_device_data(q, bk, bv, bko, bvo, n)
        q.finish()
        reps = 50
        _hip.check(_hip.lib.clo_hip_timing_enable(1))
        _hip.check(_hip.lib.clo_hip_timing_reset())
        for _ in range(reps):
            s_kv.by_key_with_device_data(q, bk, bv, bko, bvo, n)
        q.finish()
        per = {}
        for l in labels:
            cnt, tot = _hip.timing_read(l)
            if cnt:
                per[l] = round(tot / reps * 1e3, 2)
        _hip.check(_hip.lib.clo_hip_timing_enable(0))
        rec["pack_unpack"].append({"n": n, "us_per_sort_by_label": per})
        for b in (bk, bv, bko, bvo):
            b.close()

    timer.close()
    s_aos.close()
    s_kv.close()
    q.close()
    ctx.close()
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
