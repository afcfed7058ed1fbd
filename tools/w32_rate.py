#!/usr/bin/env python3
"""Streaming rate of the 32-bit word form beside the 64-bit one, in ONE process (GPU box).

For each of X25519, NIST256, X448 at 2^24 elements on tiles of 4096: four operand triples per word length (the placement probe of
docs/measurement.md), both kernels warmed up, then modmul at word length 64 (the kernel the 32-bit form leaves untouched) and at word
length 32 timed ALTERNATING by device events, at least 20 launches per placement; the same for modsqr and for modadd (the three-stream
control).  In the same alternation the 32-bit kernel runs at every (elements per lane, workgroup size) the library holds
(MA_W32_EPT x MA_W32_BLOCK): the alternatives the default launch shape of each prime was chosen from.

Reported per kernel and placement: ms (median over the launches), elements/s, algorithmic bytes/s (operands read + result written:
3 x Nlimbs x word bytes for modmul / modadd, 2 x for modsqr), share of the 8 TB/s HBM peak, and for each 32-bit kernel its ratio to
modadd at 32 bits on the same buffers.  The judgement the numbers are for: the median-over-placements bytes/s of the 32-bit modmul is
not below the LOWEST placement of the 64-bit one in the same run.

  python tools/w32_rate.py [--log2n 24] [--launches 20] [--placements 4] [--out profiles/w32_rate.json]
  rocprofv3 --kernel-trace --stats -d <dir> -- python tools/w32_rate.py --launches 5 --placements 1 --out <dir>/w32_rate_traced.json
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
PRIMES = ("X25519", "NIST256", "X448")
KERNELS = (("modmul", 3), ("modsqr", 2), ("modadd", 3))          # (name, streams)
VARIANTS = tuple((e, b) for e in (4, 2, 1) for b in (256, 128, 64)) + ((1, 512),)   # (elements per lane, workgroup size) of the 32-bit streaming kernels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--placements", type=int, default=4)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--primes", default=",".join(PRIMES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w32_rate.json"))
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "w32_rate.py measures on the GPU: no device, no number"
    from modarith_amd.field import Field
    n = 1 << args.log2n
    os.environ.pop("MA_W32_EPT", None)
    report = {"n": n, "tile": args.tile, "launches": args.launches, "placements": args.placements, "hbm_peak_Bps": HBM_PEAK,
              "device": torch.cuda.get_device_name(0), "timing": "device events around single launches, median per placement", "primes": {}}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        return e0, e1

    for P in args.primes.split(","):
        F = {64: Field(P, tile=args.tile), 32: Field(P, wl=32, tile=args.tile)}
        wbytes = {64: 8, 32: 4}
        # four operand triples per word length, allocated interleaved, inputs in Montgomery / internal form (field-function outputs)
        trip = {64: [], 32: []}
        for k in range(args.placements):
            for wl in (64, 32):
                a = F[wl].nres(F[wl].uniform(n, seed=11, array=2 * k))
                b = F[wl].nres(F[wl].uniform(n, seed=11, array=2 * k + 1))
                trip[wl].append((a, b, F[wl].empty(n)))
        per = {"nlimbs": {wl: F[wl].N for wl in (64, 32)}, "kernels": {}}
        for kname, streams in KERNELS:
            def launch(wl, t):
                a, b, c = t
                if streams == 3:
                    getattr(F[wl], kname)(a, b, out=c)
                else:
                    getattr(F[wl], kname)(a, out=c)
            def variant_env(v):
                for key in ("MA_W32_EPT", "MA_W32_BLOCK"):
                    os.environ.pop(key, None)
                if v is not None:
                    os.environ["MA_W32_EPT"], os.environ["MA_W32_BLOCK"] = str(v[0]), str(v[1])

            # what is timed side by side: the 64-bit kernel, the 32-bit kernel as the library launches it, and the 32-bit kernel at
            # every (elements per lane, workgroup size) the library holds (MA_W32_EPT / MA_W32_BLOCK: read at every call)
            runs = [("w64", 64, None), ("w32", 32, None)] + [("w32_e%d_b%d" % v, 32, v) for v in VARIANTS]
            rows = {name: [] for name, _, _ in runs}
            for k in range(args.placements):
                for name, wl, v in runs:                   # warm up every kernel on these buffers
                    variant_env(v)
                    for _ in range(3):
                        launch(wl, trip[wl][k])
                torch.cuda.synchronize()
                ev = {name: [] for name, _, _ in runs}
                for _ in range(args.launches):             # alternating
                    for name, wl, v in runs:
                        variant_env(v)
                        ev[name].append(timed(lambda: launch(wl, trip[wl][k])))
                torch.cuda.synchronize()
                variant_env(None)
                for name, wl, v in runs:
                    ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[name])
                    nbytes = streams * F[wl].N * wbytes[wl] * n
                    rows[name].append({"placement": k, "ms": ms, "elements_per_s": n / (ms * 1e-3), "bytes_per_s": nbytes / (ms * 1e-3),
                                       "hbm_share": nbytes / (ms * 1e-3) / HBM_PEAK, "bytes_per_element": streams * F[wl].N * wbytes[wl]})
            med = lambda name, key: statistics.median(r[key] for r in rows[name])
            per["kernels"][kname] = {
                "w64": rows["w64"], "w32": rows["w32"],
                "w32_variants": {name: rows[name] for name, _, v in runs if v is not None},
                "w32_variants_median_hbm_share": {name: med(name, "hbm_share") for name, _, v in runs if v is not None},
                "median_bytes_per_s": {"w64": med("w64", "bytes_per_s"), "w32": med("w32", "bytes_per_s")},
                "lowest_w64_bytes_per_s": min(r["bytes_per_s"] for r in rows["w64"]),
                "w32_median_not_below_lowest_w64": med("w32", "bytes_per_s") >= min(r["bytes_per_s"] for r in rows["w64"]),
                "elements_ratio_w32_over_w64": med("w32", "elements_per_s") / med("w64", "elements_per_s")}
        for kname, _ in KERNELS:                           # each 32-bit kernel against modadd at 32 bits on the same buffers
            k32, add32 = per["kernels"][kname]["w32"], per["kernels"]["modadd"]["w32"]
            per["kernels"][kname]["w32_ms_over_modadd_w32_ms"] = [r["ms"] / a["ms"] for r, a in zip(k32, add32)]
        report["primes"][P] = per
        for kname, _ in KERNELS:
            k = per["kernels"][kname]
            best = max(k["w32_variants_median_hbm_share"].items(), key=lambda kv: kv[1])
            print("%-8s %-7s w64 %.3f ms %.3f of peak (lowest %.3f) | w32 %.3f ms %.3f of peak | elements w32/w64 %.3f | w32 median >= lowest w64: %s | best variant %s %.3f" % (
                P, kname, statistics.median(r["ms"] for r in k["w64"]), k["median_bytes_per_s"]["w64"] / HBM_PEAK, k["lowest_w64_bytes_per_s"] / HBM_PEAK,
                statistics.median(r["ms"] for r in k["w32"]), k["median_bytes_per_s"]["w32"] / HBM_PEAK, k["elements_ratio_w32_over_w64"],
                k["w32_median_not_below_lowest_w64"], best[0], best[1]), flush=True)
            print("         variants (median share of peak): " + " ".join("%s %.3f" % (nm[4:], v) for nm, v in k["w32_variants_median_hbm_share"].items()), flush=True)
        del trip, F
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
