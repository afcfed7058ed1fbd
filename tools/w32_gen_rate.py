#!/usr/bin/env python3
"""Streaming rate of GENERATED 32-bit fields beside the 64-bit field of the same prime, in ONE process (GPU box).

The method is that of tools/w32_rate.py.  For each of BP256, NIST384 and PM512 at 2^24 elements on tiles of 4096: several operand
triples per word length (the placement probe of docs/measurement.md), both kernels warmed up, then modmul at word length 64 (the
64-bit plug-in or built-in field of the prime) and at word length 32 (the plug-in of `generate w32`, at the library's default launch
shape) timed ALTERNATING by device events, at least 20 launches per placement; the same for modsqr.  Then, for one generated prime
(BP256) at 2^22 elements, modinv with shared inversions against MA_INV_SIMUL=0 (one inversion per element), each path in child
processes of its own, alternating A B A B (the library reads the knob once per process).

Reported per kernel and placement: ms (median over the launches), elements/s, algorithmic bytes/s (operands read + result written),
share of the 8 TB/s HBM peak.  The judgement the numbers are for -- the project's rule for this word length --: the
median-over-placements bytes/s of the 32-bit modmul is not below the LOWEST placement of the 64-bit one in the same run.

  python tools/w32_gen_rate.py [--log2n 24] [--launches 20] [--placements 4] [--out profiles/w32_gen_rate.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
# 32-bit tag -> (command-line argument of `generate w32`, family, the 64-bit field of the same prime)
PRIMES = {"BP256": ("BP256=0xa9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377", "monty", "BP256"),
          "NIST384": ("NIST384", None, "NIST384"), "PM512": ("PM512", None, "PM512")}
KERNELS = (("modmul", 3), ("modsqr", 2))          # (name, streams)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--log2n-inv", type=int, default=22)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--placements", type=int, default=4)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--primes", default=",".join(PRIMES))
    ap.add_argument("--inv-prime", default="BP256")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w32_gen_rate.json"))
    ap.add_argument("--inv-child", default=None, help="(internal) time modinv of this prime in this process and print one JSON line")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "w32_gen_rate.py measures on the GPU: no device, no number"
    from modarith_amd import _lib, generate as gen
    from modarith_amd.field import Field
    if args.inv_child:
        F = Field(args.inv_child, wl=32, tile=args.tile)
        m = 1 << args.log2n_inv
        x, z = F.nres(F.uniform(m, seed=13, array=0)), F.empty(m)
        for _ in range(3):
            F.modinv(x, out=z)
        torch.cuda.synchronize()
        ev = []
        for _ in range(10):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            F.modinv(x, out=z)
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize()
        ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)
        print(json.dumps({"ms": round(ms, 3), "elements_per_s": m / (ms * 1e-3), "launch": _lib.load().modarith_amd_last_launch().decode()}))
        return
    n = 1 << args.log2n
    for key in ("MA_W32_EPT", "MA_W32_BLOCK", "MA_INV_SIMUL"):
        os.environ.pop(key, None)
    report = {"n": n, "tile": args.tile, "launches": args.launches, "placements": args.placements, "hbm_peak_Bps": HBM_PEAK,
              "device": torch.cuda.get_device_name(0), "timing": "device events around single launches, median per placement", "primes": {}}

    def timed(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        return e0, e1

    for T in args.primes.split(","):
        arg, fam, P64 = PRIMES[T]
        assert gen.generate_w32(arg, family=fam).tag == T
        F = {64: Field(P64, tile=args.tile), 32: Field(T, wl=32, tile=args.tile)}
        assert F[64].params.p == F[32].params.p
        wbytes = {64: 8, 32: 4}
        trip = {64: [], 32: []}
        for k in range(args.placements):                      # operand triples of the two word lengths, allocated interleaved
            for wl in (64, 32):
                a = F[wl].nres(F[wl].uniform(n, seed=11, array=2 * k))
                b = F[wl].nres(F[wl].uniform(n, seed=11, array=2 * k + 1))
                trip[wl].append((a, b, F[wl].empty(n)))
        per = {"nlimbs": {str(wl): F[wl].N for wl in (64, 32)}, "radix": {str(wl): F[wl].radix for wl in (64, 32)}, "kernels": {}}
        for kname, streams in KERNELS:
            def launch(wl, t):
                a, b, c = t
                if streams == 3:
                    getattr(F[wl], kname)(a, b, out=c)
                else:
                    getattr(F[wl], kname)(a, out=c)
            for wl in (64, 32):
                for t in trip[wl]:
                    launch(wl, t)
            torch.cuda.synchronize()
            rows = {64: [], 32: []}
            for k in range(args.placements):
                ev = {64: [], 32: []}
                for _ in range(args.launches):
                    for wl in (64, 32):
                        ev[wl].append(timed(lambda: launch(wl, trip[wl][k])))
                torch.cuda.synchronize()
                for wl in (64, 32):
                    ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev[wl])
                    bps = streams * F[wl].N * wbytes[wl] * n / (ms * 1e-3)
                    rows[wl].append({"placement": k, "ms": round(ms, 4), "elements_per_s": n / (ms * 1e-3), "bytes_per_s": bps, "hbm_share": round(bps / HBM_PEAK, 4)})
            med32 = statistics.median(r["bytes_per_s"] for r in rows[32])
            low64 = min(r["bytes_per_s"] for r in rows[64])
            per["kernels"][kname] = {"wl64": rows[64], "wl32": rows[32], "wl32_median_bytes_per_s": med32, "wl64_lowest_bytes_per_s": low64,
                                     "wl32_median_hbm_share": round(med32 / HBM_PEAK, 4), "wl64_lowest_hbm_share": round(low64 / HBM_PEAK, 4),
                                     "wl32_median_elements_per_s": statistics.median(r["elements_per_s"] for r in rows[32]),
                                     "wl64_median_elements_per_s": statistics.median(r["elements_per_s"] for r in rows[64]),
                                     "meets_the_rule": bool(med32 >= low64)}
            print("%-8s %-7s wl32 median %.3f of peak (%d x %d bits), wl64 lowest %.3f of peak (%d x %d bits): %s" % (
                T, kname, med32 / HBM_PEAK, F[32].N, F[32].radix, low64 / HBM_PEAK, F[64].N, F[64].radix, "meets the rule" if med32 >= low64 else "BELOW"), flush=True)
        report["primes"][T] = per
        del trip, F
        torch.cuda.empty_cache()

    # shared against per-element inversion of one generated prime: the library reads MA_INV_SIMUL once per process, so each path runs in
    # child processes of its own, alternating A B A B (the method of tools/w32_inv_rate.py)
    import subprocess
    T = args.inv_prime
    rows = {"shared": [], "per_element": []}
    for rep in range(2):
        for name, knob in (("shared", None), ("per_element", "0")):
            env = dict(os.environ)
            env.pop("MA_INV_SIMUL", None)
            if knob is not None:
                env["MA_INV_SIMUL"] = knob
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--inv-child", T, "--log2n-inv", str(args.log2n_inv), "--tile", str(args.tile)],
                               capture_output=True, text=True, env=env, timeout=600)
            assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
            row = json.loads(r.stdout.strip().splitlines()[-1])
            assert row["launch"] == ("modinv(w32, simultaneous)" if knob is None else "modinv(w32)"), row
            rows[name].append(row)
    m = 1 << args.log2n_inv
    med = {name: statistics.median(r["elements_per_s"] for r in rows[name]) for name in rows}
    report["modinv"] = {"prime": T, "n": m, "rows": rows, "shared_elements_per_s": med["shared"], "per_element_elements_per_s": med["per_element"],
                        "speedup": round(med["shared"] / med["per_element"], 2)}
    print("%-8s modinv at 2^%d: shared %.3g/s, per element %.3g/s (x %.1f)" % (T, args.log2n_inv, med["shared"], med["per_element"], med["shared"] / med["per_element"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
