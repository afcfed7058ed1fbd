#!/usr/bin/env python3
"""Rate of fused chains with a batch-wide operand (Chain.shared()) beside the forms that stream it, in ONE process (GPU box).

Per prime (X25519, NIST256, X448) and word length (64, 32), at 2^24 elements on tiles of 4096:

 (1) the one-operation chain x * b with b shared (two arrays of traffic) beside the library's modmuls kernel (64 bits: the same two
     arrays, b0 in the kernel arguments) and beside modmul with b as a broadcast batch (three arrays);
 (2) the Edwards-add-shaped chain x y d + t with d shared (three arrays in, one out) beside the same chain with d as a fourth input
     batch (four in, one out) -- the form a caller could write before shared operands, whose text this work does not change: the baseline.

Every variant is warmed for at least 60 ms (and three launches), then timed ALTERNATING on the same buffers, each launch singly between
device events; the median of 20 launches is one reading, and the readings are repeated (--rounds) so that the run carries its own
spread: the largest relative difference between the baseline's repeated medians.  Each fused output is compared with the call-by-call
truth before anything is timed.  Reported: ms, the share of the 8 TB/s HBM peak over each variant's own bytes, shared / baseline beside
the ratio bytes predict (0.8) and shared chain / modmuls.  REQUIRED: the shared form of (2) is not slower than the fourth-batch form by
more than the spread -- the tool exits 1 where it is.

  python tools/chain_shared_rate.py [--log2n 24] [--launches 20] [--rounds 3] [--out profiles/chain_shared_rate.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12
PRIMES = ("X25519", "NIST256", "X448")
WARM_S = 0.060


def chains(P, wl):
    from modarith_amd.fuse import Chain
    mul = Chain(P, "rate_muls", wl=wl)
    mul.output(mul.modmul(mul.input(), mul.shared()))
    ed = Chain(P, "rate_edadd_s", wl=wl)
    x, y, t = ed.inputs(3)
    d = ed.shared()
    ed.output(ed.modadd(ed.modmul(ed.modmul(x, y), d), t))
    ed4 = Chain(P, "rate_edadd_4", wl=wl)
    x, y, t, d = ed4.inputs(4)
    ed4.output(ed4.modadd(ed4.modmul(ed4.modmul(x, y), d), t))
    return {"mul_shared": mul, "edadd_shared": ed, "edadd_batch": ed4}


def build_all(primes, wls):
    """every plug-in the measurement loads (hipcc: where the tree is built, before the GPU is used)"""
    return {(P, wl): {k: ch.build() for k, ch in chains(P, wl).items()} for P in primes for wl in wls}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--primes", default=",".join(PRIMES))
    ap.add_argument("--wl", default="64,32")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_shared_rate.json"))
    args = ap.parse_args()
    primes, wls = args.primes.split(","), [int(w) for w in args.wl.split(",")]
    built = build_all(primes, wls)
    if args.build_only:
        return 0
    import torch
    assert torch.cuda.is_available(), "chain_shared_rate.py measures on the GPU: no device, no number"
    from modarith_amd.field import Field
    n = 1 << args.log2n
    report = {"n": n, "tile": args.tile, "launches": args.launches, "rounds": args.rounds, "warm_up_s": WARM_S, "hbm_peak_Bps": HBM_PEAK,
              "device": torch.cuda.get_device_name(0), "predicted_shared_over_batch": 0.8,
              "timing": "device events around each launch, variants alternating on the same buffers; a reading is the median of the launches of one "
                        "round; spread = largest relative difference between the baseline's (edadd_batch) readings", "cases": {}}
    failed = []
    for P in primes:
        for wl in wls:
            F = Field(P, wl=wl, tile=args.tile)
            f = built[(P, wl)]
            w = wl // 8
            x, y, t = (F.nres(F.uniform(n, seed=31, array=k)) for k in range(3))
            b = F.to_limbs(F.nres(F.uniform(1, seed=31, array=7)))[0]
            col = F.from_limbs([b])
            B = col.reshape(1, F.N, 1).expand(n // args.tile, F.N, args.tile).contiguous()
            z = F.empty(n)
            runs = [("mul_shared", 2, lambda: f["mul_shared"](x, b, out=[z])),
                    ("modmul_broadcast", 3, lambda: F.modmul(x, B, out=z)),
                    ("edadd_shared", 4, lambda: f["edadd_shared"](x, y, t, b, out=[z])),
                    ("edadd_batch", 5, lambda: f["edadd_batch"](x, y, t, B, out=[z]))]
            if wl == 64:
                runs.insert(1, ("modmuls", 2, lambda: F.modmuls(x, b, out=z)))
            # the numbers are of kernels that compute what they stand for
            want = F.modmul(x, B)
            for k in ("mul_shared", "modmuls", "modmul_broadcast"):
                run = dict((r[0], r[2]) for r in runs).get(k)
                if run is not None:
                    z.zero_()
                    run()
                    assert torch.equal(z, want), (P, wl, k)
            want = F.modadd(F.modmul(F.modmul(x, y), B), t)
            for k in ("edadd_shared", "edadd_batch"):
                z.zero_()
                dict((r[0], r[2]) for r in runs)[k]()
                assert torch.equal(z, want), (P, wl, k)
            del want
            for _, _, run in runs:                             # every shape warmed for at least 60 ms and three launches
                t0, k = time.perf_counter(), 0
                while k < 3 or time.perf_counter() - t0 < WARM_S:
                    run()
                    torch.cuda.synchronize()
                    k += 1
            readings = {k: [] for k, _, _ in runs}
            for _ in range(args.rounds):
                ev = {k: [] for k, _, _ in runs}
                for _ in range(args.launches):
                    for k, _, run in runs:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        run()
                        e1.record()
                        ev[k].append((e0, e1))
                torch.cuda.synchronize()
                for k, v in ev.items():
                    readings[k].append(statistics.median(a.elapsed_time(c) for a, c in v))
            ms = {k: statistics.median(v) for k, v in readings.items()}
            bytes_per = {k: arrays * F.N * w for k, arrays, _ in runs}
            base = readings["edadd_batch"]
            spread = (max(base) - min(base)) / min(base)
            ratio = ms["edadd_shared"] / ms["edadd_batch"]
            per = {"nlimbs": F.N, "bytes_per_element": bytes_per, "readings_ms": readings, "ms": ms,
                   "hbm_share_over_own_bytes": {k: bytes_per[k] * n / (ms[k] * 1e-3) / HBM_PEAK for k in ms},
                   "edadd_shared_over_batch": ratio, "baseline_spread": spread, "shared_not_slower_than_batch": ratio <= 1.0 + spread,
                   "mul_shared_over_modmul_broadcast": ms["mul_shared"] / ms["modmul_broadcast"]}
            if wl == 64:
                per["mul_shared_over_modmuls"] = ms["mul_shared"] / ms["modmuls"]
            report["cases"]["%s/w%d" % (P, wl)] = per
            if not per["shared_not_slower_than_batch"]:
                failed.append("%s/w%d" % (P, wl))
            sh = per["hbm_share_over_own_bytes"]
            print("%-8s w%d  x*b shared %.3f ms (%.3f)%s | modmul broadcast %.3f ms (%.3f) || edadd shared %.3f ms (%.3f) | fourth batch %.3f ms (%.3f) | "
                  "shared / batch %.3f (bytes: 0.800; spread %.3f)" % (
                      P, wl, ms["mul_shared"], sh["mul_shared"], " | modmuls %.3f ms (%.3f)" % (ms["modmuls"], sh["modmuls"]) if wl == 64 else "",
                      ms["modmul_broadcast"], sh["modmul_broadcast"], ms["edadd_shared"], sh["edadd_shared"], ms["edadd_batch"], sh["edadd_batch"],
                      ratio, spread), flush=True)
            del x, y, t, B, z
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.out)
    if failed:                                                 # the requirement of this tool
        print("FAILED: the shared form is slower than the fourth-batch form by more than the run's spread for " + ", ".join(failed))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
