#!/usr/bin/env python3
"""Rate of the entry points that end in a shared inversion (csrc/shared_inv.h), this checkout's library against another build's (GPU box).

  python tools/shared_inv_rate.py --parent OTHER/libmodarith_amd.so [--repeats 5] [--out profiles/shared_inv_one_walk.json]

Legs: rfc7748_X25519_batch_ws, rfc7748_X448_batch_ws, ecn_<c>_mul_get_batch and ecn_<c>_mul2_get_batch for ed25519, ed448, nist256,
secp256k1, at n = 2^20 records and at 4 * 65536 + 4099.  Each library runs in fresh child processes of its own (MA_LIB selects it), parent
and new alternating -- parent, new, parent, new, ... --, `repeats` of each in this one command; a child times every leg with device
events after warm-up (median of 5 launches) on inputs from a fixed seed and hashes what the leg wrote.
  * Every child's hashes must agree: both libraries write the same bytes.
  * Margin: the parent's own run-to-run spread in this command, max over min of its children's medians, per leg.  A leg passes where the
    median of the new library's children is at most the median of the parent's times that spread.
Medians, spreads and verdicts go under "rate" into --out (beside the object-code figures of tools/comb_objects.py where the file
exists).  Exit status 1 where the bytes differ or a leg misses its margin."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = (1 << 20, 4 * 65536 + 4099)
CURVES = ("ED25519", "ED448", "NIST256", "SECP256K1")
LAUNCHES, WARM = 5, 2


def child(out_path):
    sys.path.insert(0, ROOT)
    import torch
    from modarith_amd.edwards import Curve
    from modarith_amd.field import rfc7748
    dev = torch.device("cuda", 0)
    res = {}

    def leg(name, fn):
        for _ in range(WARM):
            out = fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(LAUNCHES):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        h = hashlib.sha256()
        for t in (out if isinstance(out, tuple) else (out,)):
            h.update(t.cpu().numpy().tobytes())
        res[name] = {"ms": statistics.median(ms), "sha256": h.hexdigest()}
        print("%-40s %9.3f ms" % (name, res[name]["ms"]), flush=True)

    for n in SIZES:
        g = torch.Generator(device=dev).manual_seed(20260 + n)
        rnd = lambda nb: torch.randint(0, 256, (n, nb), dtype=torch.uint8, device=dev, generator=g)
        for curve, nb in (("X25519", 32), ("X448", 56)):
            k, u = rnd(nb), rnd(nb)
            u[::1000] = 0                                           # low-order inputs: z2 = 0 among the records
            leg("rfc7748_%s_batch_ws n=%d" % (curve, n), lambda: rfc7748(curve, k, u))
        for name in CURVES:
            Cv = Curve(name, dev)
            e, f = rnd(Cv.nbytes), rnd(Cv.nbytes)
            G = Cv.gen(n)
            Q = Cv.mul(rnd(Cv.nbytes), G.clone())
            leg("ecn_%s_mul_get_batch n=%d" % (name.lower(), n), lambda: Cv.mul_get(e, Q))
            leg("ecn_%s_mul2_get_batch n=%d" % (name.lower(), n), lambda: Cv.mul2_get(e, G, f, Q))
            del Cv, e, f, G, Q
            torch.cuda.empty_cache()
    with open(out_path, "w") as fo:
        json.dump(res, fo)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", help="the other build's libmodarith_amd.so")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_inv_one_walk.json"))
    ap.add_argument("--child", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    assert args.parent and os.path.exists(args.parent), "--parent: the other build's library"
    assert args.repeats >= 5, "at least five children per library"
    libs = {"parent": os.path.abspath(args.parent), "new": os.path.join(ROOT, "modarith_amd", "libmodarith_amd.so")}
    runs = {"parent": [], "new": []}
    with tempfile.TemporaryDirectory() as tmp:
        for rep in range(args.repeats):
            for which in ("parent", "new"):
                path = os.path.join(tmp, "%s_%d.json" % (which, rep))
                print("== %s, child %d" % (which, rep), flush=True)
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path], env=dict(os.environ, MA_LIB=libs[which]), check=True, timeout=900)
                runs[which].append(json.load(open(path)))
    legs, ok = {}, True
    for name in runs["parent"][0]:
        hashes = {r[name]["sha256"] for rs in runs.values() for r in rs}
        p, q = [r[name]["ms"] for r in runs["parent"]], [r[name]["ms"] for r in runs["new"]]
        spread = max(p) / min(p)
        legs[name] = {"parent_ms": p, "new_ms": q, "parent_median_ms": statistics.median(p), "new_median_ms": statistics.median(q),
                      "parent_spread_max_over_min": spread, "new_over_parent": statistics.median(q) / statistics.median(p),
                      "same_bytes": len(hashes) == 1, "within_parent_spread": statistics.median(q) <= statistics.median(p) * spread}
        ok = ok and legs[name]["same_bytes"] and legs[name]["within_parent_spread"]
        print("%-40s parent %9.3f ms  new %9.3f ms  x%.4f  spread %.4f  %s%s" % (
            name, legs[name]["parent_median_ms"], legs[name]["new_median_ms"], legs[name]["new_over_parent"], spread,
            "ok" if legs[name]["within_parent_spread"] else "OUTSIDE", "" if legs[name]["same_bytes"] else "  BYTES DIFFER"), flush=True)
    out = json.load(open(args.out)) if os.path.exists(args.out) else {}
    out["rate"] = {"timing": "device events around single calls after %d warm-up calls, median of %d per child; fresh child processes, parent and new "
                             "alternating, %d of each in one command" % (WARM, LAUNCHES, args.repeats),
                   "margin": "per leg, the parent's own spread in the same command (max over min of its children's medians)",
                   "legs": legs, "all_same_bytes": all(l["same_bytes"] for l in legs.values()), "all_within_parent_spread": all(l["within_parent_spread"] for l in legs.values())}
    with open(args.out, "w") as fo:
        json.dump(out, fo, indent=1, sort_keys=True)
    print("all legs: same bytes and within the parent's spread:", ok, "-> wrote", args.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
