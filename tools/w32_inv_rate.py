#!/usr/bin/env python3
"""Rate of modinv at word length 32: the shared inversion against one inversion per element (GPU box).

MA_INV_SIMUL is read once per process, so the two paths run in CHILD processes, alternating A B A B (A: the library as it ships, the
shared path; B: MA_INV_SIMUL=0, the per-element kernel -- unchanged by the shared path's arrival).  Each child, per prime: 2^22 elements
of nres(uniform) on tiles of 4096, out of place, three warm-up launches, then `launches` launches timed one by one with device events;
the 64-bit modinv of the same prime on its own buffers in the same process.  The parent takes, per prime and path, the median over
the children of each child's median, and reports elements/s, the ratio shared / per-element and whether it reaches the 4x the
product count (about 265 against about 8 per element) leaves room for at near one wave per SIMD.

  python tools/w32_inv_rate.py [--log2n 22] [--launches 10] [--rounds 2] [--out profiles/w32_inv_rate.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PRIMES = ("X25519", "NIST256", "X448")


def child(args):
    import torch
    assert torch.cuda.is_available(), "w32_inv_rate.py measures on the GPU: no device, no number"
    from modarith_amd import _lib
    from modarith_amd.field import Field
    n = 1 << args.log2n
    out = {}
    for P in args.primes.split(","):
        row = {}
        for wl in (32, 64):
            F = Field(P, wl=wl, tile=args.tile)
            x = F.nres(F.uniform(n, seed=21, array=wl))
            z = F.empty(n)
            for _ in range(3):
                F.modinv(x, out=z)
            torch.cuda.synchronize()
            label = _lib.load().modarith_amd_last_launch().decode()
            ev = []
            for _ in range(args.launches):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                F.modinv(x, out=z)
                e1.record()
                ev.append((e0, e1))
            torch.cuda.synchronize()
            ms = [a.elapsed_time(b) for a, b in ev]
            one = F.to_ints(F.redc(F.modmul(F.to_flat(x)[:, :2].contiguous(), F.to_flat(z)[:, :2].contiguous())))
            assert one == [1, 1], (P, wl, one)
            row["w%d" % wl] = {"launch": label, "ms": ms, "median_ms": statistics.median(ms)}
            del x, z
        out[P] = row
    print("CHILD " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=22)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=2, help="A B pairs of child processes")
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--primes", default=",".join(PRIMES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w32_inv_rate.json"))
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    n = 1 << args.log2n
    runs = {"shared": [], "per_element": []}
    for _ in range(args.rounds):
        for path, knob in (("shared", None), ("per_element", "0")):
            env = dict(os.environ)
            env.pop("MA_INV_SIMUL", None)
            if knob is not None:
                env["MA_INV_SIMUL"] = knob
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--log2n", str(args.log2n), "--launches", str(args.launches),
                                "--tile", str(args.tile), "--primes", args.primes], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
                return 1                                  # a failed child ends the run: nothing more is started on the device
            runs[path].append(json.loads([l for l in p.stdout.splitlines() if l.startswith("CHILD ")][-1][6:]))
    report = {"n": n, "tile": args.tile, "launches": args.launches, "children_per_path": args.rounds, "order": "A B A B (A shared, B MA_INV_SIMUL=0)",
              "timing": "device events around single launches; median per child, then median over children", "primes": {}}
    for P in args.primes.split(","):
        med = lambda path, wl: statistics.median(c[P][wl]["median_ms"] for c in runs[path])
        sh, pe, w64 = med("shared", "w32"), med("per_element", "w32"), med("shared", "w64")
        report["primes"][P] = {
            "shared": {"launch": runs["shared"][0][P]["w32"]["launch"], "median_ms": sh, "elements_per_s": n / (sh * 1e-3), "children_median_ms": [c[P]["w32"]["median_ms"] for c in runs["shared"]]},
            "per_element": {"launch": runs["per_element"][0][P]["w32"]["launch"], "median_ms": pe, "elements_per_s": n / (pe * 1e-3), "children_median_ms": [c[P]["w32"]["median_ms"] for c in runs["per_element"]]},
            "w64_shared": {"launch": runs["shared"][0][P]["w64"]["launch"], "median_ms": w64, "elements_per_s": n / (w64 * 1e-3)},
            "w64_per_element": {"launch": runs["per_element"][0][P]["w64"]["launch"], "median_ms": med("per_element", "w64"), "elements_per_s": n / (med("per_element", "w64") * 1e-3)},
            "ratio_shared_over_per_element": pe / sh, "at_least_4x": pe / sh >= 4.0}
        r = report["primes"][P]
        print("%-8s w32 shared %.3f ms %.3e/s [%s] | per element %.3f ms %.3e/s [%s] | ratio %.2f (>= 4: %s) | w64 shared %.3e/s, per element %.3e/s" % (
            P, sh, r["shared"]["elements_per_s"], r["shared"]["launch"], pe, r["per_element"]["elements_per_s"], r["per_element"]["launch"],
            pe / sh, r["at_least_4x"], r["w64_shared"]["elements_per_s"], r["w64_per_element"]["elements_per_s"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(report, f, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
