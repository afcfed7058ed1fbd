#!/usr/bin/env python3
"""Rate of the fused chains that decide -- ints computed inside the chain -- beside the same calls one by one, in ONE process (GPU box).

At word lengths 64 and 32, 2^24 elements on tiles of 4096:

 (1) the predicate-only chain "is (x, y) on P-256" (modarith_amd.fuse.oncurve_chain: modcmp(y^2, x^3 - 3x + b), b shared, one int32 per
     element out and no limb array: 2 N w + 4 bytes an element) beside the seven calls through Field that compute the same int, and
     beside Field.modmul on the same batches (3 N w bytes) for the share of the HBM peak a plain streaming kernel reaches in this run;
 (2) the ED25519 decompression chain (modarith_amd.fuse.decompress_chain: edwards.c:290-334 with one progenitor, a computed sign
     selector and the failure turned into the neutral element) beside the same calls through Field and beside Curve.set, which starts
     from the bytes of y (its modimp is part of what it does).  Three exponentiations per element: VALU-bound, no threshold.

The inputs of (1) are x uniform and y = modsqrt(x^3 - 3x + b): on the curve where that is a residue (about half), off it elsewhere; of
(2) y uniform (about half have an x) and random signs.  Every fused result is compared with the call-by-call one before anything is
timed.  Every variant is warmed for at least 60 ms (and three launches), then timed ALTERNATING on the same buffers, each launch singly
between device events; the median of 20 launches is one reading, three readings, their median is the figure.
REQUIRED (the standing rule for chains): the predicate-only chain is at least 2x faster than call by call -- the tool exits 1 otherwise.

  python tools/chain_pred_rate.py [--log2n 24] [--launches 20] [--rounds 3] [--out profiles/chain_pred_rate.json] [--doc docs/fused_chains.md]
  python tools/chain_pred_rate.py --table-from profiles/chain_pred_rate.json      (no GPU: rewrite the table of the document from a report)
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
WARM_S = 0.060
REQUIRED = 2.0
BEGIN, END = "<!-- chain_pred_rate: table written by tools/chain_pred_rate.py -->", "<!-- chain_pred_rate: end -->"


def build_all(wls):
    """every plug-in the measurement loads (hipcc: where the tree is built, before the GPU is used)"""
    from modarith_amd.fuse import decompress_chain, oncurve_chain
    out = {}
    for wl in wls:
        on, (b,) = oncurve_chain("NIST256", wl, name="rate_oncurve")
        de, (d,) = decompress_chain("ED25519", wl, name="rate_decompress")
        out[wl] = {"oncurve": (on.build(), b), "decompress": (de.build(), d)}
    return out


def measure(torch, runs, launches, rounds):
    """{name: [one median per round]}: warm-up, then the variants alternating, each launch between its own events"""
    for _, run in runs:
        t0, k = time.perf_counter(), 0
        while k < 3 or time.perf_counter() - t0 < WARM_S:
            run()
            torch.cuda.synchronize()
            k += 1
    readings = {k: [] for k, _ in runs}
    for _ in range(rounds):
        ev = {k: [] for k, _ in runs}
        for _ in range(launches):
            for k, run in runs:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                ev[k].append((e0, e1))
        torch.cuda.synchronize()
        for k, v in ev.items():
            readings[k].append(statistics.median(a.elapsed_time(c) for a, c in v))
    return readings


def broadcast(F, limbs, n, tile):
    return F.from_limbs([limbs]).reshape(1, F.N, 1).expand(n // tile, F.N, tile).contiguous()


def oncurve(torch, F, f, b, n, args):
    w = F.wl // 8
    Bb = broadcast(F, b, n, args.tile)
    x = F.nres(F.uniform(n, seed=41, array=0))
    rhs = lambda: F.modadd(F.modsub(F.modmul(F.modsqr(x), x), F.modmli(x, 3)), Bb)
    y = F.modsqrt(rhs())
    t1, t2, t3, z = (F.empty(n) for _ in range(4))
    ok = torch.empty(n, dtype=torch.int32, device=x.device)

    def calls():
        F.modsqr(y, out=t1)
        F.modsqr(x, out=t2)
        F.modmul(t2, x, out=t2)
        F.modmli(x, 3, out=t3)
        F.modsub(t2, t3, out=t2)
        F.modadd(t2, Bb, out=t2)
        return F.modcmp(t1, t2)

    f(x, y, b, out=[ok])
    want = calls()
    assert torch.equal(ok, want), "the fused predicate differs from the call sequence"
    on = int(ok.sum())
    assert 0.3 * n < on < 0.7 * n, "about half of the points should be on the curve (got %d of %d)" % (on, n)
    runs = [("fused", lambda: f(x, y, b, out=[ok])), ("calls", calls), ("modmul", lambda: F.modmul(x, y, out=z))]
    readings = measure(torch, runs, args.launches, args.rounds)
    ms = {k: statistics.median(v) for k, v in readings.items()}
    bytes_per = {"fused": 2 * F.N * w + 4, "calls": f.chain.unfused_traffic_bytes(), "modmul": 3 * F.N * w}
    return {"nlimbs": F.N, "on_curve": on, "bytes_per_element": bytes_per, "readings_ms": readings, "ms": ms,
            "hbm_share_over_own_bytes": {k: bytes_per[k] * n / (ms[k] * 1e-3) / HBM_PEAK for k in ms},
            "calls_over_fused": ms["calls"] / ms["fused"], "required": REQUIRED, "meets_required": ms["calls"] / ms["fused"] >= REQUIRED}


def decompress(torch, F, f, d, n, args):
    from modarith_amd.edwards import Curve
    E = Curve("ED25519", wl=F.wl)
    Db = broadcast(F, d, n, args.tile)
    plain = F.uniform(n, seed=43, array=0)
    ybytes = F.modexp(plain)
    y = F.nres(plain)
    del plain
    g = torch.Generator().manual_seed(47)
    s = torch.randint(0, 2, (n,), dtype=torch.int32, generator=g).to(y.device)
    one, zero = F.modone(n), F.modzer(n)
    one = one if one.dim() == 3 else F.to_tiled(one, args.tile)
    zero = zero if zero.dim() == 3 else F.to_tiled(zero, args.tile)
    t = [F.empty(n) for _ in range(6)]
    outs = [F.empty(n) for _ in range(3)] + [torch.empty(n, dtype=torch.int32, device=y.device)]

    def calls():
        Y, U, V, O, H, R = t
        F.modsqr(y, out=Y)
        F.modsub(one, Y, out=U)
        F.modmul(Y, Db, out=V)
        F.modneg(one, out=Y)
        F.modsub(Y, V, out=V)
        F.modsqr(U, out=O)
        F.modmul(U, O, out=U)
        F.modmul(U, V, out=U)                                    # W
        F.modpro(U, out=H)
        ok = F.modqr(H, U)
        F.modsqrt(U, H, out=R)
        F.modinv(U, H, out=V)
        F.modmul(V, R, out=V)
        F.modmul(V, O, out=V)                                    # X
        F.modneg(V, out=R)
        F.modcmv(F.modsign(V) ^ s, R, V)
        bad = 1 - ok
        F.modcpy(y, out=Y)
        return [F.modcmv(bad, zero, V), F.modcmv(bad, one, Y), one, ok]

    f(y, d, s, out=outs)
    want = calls()
    for k in range(4):
        assert torch.equal(outs[k], want[k]), "output %d of the fused decompression differs from the call sequence" % k
    Pt = E.set(s, None, ybytes)
    assert torch.equal(outs[3], 1 - E.isinf(Pt)), "ok differs from Curve.set's point at infinity"
    flat = F.to_flat(outs[0])
    assert torch.equal(F.modexp(outs[0]), F.modexp(Pt[0].contiguous() if flat.shape == Pt[0].shape else F.to_tiled(Pt[0].contiguous(), args.tile))), "x differs from Curve.set"
    have = int(outs[3].sum())
    del Pt, want, flat
    torch.cuda.empty_cache()
    runs = [("fused", lambda: f(y, d, s, out=outs)), ("calls", calls), ("curve_set", lambda: E.set(s, None, ybytes))]
    readings = measure(torch, runs, args.launches, args.rounds)
    ms = {k: statistics.median(v) for k, v in readings.items()}
    return {"nlimbs": F.N, "have_x": have, "bytes_per_element": {"fused": f.chain.traffic_bytes(), "calls": f.chain.unfused_traffic_bytes()},
            "readings_ms": readings, "ms": ms, "elements_per_s": {k: n / (ms[k] * 1e-3) for k in ms},
            "calls_over_fused": ms["calls"] / ms["fused"], "curve_set_over_fused": ms["curve_set"] / ms["fused"]}


def table(report):
    """the table of docs/fused_chains.md, from a report"""
    n = report["n"]
    L = [BEGIN, "",
         "%s, %d elements on tiles of %d, median of %d launches, %d readings (tools/chain_pred_rate.py, profiles/chain_pred_rate.json):" % (
             report["device"], n, report["tile"], report["launches"], report["rounds"]), "",
         "| chain | word length | fused ms | call by call ms | call by call / fused | fused: share of HBM peak over its own bytes | modmul: share in the same run |",
         "|---|---|---|---|---|---|---|"]
    for k, c in report["cases"].items():
        if k.startswith("oncurve"):
            L.append("| P-256 on-curve test (%d B) | %s | %.3f | %.3f | %.2f | %.3f | %.3f |" % (
                c["bytes_per_element"]["fused"], k.split("/")[1][1:], c["ms"]["fused"], c["ms"]["calls"], c["calls_over_fused"],
                c["hbm_share_over_own_bytes"]["fused"], c["hbm_share_over_own_bytes"]["modmul"]))
    L += ["", "| chain | word length | fused ms | call by call ms | Curve.set ms | fused: elements / s | Curve.set: elements / s |", "|---|---|---|---|---|---|---|"]
    for k, c in report["cases"].items():
        if k.startswith("decompress"):
            L.append("| ED25519 decompression | %s | %.2f | %.2f | %.2f | %.3g | %.3g |" % (
                k.split("/")[1][1:], c["ms"]["fused"], c["ms"]["calls"], c["ms"]["curve_set"], c["elements_per_s"]["fused"], c["elements_per_s"]["curve_set"]))
    return "\n".join(L + ["", END])


def write_table(doc, report):
    text = open(doc).read()
    if BEGIN not in text or END not in text:
        raise SystemExit("%s has no table markers (%s ... %s)" % (doc, BEGIN, END))
    head, rest = text.split(BEGIN, 1)
    open(doc, "w").write(head + table(report) + rest.split(END, 1)[1])
    print("wrote the table of", doc)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--tile", type=int, default=4096)
    ap.add_argument("--wl", default="64,32")
    ap.add_argument("--chains", default="oncurve,decompress")
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_pred_rate.json"))
    ap.add_argument("--doc", default=os.path.join(ROOT, "docs", "fused_chains.md"))
    ap.add_argument("--table-from", default=None)
    args = ap.parse_args()
    if args.table_from:
        write_table(args.doc, json.load(open(args.table_from)))
        return 0
    wls = [int(w) for w in args.wl.split(",")]
    built = build_all(wls)
    if args.build_only:
        return 0
    import torch
    assert torch.cuda.is_available(), "chain_pred_rate.py measures on the GPU: no device, no number"
    from modarith_amd.field import Field
    n = 1 << args.log2n
    report = {"n": n, "tile": args.tile, "launches": args.launches, "rounds": args.rounds, "warm_up_s": WARM_S, "hbm_peak_Bps": HBM_PEAK,
              "device": torch.cuda.get_device_name(0),
              "timing": "device events around each launch, variants alternating on the same buffers; a reading is the median of the launches of one "
                        "round, the figure the median of the readings", "cases": {}}
    failed = []
    for which in args.chains.split(","):
        for wl in wls:
            f, shared = built[wl][which]
            F = Field("NIST256" if which == "oncurve" else "X25519", wl=wl, tile=args.tile)
            per = (oncurve if which == "oncurve" else decompress)(torch, F, f, shared, n, args)
            key = "%s/w%d" % (which, wl)
            report["cases"][key] = per
            if which == "oncurve":
                if not per["meets_required"]:
                    failed.append(key)
                sh = per["hbm_share_over_own_bytes"]
                print("%-14s fused %.3f ms (%.3f of the HBM peak over %d B) | call by call %.3f ms | modmul %.3f ms (%.3f) | call by call / fused %.2f (required: %.1f)" % (
                    key, per["ms"]["fused"], sh["fused"], per["bytes_per_element"]["fused"], per["ms"]["calls"], per["ms"]["modmul"], sh["modmul"],
                    per["calls_over_fused"], REQUIRED), flush=True)
            else:
                print("%-14s fused %.2f ms (%.3g elements / s) | call by call %.2f ms | Curve.set %.2f ms (%.3g elements / s)" % (
                    key, per["ms"]["fused"], per["elements_per_s"]["fused"], per["ms"]["calls"], per["ms"]["curve_set"], per["elements_per_s"]["curve_set"]), flush=True)
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.out)
    if os.path.exists(args.doc):
        write_table(args.doc, report)
    if failed:                                                   # the requirement of this tool
        print("FAILED: the predicate-only chain is not %.1fx faster than call by call for %s" % (REQUIRED, ", ".join(failed)))
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
