#!/usr/bin/env python3
"""Rate of the fused chains that speak bytes -- modimp at the head and modexp at the tail inside the kernel -- through both ways to the
bytes of csrc/chain.inc, beside the same calls one by one, in ONE process (GPU box).

At word lengths 64 and 32, 2^24 elements, record arrays as torch allocates them (16-byte aligned), element batches on tiles of 4096:

 (1) `bytes a, b; outbytes modmul(a, b)` over X25519, NIST256 and X448 (3 Nbytes an element): the fused kernel on the STAGED path (a
     workgroup moves its records through an LDS image with 16-byte coalesced accesses) and on the DIRECT path (every lane reads and
     writes its own records), forced through MA_CHAIN_BYTES; the four calls through Field (modimp x 2, modmul, modexp); and Field.modmul
     alone on the imported batches (3 N w bytes) for the share of the HBM peak a plain streaming kernel reaches in this run;
 (2) modarith_amd.fuse.pubkey_chain over NIST256 (two coordinate records in, one int32 out: 2 Nbytes + 4) on both paths, beside
     modimp x 2 followed by the built oncurve_chain and the `&` of the three ints.

Records are uniform random bytes (X25519: about half of them spell an integer that is not below p).  Every fused output, on either
path, is compared with the call-by-call bytes before anything is timed.  Every variant is warmed for at least 60 ms (and three launches),
then timed ALTERNATING on the same buffers, each launch singly between device events; the median of 20 launches is one reading, three
readings, their median is the figure.

The tool exits 1 unless
  * the shipped path (modarith_amd.fuse.BYTES_IO_DEFAULT, what a call without MA_CHAIN_BYTES takes) is at least 2x faster than call by
    call for every chain measured (the standing rule for chains), and
  * the shipped path of each word length is the one these numbers pick: the path with the lower total over the chains of that word
    length (the sum of their figures) -- unless the two totals differ by less than the run's own spread, the largest relative
    difference between the three readings of one fused variant at that word length; then DIRECT ships: less code runs.
No other threshold: the share of the peak and the ratio to modmul are reported.

As measured (profiles/chain_bytes_rate.json; docs/fused_chains.md, "Chains that speak bytes"): direct is picked and shipped at both word
lengths (13.5 % and 5.4 % ahead over all chains), and the tool EXITS 1 on the first condition for four cases.  Call by call / shipped at
64 / 32 bits: modmul X25519 2.41 / 2.47, X448 2.19 / 2.39, NIST256 1.96 / 1.86, public-key check 1.36 / 1.25 -- over P-256 the kernels
are bound by the Montgomery products of nres and redc, which fusing does not remove, and neither path reaches 2x there.

  python tools/chain_bytes_rate.py [--log2n 24] [--launches 20] [--rounds 3] [--out profiles/chain_bytes_rate.json] [--doc docs/fused_chains.md]
  python tools/chain_bytes_rate.py --build-only                                   (hipcc only: the plug-ins the measurement loads)
  python tools/chain_bytes_rate.py --table-from profiles/chain_bytes_rate.json    (no GPU: rewrite the table of the document from a report)
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
HBM_PEAK = 8.0e12
REQUIRED = 2.0
PRIMES = ("X25519", "NIST256", "X448")
BMUL = "bytes a, b; outbytes modmul(a, b)"
BEGIN, END = "<!-- chain_bytes_rate: table written by tools/chain_bytes_rate.py -->", "<!-- chain_bytes_rate: end -->"


def build_all(wls):
    """every plug-in the measurement loads (hipcc: where the tree is built, before the GPU is used)"""
    from modarith_amd.fuse import oncurve_chain, parse, pubkey_chain
    out = {}
    for wl in wls:
        out[wl] = {"bmul/" + P: (parse(P, "rate_bmul", BMUL, wl=wl).build(), None) for P in PRIMES}
        pk, (b,) = pubkey_chain("NIST256", wl, name="rate_pubkey")
        on, _ = oncurve_chain("NIST256", wl, name="rate_oncurve")
        out[wl]["pubkey/NIST256"] = (pk.build(), (b, on.build()))
    return out


def forced(path, run):
    def go():
        os.environ["MA_CHAIN_BYTES"] = path
        try:
            return run()
        finally:
            del os.environ["MA_CHAIN_BYTES"]
    return go


def summarise(readings, bytes_per, n):
    ms = {k: statistics.median(v) for k, v in readings.items()}
    spread = max((max(readings[k]) - min(readings[k])) / min(readings[k]) for k in ("staged", "direct"))
    return {"readings_ms": readings, "ms": ms, "bytes_per_element": bytes_per, "spread_of_fused_readings": spread,
            "hbm_share_over_own_bytes": {k: bytes_per[k] * n / (ms[k] * 1e-3) / HBM_PEAK for k in ms if k in bytes_per},
            "calls_over_staged": ms["calls"] / ms["staged"], "calls_over_direct": ms["calls"] / ms["direct"]}


def bmul(torch, F, f, n, args, measure):
    g = torch.Generator(device="cuda").manual_seed(101)
    A, B = (torch.randint(0, 256, (n, F.nbytes), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
    out = torch.empty_like(A)
    a, fa = F.modimp(A)
    b, _ = F.modimp(B)
    z = F.empty(n)

    def calls():
        x, _ = F.modimp(A)
        y, _ = F.modimp(B)
        F.modmul(x, y, out=x)
        return F.modexp(x)

    want = calls()
    for path in ("staged", "direct"):
        out.zero_()
        forced(path, lambda: f(A, B, out=[out]))()
        assert torch.equal(out, want), "the fused bytes on the %s path differ from the call sequence" % path
    below = int(fa.sum())
    del want
    torch.cuda.empty_cache()
    runs = [("staged", forced("staged", lambda: f(A, B, out=[out]))), ("direct", forced("direct", lambda: f(A, B, out=[out]))),
            ("calls", calls), ("modmul", lambda: F.modmul(a, b, out=z))]
    readings = measure(torch, runs, args.launches, args.rounds)
    w = F.wl // 8
    per = summarise(readings, {"staged": f.chain.traffic_bytes(), "direct": f.chain.traffic_bytes(), "calls": f.chain.unfused_traffic_bytes(), "modmul": 3 * F.N * w}, n)
    per.update(nlimbs=F.N, nbytes=F.nbytes, below_p=below)
    per["staged_over_modmul"], per["direct_over_modmul"] = per["ms"]["staged"] / per["ms"]["modmul"], per["ms"]["direct"] / per["ms"]["modmul"]
    return per


def pubkey(torch, F, f, extra, n, args, measure):
    b, on = extra
    g = torch.Generator(device="cuda").manual_seed(103)
    X, Y = (torch.randint(0, 256, (n, F.nbytes), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
    # half of the keys on the curve: y = sqrt(x^3 - 3x + b) where that is a residue, exported back into the records
    x, _ = F.modimp(X[: n // 2].contiguous())
    Bb = F.from_limbs([b]).reshape(1, F.N, 1).expand(n // 2 // args.tile, F.N, args.tile).contiguous()
    y = F.modsqrt(F.modadd(F.modsub(F.modmul(F.modsqr(x), x), F.modmli(x, 3)), Bb))
    Y[: n // 2] = F.modexp(y)
    del x, y, Bb
    ok = torch.empty(n, dtype=torch.int32, device="cuda")

    def calls():
        (x, fx), (y, fy) = F.modimp(X), F.modimp(Y)
        return fx & fy & on(x, y, b)[0]

    want = calls()
    for path in ("staged", "direct"):
        ok.zero_()
        forced(path, lambda: f(X, Y, b, out=[ok]))()
        assert torch.equal(ok, want), "the fused int on the %s path differs from the call sequence" % path
    good = int(want.sum())
    assert 0.1 * n < good < 0.4 * n, "about a quarter of the keys should pass (got %d of %d)" % (good, n)
    del want
    torch.cuda.empty_cache()
    runs = [("staged", forced("staged", lambda: f(X, Y, b, out=[ok]))), ("direct", forced("direct", lambda: f(X, Y, b, out=[ok]))), ("calls", calls)]
    readings = measure(torch, runs, args.launches, args.rounds)
    w = F.wl // 8
    calls_bytes = 2 * (F.nbytes + F.N * w + 4) + on.chain.traffic_bytes() + 16          # (the two `&`: three int arrays in, one out, at the least)
    per = summarise(readings, {"staged": f.chain.traffic_bytes(), "direct": f.chain.traffic_bytes(), "calls": calls_bytes}, n)
    per.update(nlimbs=F.N, nbytes=F.nbytes, valid_keys=good)
    return per


def decide(report, shipped):
    """per word length: the totals of both paths over the chains measured, the run's spread, the path the rule picks and the one shipped"""
    out = {}
    for wl in sorted({k.split("/")[2] for k in report["cases"]}):
        cs = [c for k, c in report["cases"].items() if k.endswith("/" + wl)]
        tot = {p: sum(c["ms"][p] for c in cs) for p in ("staged", "direct")}
        spread = max(c["spread_of_fused_readings"] for c in cs)
        gap = abs(tot["staged"] - tot["direct"]) / min(tot.values())
        pick = "direct" if gap < spread or tot["direct"] <= tot["staged"] else "staged"
        out[wl] = {"total_ms": tot, "relative_gap": gap, "spread": spread, "picked": pick, "shipped": shipped[int(wl[1:])],
                   "direct_over_staged": tot["direct"] / tot["staged"]}
    return out


def table(report):
    """the table of docs/fused_chains.md, from a report"""
    L = [BEGIN, "",
         "%s, %d elements, median of %d launches, %d readings (tools/chain_bytes_rate.py, profiles/chain_bytes_rate.json):" % (
             report["device"], report["n"], report["launches"], report["rounds"]), "",
         "| chain | word length | staged ms | direct ms | call by call ms | call by call / shipped | shipped: share of HBM peak over its own bytes | shipped / modmul | modmul: share in the same run |",
         "|---|---|---|---|---|---|---|---|---|"]
    for k, c in report["cases"].items():
        what, P, wl = k.split("/")
        ship = report["decision"][wl]["shipped"]
        name = "`outbytes modmul(a, b)` %s (%d B)" % (P, c["bytes_per_element"]["direct"]) if what == "bmul" else "P-256 public-key check (%d B)" % c["bytes_per_element"]["direct"]
        L.append("| %s | %s | %.3f | %.3f | %.3f | %.2f | %.3f | %s | %s |" % (
            name, wl[1:], c["ms"]["staged"], c["ms"]["direct"], c["ms"]["calls"], c["ms"]["calls"] / c["ms"][ship], c["hbm_share_over_own_bytes"][ship],
            "%.2f" % (c["ms"][ship] / c["ms"]["modmul"]) if "modmul" in c["ms"] else "", "%.3f" % c["hbm_share_over_own_bytes"]["modmul"] if "modmul" in c["ms"] else ""))
    L += ["", "| word length | staged, all chains ms | direct, all chains ms | direct / staged | gap | spread of the run | picked | shipped |", "|---|---|---|---|---|---|---|---|"]
    for wl, d in report["decision"].items():
        L.append("| %s | %.3f | %.3f | %.3f | %.1f %% | %.1f %% | %s | %s |" % (wl[1:], d["total_ms"]["staged"], d["total_ms"]["direct"], d["direct_over_staged"],
                                                                          100 * d["relative_gap"], 100 * d["spread"], d["picked"], d["shipped"]))
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
    ap.add_argument("--build-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_bytes_rate.json"))
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
    assert torch.cuda.is_available(), "chain_bytes_rate.py measures on the GPU: no device, no number"
    from chain_pred_rate import WARM_S, measure
    from modarith_amd.field import Field
    from modarith_amd.fuse import BYTES_IO_DEFAULT
    os.environ.pop("MA_CHAIN_BYTES", None)
    n = 1 << args.log2n
    report = {"n": n, "tile": args.tile, "launches": args.launches, "rounds": args.rounds, "warm_up_s": WARM_S, "hbm_peak_Bps": HBM_PEAK,
              "device": torch.cuda.get_device_name(0), "shipped": {"w%d" % wl: BYTES_IO_DEFAULT[wl] for wl in wls},
              "timing": "device events around each launch, variants alternating on the same buffers; a reading is the median of the launches of one "
                        "round, the figure the median of the readings", "cases": {}}
    for wl in wls:
        for key, (f, extra) in built[wl].items():
            what, P = key.split("/")
            F = Field(P, wl=wl, tile=args.tile)
            per = bmul(torch, F, f, n, args, measure) if what == "bmul" else pubkey(torch, F, f, extra, n, args, measure)
            report["cases"]["%s/w%d" % (key, wl)] = per
            print("%-20s staged %.3f ms | direct %.3f ms | call by call %.3f ms (x %.2f / %.2f)%s" % (
                "%s/w%d" % (key, wl), per["ms"]["staged"], per["ms"]["direct"], per["ms"]["calls"], per["calls_over_staged"], per["calls_over_direct"],
                " | modmul %.3f ms" % per["ms"]["modmul"] if "modmul" in per["ms"] else ""), flush=True)
            del F
            torch.cuda.empty_cache()
    report["decision"] = decide(report, BYTES_IO_DEFAULT)
    failed = []
    for wl, d in report["decision"].items():
        print("%s: staged %.3f ms, direct %.3f ms over all chains (gap %.1f %%, spread %.1f %%): picked %s, shipped %s" % (
            wl, d["total_ms"]["staged"], d["total_ms"]["direct"], 100 * d["relative_gap"], 100 * d["spread"], d["picked"], d["shipped"]))
        if d["picked"] != d["shipped"]:
            failed.append("%s ships %s where the numbers pick %s" % (wl, d["shipped"], d["picked"]))
    for k, c in report["cases"].items():
        ship = report["decision"][k.split("/")[2]]["shipped"]
        c["calls_over_shipped"], c["required"] = c["ms"]["calls"] / c["ms"][ship], REQUIRED
        if c["calls_over_shipped"] < REQUIRED:
            failed.append("%s: the shipped path is %.2fx faster than call by call (required: %.1f)" % (k, c["calls_over_shipped"], REQUIRED))
    report["failed"] = failed
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.out)
    if os.path.exists(args.doc):
        write_table(args.doc, report)
    for msg in failed:
        print("FAILED:", msg)
    return 1 if failed else 0


if __name__ == "__main__":
    sys.exit(main())
