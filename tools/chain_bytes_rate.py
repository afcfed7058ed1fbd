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

With --le the tool measures the LITTLE-ENDIAN records instead (profiles/chain_le_rate.json, the table "chain_le_rate" of the document):
`lebytes a, b; outlebytes modmul(a, b)` -- the body of (1), records least significant byte first: no bswap, the same traffic -- over
X25519 and NIST256 at both word lengths and through both ways to the bytes, ALTERNATING in the same run with the big-endian chain of (1)
on the same buffers and with the sequence a caller runs today (torch.flip x 2, modimp x 2, modmul, modexp, torch.flip).  Recorded per
case: little-endian / big-endian per path beside the spread of the run's three readings (the kernel does strictly less work: the ratio
is expected within that spread of 1), the big-endian figures against those the parent's profiles/chain_bytes_rate.json records (the
shared frame did not move them), and call by call / shipped path, which the standing rule wants at 2 or more.  Then
modarith_amd.fuse.rfc8032_decode_chain beside decompress_chain on the values the records spell: three exponentiations, no threshold,
reported.  Exits 1 where a little-endian kernel is SLOWER than its big-endian twin by more than the spread, or the 2x rule fails.

  python tools/chain_bytes_rate.py --le [--le-out profiles/chain_le_rate.json]     (GPU; --build-only and --table-from work with it)
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
LE_PRIMES = ("X25519", "NIST256")
LMUL = "lebytes a, b; outlebytes modmul(a, b)"
LE_BEGIN, LE_END = "<!-- chain_le_rate: table written by tools/chain_bytes_rate.py --le -->", "<!-- chain_le_rate: end -->"


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


# ---------------------------------------------------------------------------------------------------------------- little-endian records
def build_le(wls):
    from modarith_amd.fuse import decompress_chain, parse, rfc8032_decode_chain
    out = {}
    for wl in wls:
        out[wl] = {"lmul/" + P: (parse(P, "rate_lmul", LMUL, wl=wl).build(), parse(P, "rate_bmul", BMUL, wl=wl).build()) for P in LE_PRIMES}
        dec, (d,) = rfc8032_decode_chain("ED25519", wl, name="rate_rfc8032_decode")
        dc, _ = decompress_chain("ED25519", wl, name="rate_decompress")
        out[wl]["decode/X25519"] = (dec.build(), (dc.build(), d))
    return out


def lmul(torch, F, fle, fbe, n, args, measure, parent):
    g = torch.Generator(device="cuda").manual_seed(101)
    A, B = (torch.randint(0, 256, (n, F.nbytes), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
    out = torch.empty_like(A)

    def calls():                                                 # what a caller of little-endian records runs today
        x, _ = F.modimp(torch.flip(A, [1]))
        y, _ = F.modimp(torch.flip(B, [1]))
        F.modmul(x, y, out=x)
        return torch.flip(F.modexp(x), [1])

    want = calls()
    bwant = F.modexp(F.modmul(F.modimp(A)[0], F.modimp(B)[0]))
    for path in ("staged", "direct"):
        for f, w, what in ((fle, want, "little"), (fbe, bwant, "big")):
            out.zero_()
            forced(path, lambda: f(A, B, out=[out]))()
            assert torch.equal(out, w), "the fused %s-endian bytes on the %s path differ from the call sequence" % (what, path)
    del want, bwant
    torch.cuda.empty_cache()
    fused = [("%s_%s" % (e, path), forced(path, lambda f=f: f(A, B, out=[out]))) for path in ("staged", "direct") for e, f in (("le", fle), ("be", fbe))]
    readings = measure(torch, fused + [("calls", calls)], args.launches, args.rounds)
    ms = {k: statistics.median(v) for k, v in readings.items()}
    spread = max((max(readings[k]) - min(readings[k])) / min(readings[k]) for k, _ in fused)
    per = {"readings_ms": readings, "ms": ms, "spread_of_fused_readings": spread, "nbytes": F.nbytes,
           "bytes_per_element": {"fused": fle.chain.traffic_bytes(), "calls": fle.chain.unfused_traffic_bytes()},
           "le_over_be": {path: ms["le_" + path] / ms["be_" + path] for path in ("staged", "direct")},
           "be_recorded_by_parent_ms": {path: parent["ms"][path] for path in ("staged", "direct")} if parent else None,
           "be_over_parent": {path: ms["be_" + path] / parent["ms"][path] for path in ("staged", "direct")} if parent else None}
    per["le_within_spread_of_be"] = {path: abs(r - 1) <= spread for path, r in per["le_over_be"].items()}
    per["be_within_spread_of_parent"] = {path: abs(r - 1) <= spread for path, r in per["be_over_parent"].items()} if parent else None
    return per


def decode(torch, F, f, extra, n, args, measure):
    dc, d = extra
    g = torch.Generator(device="cuda").manual_seed(107)
    R = torch.randint(0, 256, (n, F.nbytes), dtype=torch.uint8, device="cuda", generator=g)
    masked = torch.flip(R, [1]).contiguous()
    masked[:, 0] &= 0x7f
    s = (R[:, -1] >> 7).to(torch.int32)
    y, fy = F.modimp(masked)
    del masked
    outs = [F.empty(n) for _ in range(3)] + [torch.empty(n, dtype=torch.int32, device="cuda")]
    outs2 = [F.empty(n) for _ in range(3)] + [torch.empty(n, dtype=torch.int32, device="cuda")]
    f(R, d, out=outs)
    dc(y, d, s, out=outs2)
    agree = fy == 1                                              # (where y was not below p the decode chain answers the neutral element)
    assert torch.equal(outs[3][agree], outs2[3][agree]) and torch.equal(F.to_flat(outs[0])[:, agree], F.to_flat(outs2[0])[:, agree]), "decode differs from decompress"
    readings = measure(torch, [("decode", lambda: f(R, d, out=outs)), ("decompress", lambda: dc(y, d, s, out=outs2))], args.launches, args.rounds)
    ms = {k: statistics.median(v) for k, v in readings.items()}
    return {"readings_ms": readings, "ms": ms, "decode_over_decompress": ms["decode"] / ms["decompress"], "points": int(outs[3].sum()),
            "bytes_per_element": {"decode": f.chain.traffic_bytes(), "decompress": dc.chain.traffic_bytes()}}


def le_table(report):
    L = [LE_BEGIN, "",
         "%s, %d elements, median of %d launches, %d readings (tools/chain_bytes_rate.py --le, profiles/chain_le_rate.json):" % (
             report["device"], report["n"], report["launches"], report["rounds"]), "",
         "| `outlebytes modmul(a, b)` | word length | LE staged ms | BE staged ms | LE / BE | LE direct ms | BE direct ms | LE / BE | spread of the run | BE now / parent's record (staged, direct) | call by call ms | call by call / shipped |",
         "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for k, c in report["cases"].items():
        what, P, wl = k.split("/")
        if what != "lmul":
            continue
        m = c["ms"]
        par = "%.3f, %.3f" % (c["be_over_parent"]["staged"], c["be_over_parent"]["direct"]) if c["be_over_parent"] else ""
        L.append("| %s (%d B) | %s | %.3f | %.3f | %.3f | %.3f | %.3f | %.3f | %.1f %% | %s | %.3f | %.2f |" % (
            P, c["bytes_per_element"]["fused"], wl[1:], m["le_staged"], m["be_staged"], c["le_over_be"]["staged"], m["le_direct"], m["be_direct"], c["le_over_be"]["direct"],
            100 * c["spread_of_fused_readings"], par, m["calls"], c["calls_over_shipped"]))
    L += ["", "| `rfc8032_decode_chain` | word length | decode ms (records in) | `decompress_chain` ms (limbs and signs in) | decode / decompress |", "|---|---|---|---|---|"]
    for k, c in report["cases"].items():
        what, P, wl = k.split("/")
        if what == "decode":
            L.append("| ED25519 (%d B against %d B) | %s | %.3f | %.3f | %.3f |" % (c["bytes_per_element"]["decode"], c["bytes_per_element"]["decompress"], wl[1:],
                                                                                 c["ms"]["decode"], c["ms"]["decompress"], c["decode_over_decompress"]))
    return "\n".join(L + ["", LE_END])


def main_le(args, wls):
    built = build_le(wls)
    if args.build_only:
        return 0
    import torch
    assert torch.cuda.is_available(), "chain_bytes_rate.py measures on the GPU: no device, no number"
    from chain_pred_rate import WARM_S, measure
    from modarith_amd.field import Field
    from modarith_amd.fuse import BYTES_IO_DEFAULT
    os.environ.pop("MA_CHAIN_BYTES", None)
    n = 1 << args.log2n
    recorded = json.load(open(args.out))["cases"] if os.path.exists(args.out) else {}
    report = {"n": n, "tile": args.tile, "launches": args.launches, "rounds": args.rounds, "warm_up_s": WARM_S, "device": torch.cuda.get_device_name(0),
              "shipped": {"w%d" % wl: BYTES_IO_DEFAULT[wl] for wl in wls}, "parent_record": os.path.relpath(args.out, ROOT),
              "timing": "device events around each launch, variants alternating on the same buffers; a reading is the median of the launches of one "
                        "round, the figure the median of the readings", "cases": {}}
    failed = []
    for wl in wls:
        for key, (f, extra) in built[wl].items():
            what, P = key.split("/")
            F = Field(P, wl=wl, tile=args.tile)
            name = "%s/w%d" % (key, wl)
            if what == "lmul":
                per = lmul(torch, F, f, extra, n, args, measure, recorded.get("bmul/%s/w%d" % (P, wl)))
                ship = BYTES_IO_DEFAULT[wl]
                per["calls_over_shipped"], per["required"] = per["ms"]["calls"] / per["ms"]["le_" + ship], REQUIRED
                print("%-18s LE staged %.3f direct %.3f | BE staged %.3f direct %.3f | LE / BE %.3f %.3f (spread %.1f %%) | call by call %.3f ms (x %.2f)" % (
                    name, per["ms"]["le_staged"], per["ms"]["le_direct"], per["ms"]["be_staged"], per["ms"]["be_direct"], per["le_over_be"]["staged"],
                    per["le_over_be"]["direct"], 100 * per["spread_of_fused_readings"], per["ms"]["calls"], per["calls_over_shipped"]), flush=True)
                if per["calls_over_shipped"] < REQUIRED:
                    failed.append("%s: the shipped path is %.2fx faster than call by call (required: %.1f)" % (name, per["calls_over_shipped"], REQUIRED))
                for path, r in per["le_over_be"].items():
                    if r - 1 > per["spread_of_fused_readings"]:
                        failed.append("%s: little-endian %s is %.1f %% slower than big-endian (spread %.1f %%)" % (name, path, 100 * (r - 1), 100 * per["spread_of_fused_readings"]))
            else:
                per = decode(torch, F, f, extra, n, args, measure)
                print("%-18s decode %.3f ms | decompress %.3f ms (x %.3f)" % (name, per["ms"]["decode"], per["ms"]["decompress"], per["decode_over_decompress"]), flush=True)
            report["cases"][name] = per
            del F
            torch.cuda.empty_cache()
    report["failed"] = failed
    os.makedirs(os.path.dirname(os.path.abspath(args.le_out)), exist_ok=True)
    with open(args.le_out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.le_out)
    if os.path.exists(args.doc):
        write_table(args.doc, report, le_table, LE_BEGIN, LE_END)
    for msg in failed:
        print("FAILED:", msg)
    return 1 if failed else 0


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


def write_table(doc, report, table=table, BEGIN=BEGIN, END=END):
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
    ap.add_argument("--le", action="store_true", help="measure the little-endian records (see the head of this file)")
    ap.add_argument("--le-out", default=os.path.join(ROOT, "profiles", "chain_le_rate.json"))
    args = ap.parse_args()
    if args.table_from:
        if args.le:
            write_table(args.doc, json.load(open(args.table_from)), le_table, LE_BEGIN, LE_END)
        else:
            write_table(args.doc, json.load(open(args.table_from)))
        return 0
    wls = [int(w) for w in args.wl.split(",")]
    if args.le:
        return main_le(args, wls)
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
