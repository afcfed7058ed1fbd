#!/usr/bin/env python3
"""Rates of the batched hashes (modarith_amd.hash) and what they buy the Ed448 flows, in ONE process (GPU box).

  python tools/hash_rate.py [--out profiles/hash_rate.json] [--log2n 20] [--log2n-ratio 18] [--log2n-flow 16]

Method of docs/measurement.md: every figure is the median of 7 launches timed singly between device events after 3 warm-up launches,
and the shader clock the part held is read beside one further launch (modarith_amd.clock).  Written to the report:

 1. records/s of SHA-256, SHA-512 and SHAKE256 (114 bytes out) at 2^20 records of 64, 181 and 1 024 bytes -- one contiguous row per
    record, one record per lane: an uncoalesced read; the 1 024-byte point shows what that costs -- with the shader clock under each;
 2. the Ed448 verify shape at 2^18 records: the launch of SHAKE256(dom4 || R || A || M) (10 shared + 57 + 57 + ragged 0..119 bytes,
    114 out) beside the ecn_ed448_mul2 launch of the same records, and their ratio;
 3. end to end at 2^16 records: examples/batch_signatures_device.Ed448Device.verify (hashes on the device) against
    examples/batch_signatures.Ed448.verify (hashlib in a Python loop: the path before this module), ALTERNATING in this process, each on
    its own native inputs (device tensors / lists of bytes, both prepared before the clock starts), host wall time around a device
    synchronisation because the host path's time is host time; three rounds, medians.  Both must return all-valid verdicts.

The tool exits 1 unless the device flow is the faster of the two; no other threshold.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_rate.json"))
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--log2n-ratio", type=int, default=18)
    ap.add_argument("--log2n-flow", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "hash_rate.py measures on the GPU: no device, no number"
    from modarith_amd import _lib
    from modarith_amd import hash as mh
    from modarith_amd.clock import timed_with_clock
    import batch_signatures as host_flow
    import batch_signatures_device as dev_flow

    launch = lambda: _lib.load().modarith_amd_last_launch().decode()      # noqa: E731
    report = {"device": torch.cuda.get_device_name(0),
              "timing": "median of 7 launches, each between device events, after 3 warm-up launches; shader clock from a probe beside one further launch",
              "rates": {}, "ed448_verify_shape": {}, "end_to_end": {}}
    g = torch.Generator(device="cuda").manual_seed(202)

    # ---- 1. records/s
    n = 1 << args.log2n
    algos = {"sha256": lambda p: mh.sha256([p]), "sha512": lambda p: mh.sha512([p]), "shake256": lambda p: mh.shake256([p], 114)}
    for L in (64, 181, 1024):
        rows = torch.randint(0, 256, (n, L), dtype=torch.uint8, device="cuda", generator=g)
        for name, fn in algos.items():
            t, ghz, _ = timed_with_clock(lambda: fn(rows), reps=7, warm=3)
            report["rates"]["%s/%d" % (name, L)] = {"records": n, "bytes_per_record": L, "ms": t * 1e3, "records_per_s": n / t, "message_bytes_per_s": n * L / t,
                                                    "shader_clock_ghz": ghz, "launch": launch()}
            print("%-9s %5d B  %8.3f ms  %.3e records/s  %.2f GHz" % (name, L, t * 1e3, n / t, ghz or 0), flush=True)
        del rows
        torch.cuda.empty_cache()

    # ---- 2. the verify shape: the hash launch beside the mul2 launch of the same records
    m = 1 << args.log2n_ratio
    E = dev_flow.Ed448Device()
    prv = torch.randint(0, 256, (m, 57), dtype=torch.uint8, device="cuda", generator=g)
    msg = torch.randint(0, 256, (m, 120), dtype=torch.uint8, device="cuda", generator=g)
    mlen = (torch.arange(m, device="cuda") % 120).to(torch.int32)
    pub = E.key_pair(prv)
    sig = E.sign(prv, pub, msg, mlen)
    parts, lens = [E._dom4(m), sig[:, :57], pub, msg], [None, None, None, mlen]
    th, ghz_h, digest = timed_with_clock(lambda: mh.shake256(parts, 114, lens=lens), reps=7, warm=3)
    name_h = launch()
    C, G = E.C, E.G
    Gp = C.cof(C.gen(m))
    Q = C.cof(C.set(((pub[:, 56] >> 7) & 1).to(torch.int32), None, pub[:, :56].flip(1).contiguous()))
    e = sig[:, 57:113].flip(1).contiguous()
    u = E.reduce(digest)
    G.modneg(u, u)
    f = G.modexp(u)
    tm, ghz_m, _ = timed_with_clock(lambda: C.mul2(e, Gp, f, Q), reps=7, warm=3)
    report["ed448_verify_shape"] = {"records": m, "hash_ms": th * 1e3, "hash_launch": name_h, "hash_shader_clock_ghz": ghz_h, "mul2_ms": tm * 1e3, "mul2_launch": launch(),
                                    "mul2_shader_clock_ghz": ghz_m, "hash_over_mul2": th / tm, "message_bytes": "10 shared + 57 + 57 + j % 120"}
    print("verify shape, %d records: hash %.3f ms, mul2 %.3f ms, ratio %.4f" % (m, th * 1e3, tm * 1e3, th / tm), flush=True)
    del prv, msg, mlen, pub, sig, parts, digest, Gp, Q, e, u, f
    torch.cuda.empty_cache()

    # ---- 3. end to end: device-hash verify against host-hash verify, alternating
    k = 1 << args.log2n_flow
    H = host_flow.Ed448()
    prv = torch.randint(0, 256, (k, 57), dtype=torch.uint8, device="cuda", generator=g)
    msg = torch.randint(0, 256, (k, 120), dtype=torch.uint8, device="cuda", generator=g)
    mlen = (torch.arange(k, device="cuda") % 120).to(torch.int32)
    pub = E.key_pair(prv)
    sig = E.sign(prv, pub, msg, mlen)
    rows = lambda t: [bytes(r) for r in t.cpu().tolist()]                  # noqa: E731
    hpub, hsig = rows(pub), rows(sig)
    hmsg = [r[:j % 120] for j, r in enumerate(rows(msg))]

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    _, vd = wall(lambda: E.verify(pub, msg, mlen, sig))                     # warm-up of both flows, and the verdicts
    _, vh = wall(lambda: H.verify(hpub, hmsg, hsig))
    assert vd.tolist() == vh == [1] * k, "the two flows must accept every signature"
    td, thost = [], []
    for _ in range(args.rounds):
        td.append(wall(lambda: E.verify(pub, msg, mlen, sig).cpu())[0])     # the verdicts on the host, as the host flow returns them
        thost.append(wall(lambda: H.verify(hpub, hmsg, hsig))[0])
    d, h = statistics.median(td), statistics.median(thost)
    report["end_to_end"] = {"records": k, "rounds": args.rounds, "device_flow_s": td, "host_hash_flow_s": thost, "device_flow_median_s": d, "host_hash_flow_median_s": h,
                            "host_over_device": h / d, "verifications_per_s": {"device_flow": k / d, "host_hash_flow": k / h},
                            "timing": "host wall clock around a device synchronisation, flows alternating, inputs in each flow's own form prepared beforehand"}
    print("end to end, %d records: device flow %.4f s, host-hash flow %.4f s: x %.1f" % (k, d, h, h / d), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.out)
    if not d < h:
        print("FAILED: the device flow is not the faster of the two")
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
