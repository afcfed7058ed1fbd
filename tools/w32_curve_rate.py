#!/usr/bin/env python3
"""Rate of the curve layer's scalar multiplications at word length 32 against the 64-bit bit-exact ones (GPU box, one MI355X).

Per curve (ED25519, NIST256, ED448), in ONE process and alternating pass by pass:
  w64 mul         ecn_<c>_mul_batch            the 64-bit constant-time multiplication (resident half-limb forms where they exist)
  w64 mul2_exact  ecn_<c>_mul2_exact_batch     the reference's own walk at 64 bits
  w32 mul         ecn_<c>_w32_mul_batch        the window table with one limb per 256-byte row (the layout that ships)
  w32 mul2        ecn_<c>_w32_mul2_batch       the reference's own walk at 32 bits
  w32p mul / mul2 the same two kernels with two limbs packed per 64-bit table word (csrc/curve.h MA_W32_TABLE_PACKED), when a side
                  library holding them was built beforehand with --build-packed (hipcc, no GPU needed) -- "both layouts, measured"
2^20 points (legitimate points: random multiples of the generator, scalars random), device events around single launches, three
warm-up passes, then the median over `passes` passes; the shader clock during one further launch of each (modarith_amd.clock).
VGPRs and waves per SIMD come from the code objects (tools/kernel_resources.py) where the build's objects are at hand.  Writes
profiles/w32_curve_rate.json: rates, ratios w32 / w64, clocks, registers.  No rate is asserted anywhere: this measures.

  python tools/w32_curve_rate.py --build-packed          (build box)
  python tools/w32_curve_rate.py [--log2n 20] [--passes 7] [--out profiles/w32_curve_rate.json]
"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CURVES = ("ED25519", "NIST256", "ED448")
PACKED_LIB = os.path.join(ROOT, "tools", "libw32_curve_packed.so")


def build_packed():
    """the mul / mul2 parts of the three w32 curve units once more with the packed table layout, under ecn_<c>_w32p_*_batch, into a
    side library next to this tool (not part of the product build)"""
    from modarith_amd import build
    csrc = build.CSRC
    objs = []
    for c in CURVES:
        for part in (1, 2):
            o = os.path.join(ROOT, "tools", "w32p_%s_%d.o" % (c, part))
            subprocess.check_call([build.HIPCC] + build.FLAGS + ["-DMA_W32_TABLE_PACKED", "-DMA_CNAME=%s_w32p" % c.lower(), "-DMA_CURVE_PART=%d" % part,
                                   "-c", os.path.join(csrc, "capi_%s_w32_ecn.hip" % c), "-o", o])
            objs.append(o)
    subprocess.check_call([build.HIPCC, "--offload-arch=" + build.ARCH, "-shared", "-fPIC", "-o", PACKED_LIB] + objs +
                          ["-L" + build.HERE, "-l:libmodarith_amd.so", "-Wl,-rpath,$ORIGIN/" + os.path.relpath(build.HERE, os.path.dirname(PACKED_LIB)), "-Wl,-rpath," + build.HERE])
    for o in objs:
        os.remove(o)
    print("built", PACKED_LIB)
    return 0


def registers():
    """{kernel family: {vgprs, waves_per_simd}} of the scalar-multiplication kernels, from the build's objects (absent: {})"""
    import kernel_resources
    out = {}
    bdir = os.path.join(ROOT, "modarith_amd", "build")
    want = {"w32": [("capi_%s_w32_ecn_mul.o", "k_ed_mul<"), ("capi_%s_w32_ecn_mul2.o", "k_ed_mul2x<")],
            "w64": [("capi_%s_part1.o", "k_ed_mul<"), ("capi_%s_part2.o", "k_ed_mul2x<")]}
    for c in CURVES:
        for wl, specs in want.items():
            for pat, kern in specs:
                unit = c + ("W" if (wl == "w64" and c == "NIST256") else "")
                o = os.path.join(bdir, pat % unit)
                if not os.path.exists(o):
                    continue
                for k in kernel_resources.kernels_of(o):
                    if kern in k["name"] and ", -1>(" not in k["name"]:          # (not the exact class behind a 64-bit fast kernel)
                        v = k["vgpr_count"] + k["agpr_count"]
                        out["%s %s %s" % (c, wl, "mul" if kern == "k_ed_mul<" else "mul2")] = {
                            "vgprs": k["vgpr_count"], "agprs": k["agpr_count"], "spilled": k["vgpr_spill_count"], "waves_per_simd_by_registers": min(8, 512 // max(v, 64))}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2n", type=int, default=20)
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--curves", default=",".join(CURVES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w32_curve_rate.json"))
    ap.add_argument("--build-packed", action="store_true")
    args = ap.parse_args()
    if args.build_packed:
        return build_packed()
    import torch
    assert torch.cuda.is_available(), "w32_curve_rate.py measures on the GPU: no device, no number"
    from modarith_amd import _lib, clock
    from modarith_amd.edwards import Curve
    n = 1 << args.log2n
    packed = ctypes.CDLL(PACKED_LIB) if os.path.exists(PACKED_LIB) and _lib.load() else None
    regs = registers()
    report = {"n": n, "passes": args.passes, "timing": "device events around single launches, alternating variants pass by pass in one process; median",
              "device": torch.cuda.get_device_name(0), "table_layouts": ["one limb per 256-byte row"] + (["two limbs per 64-bit word (packed)"] if packed else []),
              "registers": regs, "curves": {}}
    for name in args.curves.split(","):
        W64, W32 = Curve(name), Curve(name, wl=32)
        nb = W64.nbytes
        g = torch.Generator(device="cuda").manual_seed(99)
        rnd = lambda: torch.randint(0, 256, (n, nb), dtype=torch.uint8, device="cuda", generator=g)
        e, f = rnd(), rnd()
        pts = {}
        for tag, W in (("w64", W64), ("w32", W32)):
            k0 = rnd()
            P = W.mul(k0, W.gen(n))
            pts[tag] = (P, W.dbl(P.clone()), torch.empty_like(P))
        ws = W64._workspace(n)
        ws32 = W32._workspace(n)
        st = lambda: torch.cuda.current_stream().cuda_stream

        def sym(lib, s):
            fn = getattr(lib, s)
            fn.restype = ctypes.c_int
            return fn

        def mul_of(lib, s, tag, w):
            fn = sym(lib, "ecn_%s_mul_batch" % s)
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            return lambda: _lib.check(fn(e.data_ptr(), pts[tag][0].data_ptr(), n, n, w.data_ptr(), w.numel(), st()), s + " mul")

        def mul2_of(lib, s, tag, w):
            fn = sym(lib, "ecn_%s_batch" % s)
            fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            P, Q, R = pts[tag]
            return lambda: _lib.check(fn(e.data_ptr(), P.data_ptr(), f.data_ptr(), Q.data_ptr(), R.data_ptr(), n, n, w.data_ptr(), w.numel(), st()), s)

        low = name.lower()
        variants = {"w64 mul": mul_of(W64.lib, low, "w64", ws), "w64 mul2_exact": mul2_of(W64.lib, low + "_mul2_exact", "w64", ws),
                    "w32 mul": mul_of(W32.lib, low + "_w32", "w32", ws32), "w32 mul2": mul2_of(W32.lib, low + "_w32_mul2", "w32", ws32)}
        if packed is not None:
            # the packed table is never larger than the plain one at an even limb count and 10/9 of it at nine limbs: a workspace of its own
            wsp = torch.empty(ws32.numel() * 10 // 9 + 64, dtype=torch.uint8, device="cuda")
            variants["w32p mul"] = mul_of(packed, low + "_w32p", "w32", wsp)
            variants["w32p mul2"] = mul2_of(packed, low + "_w32p_mul2", "w32", wsp)
        ms = {k: [] for k in variants}
        for p in range(3 + args.passes):
            for k, fn in variants.items():
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                fn()
                b.record()
                torch.cuda.synchronize()
                if p >= 3:
                    ms[k].append(a.elapsed_time(b))
        row = {}
        for k, fn in variants.items():
            med = statistics.median(ms[k])
            ghz, _ = clock.clock_during(fn, med * 1e-3)
            row[k] = {"median_ms": med, "ms": ms[k], "per_s": n / (med * 1e-3), "shader_clock_ghz": ghz}
        # the two word lengths computed the same points (the multiplications above ran the same number of times on each)
        x64, y64, _ = W64.get(pts["w64"][0].clone())
        x32, y32, _ = W32.get(pts["w32"][0].clone())
        row["same_points_at_both_word_lengths"] = bool(torch.equal(x64, x32) and torch.equal(y64, y32)) if packed is None else None
        row["ratio_w32_over_w64"] = {"mul": row["w32 mul"]["per_s"] / row["w64 mul"]["per_s"], "mul2": row["w32 mul2"]["per_s"] / row["w64 mul2_exact"]["per_s"]}
        if packed is not None:
            variants["w32 mul2"](); r_plain = pts["w32"][2].clone()
            variants["w32p mul2"](); torch.cuda.synchronize()
            row["packed_layout_returns_the_same_limbs"] = bool(torch.equal(r_plain, pts["w32"][2]))
            row["ratio_packed_over_plain"] = {"mul": row["w32p mul"]["per_s"] / row["w32 mul"]["per_s"], "mul2": row["w32p mul2"]["per_s"] / row["w32 mul2"]["per_s"]}
        report["curves"][name] = row
        print("%-8s " % name + " | ".join("%s %.3e/s @ %s GHz" % (k, row[k]["per_s"], ("%.2f" % row[k]["shader_clock_ghz"]) if row[k]["shader_clock_ghz"] else "?") for k in variants)
              + " | w32/w64 mul %.2f mul2 %.2f" % (row["ratio_w32_over_w64"]["mul"], row["ratio_w32_over_w64"]["mul2"]), flush=True)
        del pts, ws, ws32
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
