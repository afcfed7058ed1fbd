#!/usr/bin/env python3
"""Rate of the scalar multiplications of GENERATED curves at word length 32 (modarith_amd.generate.generate_curve(..., wl=32)) against
the 64-bit bit-exact ones of the same curve (GPU box, one MI355X) -- the method of tools/w32_curve_rate.py.

Per curve (SECP256K1: 9 limbs, NIST384: 14, NIST521 and ED500: 18; ED25519, built in, as the control), in ONE process and alternating
pass by pass:
  w64 mul         ecn_<c>_mul_batch            the 64-bit constant-time multiplication
  w64 mul2_exact  ecn_<c>_mul2_exact_batch     the reference's own walk at 64 bits
  w32 mul         ecn_<c>_w32_mul_batch        the plug-in's constant-time multiplication
  w32 mul2        ecn_<c>_w32_mul2_batch       the reference's own walk at 32 bits
  w32alt mul / mul2   at 18 limbs: the same curve built with the OTHER launch width (MA_MUL_WPS 1 where the driver chooses 2 and the
                  reverse) under a name of its own -- one wave per SIMD on the whole register file against two waves
2^20 legitimate points (2^19 from 14 limbs up; random multiples of the generator, scalars random), device events around single
launches, three warm-up passes, then the median over `passes` passes; the shader clock during one further launch of each
(modarith_amd.clock).  The reference point is the 64-bit kernel in the same process.  Per variant the pass-to-pass spread
(max - min) / median is recorded; a generated curve whose ratio w32 / w64 lies below the control's by more than that is explained in
docs/curve_layer.md, not tuned blind.  Writes profiles/w32_curve_gen_rate.json.  No rate is asserted anywhere: this measures.

The plug-ins go to a directory of this tool's own (tools/w32_curve_gen_plugins/, not the default plug-in directory):
  python tools/w32_curve_gen_rate.py --generate          (build box: hipcc, no GPU needed; also records the kernels' registers)
  python tools/w32_curve_gen_rate.py [--passes 7] [--out profiles/w32_curve_gen_rate.json]
"""
import argparse
import concurrent.futures as cf
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CURVES = ("SECP256K1", "NIST384", "NIST521", "ED500")
CONTROL = "ED25519"
ALT = {"NIST521": "NIST521ALT", "ED500": "ED500ALT"}          # the 18-limb curves under the other launch width
PLUGINS = os.path.join(ROOT, "tools", "w32_curve_gen_plugins")


def generate():
    import kernel_resources
    from modarith_amd import emit, generate as gen
    specs = []
    for c in CURVES:
        s = gen.named_curve(c)
        specs.append((s, None))
        if c in ALT:
            fp = gen.resolve(s["field"], wl=32)
            specs.append((dict(s, name=ALT[c]), 3 - emit.w32_curve_mul_wps(fp.nlimbs, fp.montgomery, s["kind"])))
    for c in CURVES:                                         # fields first: the alternative builds share them
        gen.generate_w32(gen.named_curve(c)["field"], plugin_dir=PLUGINS)
    with cf.ThreadPoolExecutor(max_workers=3) as ex:
        out = list(ex.map(lambda t: gen.generate_curve(**t[0], wl=32, plugin_dir=PLUGINS, mul_wps=t[1]), specs))
    regs = {}
    for g in out:
        meta = json.load(open(os.path.join(PLUGINS, "curve_%s_w32.json" % g.name)))
        for part, kern, key in (("mul", "k_ed_mul<", "mul"), ("mul2", "k_ed_mul2x<", "mul2")):
            o = os.path.join(PLUGINS, "capi_curve_%s_w32_ecn_%s.o" % (g.name, part))
            for k in kernel_resources.kernels_of(o):
                if kern in k["name"]:
                    regs["%s w32 %s" % (g.name, key)] = {"limbs": g.nlimbs, "MA_MUL_WPS": meta["mul_wps"], "vgprs": k["vgpr_count"], "agprs": k["agpr_count"],
                                                          "spilled": k["vgpr_spill_count"], "scratch_bytes": k["private_segment_fixed_size"]}
        print(g.name, g.nlimbs, "limbs, MA_MUL_WPS", meta["mul_wps"], "built" if g.built else "up to date")
    with open(os.path.join(PLUGINS, "registers.json"), "w") as f:
        json.dump(regs, f, indent=1)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--passes", type=int, default=7)
    ap.add_argument("--curves", default=",".join((CONTROL,) + CURVES))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "w32_curve_gen_rate.json"))
    ap.add_argument("--generate", action="store_true")
    args = ap.parse_args()
    if args.generate:
        return generate()
    import torch
    assert torch.cuda.is_available(), "w32_curve_gen_rate.py measures on the GPU: no device, no number"
    from modarith_amd import _lib, clock
    from modarith_amd.edwards import Curve
    regs = json.load(open(os.path.join(PLUGINS, "registers.json"))) if os.path.exists(os.path.join(PLUGINS, "registers.json")) else {}
    report = {"passes": args.passes, "timing": "device events around single launches, alternating variants pass by pass in one process; median of the passes after 3 warm-up passes",
              "device": torch.cuda.get_device_name(0), "control": CONTROL, "registers": regs, "curves": {}}
    for name in args.curves.split(","):
        W64 = Curve(name)
        W32 = Curve(name, wl=32) if name == CONTROL else Curve(name, wl=32, plugin_dir=PLUGINS)
        WA = Curve(ALT[name], wl=32, plugin_dir=PLUGINS) if name in ALT else None
        n = 1 << (20 if W32.N < 14 else 19)
        nb = W64.nbytes
        g = torch.Generator(device="cuda").manual_seed(99)
        rnd = lambda: torch.randint(0, 256, (n, nb), dtype=torch.uint8, device="cuda", generator=g)
        e, f = rnd(), rnd()
        pts = {}
        k0 = rnd()
        for tag, W in (("w64", W64), ("w32", W32)) + ((("w32alt", WA),) if WA else ()):
            P = W.mul(k0, W.gen(n))
            pts[tag] = (P, W.dbl(P.clone()), torch.empty_like(P))
        wss = {"w64": W64._workspace(n), "w32": W32._workspace(n)}
        if WA:
            wss["w32alt"] = WA._workspace(n)
        st = lambda: torch.cuda.current_stream().cuda_stream

        def sym(lib, s):
            fn = getattr(lib, s)
            fn.restype = ctypes.c_int
            return fn

        def mul_of(lib, s, tag):
            fn, w = sym(lib, "ecn_%s_mul_batch" % s), wss[tag]
            fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            return lambda: _lib.check(fn(e.data_ptr(), pts[tag][0].data_ptr(), n, n, w.data_ptr(), w.numel(), st()), s + " mul")

        def mul2_of(lib, s, tag):
            fn, w = sym(lib, "ecn_%s_batch" % s), wss[tag]
            fn.argtypes = [ctypes.c_void_p] * 5 + [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
            P, Q, R = pts[tag]
            return lambda: _lib.check(fn(e.data_ptr(), P.data_ptr(), f.data_ptr(), Q.data_ptr(), R.data_ptr(), n, n, w.data_ptr(), w.numel(), st()), s)

        low = name.lower()
        variants = {"w64 mul": mul_of(W64.lib, low, "w64"), "w64 mul2_exact": mul2_of(W64.lib, low + "_mul2_exact", "w64"),
                    "w32 mul": mul_of(W32.lib, low + "_w32", "w32"), "w32 mul2": mul2_of(W32.lib, low + "_w32_mul2", "w32")}
        if WA:
            alt = ALT[name].lower()
            variants["w32alt mul"] = mul_of(WA.lib, alt + "_w32", "w32alt")
            variants["w32alt mul2"] = mul2_of(WA.lib, alt + "_w32_mul2", "w32alt")
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
        row = {"n": n, "limbs": W32.N}
        for k, fn in variants.items():
            med = statistics.median(ms[k])
            ghz, _ = clock.clock_during(fn, med * 1e-3)
            row[k] = {"median_ms": med, "ms": ms[k], "per_s": n / (med * 1e-3), "spread": (max(ms[k]) - min(ms[k])) / med, "shader_clock_ghz": ghz}
        # the word lengths computed the same points (the multiplications above ran the same number of times on each)
        x64, y64, _ = W64.get(pts["w64"][0].clone())
        same = []
        for tag, W in (("w32", W32),) + ((("w32alt", WA),) if WA else ()):
            x32, y32, _ = W.get(pts[tag][0].clone())
            same.append(bool(torch.equal(x64, x32) and torch.equal(y64, y32)))
        row["same_points_at_both_word_lengths"] = all(same)
        if WA:
            row["both_launch_widths_return_the_same_limbs"] = bool(torch.equal(pts["w32"][0], pts["w32alt"][0]) and torch.equal(pts["w32"][2], pts["w32alt"][2]))
            row["ratio_alt_over_chosen"] = {"mul": row["w32alt mul"]["per_s"] / row["w32 mul"]["per_s"], "mul2": row["w32alt mul2"]["per_s"] / row["w32 mul2"]["per_s"]}
        row["ratio_w32_over_w64"] = {"mul": row["w32 mul"]["per_s"] / row["w64 mul"]["per_s"], "mul2": row["w32 mul2"]["per_s"] / row["w64 mul2_exact"]["per_s"]}
        row["spread_of_the_ratio"] = {"mul": row["w32 mul"]["spread"] + row["w64 mul"]["spread"], "mul2": row["w32 mul2"]["spread"] + row["w64 mul2_exact"]["spread"]}
        report["curves"][name] = row
        print("%-9s n=2^%d " % (name, n.bit_length() - 1) + " | ".join("%s %.3e/s @ %s GHz" % (k, row[k]["per_s"], ("%.2f" % row[k]["shader_clock_ghz"]) if row[k]["shader_clock_ghz"] else "?") for k in variants)
              + " | w32/w64 mul %.3f mul2 %.3f | same points: %s" % (row["ratio_w32_over_w64"]["mul"], row["ratio_w32_over_w64"]["mul2"], row["same_points_at_both_word_lengths"]), flush=True)
        del pts, wss
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(report, fh, indent=1)
    print("wrote", args.out)
    return 0


if __name__ == "__main__":
    sys.exit(main())
