#!/usr/bin/env python3
"""Code objects of a set of fused chains, without running them (CPU): per kernel the registers, LDS, scratch, spills, the static
instruction count and its mix by class (tools/isa_mix.py), and per plug-in its dynamic symbols.

  python tools/chain_objects.py [--tree DIR] [--big TAG] [--out FILE]

--tree: the checkout whose modarith_amd/fuse.py emits and builds the chains (default: this one; it must hold a built
libmodarith_amd.so).  Run on two checkouts, the two files say what a change to the emitter or to csrc/chain.inc did to the kernels:
profiles/chain_one_include.json holds such a pair.  --big: the tag of a generated 64-bit field of more than 14 limbs, for the unit
whose element-major entry is the refusing stub."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import isa_mix  # noqa: E402
import kernel_resources  # noqa: E402


def accept(ch):
    x, y = ch.inputs(2)
    ch.output(ch.modinv(ch.modsqr(ch.modmul(ch.modadd(x, y), ch.modsub(x, y)))))


def prod(ch):
    u, v = ch.inputs(2)
    ch.output(ch.modsqr(ch.modmul(ch.modadd(u, v), ch.modsub(u, v))))


def aosio(ch):
    a, b = ch.inputs(2)
    g, h = ch.modcsw(ch.selector(), a, b)
    ch.output(ch.modmul(ch.modadd(g, h), ch.modsub(g, h)))
    ch.output(ch.modinv(h))


def ladderstep(ch, a24=121665):
    x1, x2, z2, x3, z3 = ch.inputs(5)
    sw = ch.selector()
    x2, x3 = ch.modcsw(sw, x2, x3)
    z2, z3 = ch.modcsw(sw, z2, z3)
    A, B, C, D = ch.modadd_lazy(x2, z2), ch.modsub_lazy(x2, z2), ch.modadd_lazy(x3, z3), ch.modsub_lazy(x3, z3)
    AA, BB, DA, CB = ch.modsqr(A), ch.modsqr(B), ch.modmul(D, A), ch.modmul(C, B)
    E = ch.modsub_lazy(AA, BB)
    for v in (ch.modmul(AA, BB), ch.modmul(E, ch.modadd_lazy(AA, ch.modmli(E, a24))),
              ch.modsqr(ch.modadd_lazy(DA, CB)), ch.modmul(x1, ch.modsqr(ch.modsub_lazy(DA, CB)))):
        ch.output(v)


def twoout(ch):
    x, y = ch.inputs(2)
    t, w = ch.modadd(x, y), ch.modsub(x, y)
    ch.output(ch.modmul(t, w))
    ch.output(ch.modmli(ch.modsqr(t), 121665))


# (key, prime, chain name, word length, builder, build keywords)
CHAINS = ([("bench_prod/X25519", "X25519", "bench_prod", 64, prod, {})]
          + [("accept/%s%s" % (P, "" if wl == 64 else "/w32"), P, "accept", wl, accept, {}) for wl in (64, 32) for P in ("X25519", "NIST256", "X448")]
          + [("accept/NIST521", "NIST521", "accept", 64, accept, {}), ("aosio/X448", "X448", "aosio", 64, aosio, {}),
             ("ladderstep/X25519", "X25519", "ladderstep", 64, ladderstep, {}),
             ("twoout/NIST256/w32", "NIST256", "twoout", 32, twoout, {}), ("twoout/NIST256/w32/ept4", "NIST256", "twoout", 32, twoout, {"ept": 4})])


def short(name):
    """k_chain<2> of `(anonymous namespace)::k_chain<2>((anonymous namespace)::Args, unsigned long, ma::Ld)`"""
    return re.sub(r"^\(anonymous namespace\)::", "", name.split("(anonymous namespace)::Args")[0].rstrip("("))


def figures(fuse, key, prime, name, wl, make, kw, d):
    ch = fuse.Chain(prime, name, wl=wl)
    make(ch)
    f = ch.build(plugin_dir=d, force=True, **kw)
    obj = os.path.join(d, "chain_%s_%s%s.o" % (name, prime, "" if wl == 64 else "_w32"))
    mix = {short(nm): isa_mix.analyse(code)["static"] for (_, nm), code in isa_mix.kernels(obj, "k_chain").items()}
    ks = {}
    for k in kernel_resources.kernels_of(obj):
        nm = short(k["name"])
        ks[nm] = dict({x: k[x] for x in kernel_resources.KEYS}, instructions=sum(mix[nm].values()), mix=mix[nm])
    nm = subprocess.run(["nm", "-D", f.path], capture_output=True, text=True, check=True).stdout.split("\n")
    syms = sorted(" ".join(l.split()[-2:]) for l in nm if l.strip() and "__hip_cuid_" not in l)
    return {"kernels": ks, "unit_lines": len(ch.source(**kw).splitlines()), "nm_D": syms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--big", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    from modarith_amd import fuse
    assert os.path.abspath(fuse.__file__).startswith(os.path.abspath(args.tree) + os.sep), fuse.__file__
    chains = CHAINS + ([("accept/%s" % args.big, args.big, "accept", 64, accept, {})] if args.big else [])
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for c in chains:
            out[c[0]] = figures(fuse, *c, d)
            print(c[0], {k: [v[x] for x in kernel_resources.KEYS] + [v["instructions"]] for k, v in out[c[0]]["kernels"].items()}, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
