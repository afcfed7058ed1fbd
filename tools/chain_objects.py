#!/usr/bin/env python3
"""Code objects of a set of fused chains, without running them (CPU): per kernel the registers, LDS, scratch, spills, the static
instruction count and its mix by class (tools/isa_mix.py), and per plug-in its dynamic symbols.

  python tools/chain_objects.py [--tree DIR] [--big TAG] [--out FILE]
  python tools/chain_objects.py [--tree DIR] --sources FILE
  python tools/chain_objects.py --pair PARENT NEW [--pair-sources PARENT NEW] --out FILE

--tree: the checkout whose modarith_amd/fuse.py emits and builds the chains (default: this one; it must hold a built
libmodarith_amd.so).  Run on two checkouts, the two files say what a change to the emitter or to csrc/chain.inc did to the kernels;
--pair puts two such files side by side (profiles/chain_one_include.json and profiles/chain_one_entry.json hold such pairs; the
latter's "rate" is tools/chain_ab_rate.py's output).  --big: the tag of a generated 64-bit field of more than 14 limbs, for the unit
whose element-major entry is the refusing stub.  --sources: no build; the text Chain.source() emits for every chain under every build
keyword set (KEYWORDS), for --pair-sources to compare between two checkouts byte by byte."""
import argparse
import hashlib
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


def everykind(ch):
    """every kind of array in one call: an element input, a byte input, a shared operand and a selector in; an element, a byte record
    and an int out (the chain of tests/test_gpu_fuse_bytes.py::test_every_kind_of_array)"""
    a = ch.input()
    r, ok = ch.input_bytes()
    k, d = ch.shared(), ch.selector()
    t = ch.modmul(a, k)
    u = ch.modadd(t, r)
    ch.output(ch.modcmv(d, t, u))
    ch.output_bytes(u)
    ch.output(ch.land(ok, ch.lnot(ch.modis0(u))))


def library(which):
    """a chain the library carries (fuse.oncurve_chain / pubkey_chain / decompress_chain over their default curves), made by the
    tree's own fuse.py: the builder returns it in place of the empty chain it is given"""
    return lambda ch: getattr(sys.modules[type(ch).__module__], which)(wl=ch.wl, name=ch.name)[0]


def negint(ch):
    x = ch.input()
    ch.output(ch.modmul(ch.modadd(x, ch.shared()), ch.modint(-3)))


# (key, prime, chain name, word length, builder, build keywords)
CHAINS = ([("bench_prod/X25519", "X25519", "bench_prod", 64, prod, {})]
          + [("accept/%s%s" % (P, "" if wl == 64 else "/w32"), P, "accept", wl, accept, {}) for wl in (64, 32) for P in ("X25519", "NIST256", "X448")]
          + [("accept/NIST521", "NIST521", "accept", 64, accept, {}), ("aosio/X448", "X448", "aosio", 64, aosio, {}),
             ("ladderstep/X25519", "X25519", "ladderstep", 64, ladderstep, {}),
             ("twoout/NIST256/w32", "NIST256", "twoout", 32, twoout, {}), ("twoout/NIST256/w32/ept4", "NIST256", "twoout", 32, twoout, {"ept": 4})]
          # shared operands, ints and byte records: the chains the library carries and one call with every kind of array, at both word lengths
          + [("%s/%s%s" % (nm, P, "" if wl == 64 else "/w32"), P, nm, wl, make, {}) for wl in (64, 32)
             for nm, P, make in (("oncurve", "NIST256", library("oncurve_chain")), ("pubkey", "NIST256", library("pubkey_chain")),
                                 ("decompress", "X25519", library("decompress_chain")), ("everykind", "X25519", everykind))])
# --sources: the text of these under every keyword set of KEYWORDS that the word length takes, nothing built
TEXT_CHAINS = CHAINS + [("negint/X25519%s" % ("" if wl == 64 else "/w32"), "X25519", "negint", wl, negint, {}) for wl in (64, 32)]
KEYWORDS = ({}, {"ept": 1}, {"policy": "exact"}, {"policy": "fast"}, {"waves": 2}, {"block": 128})


def short(name):
    """k_chain<2> of `(anonymous namespace)::k_chain<2>((anonymous namespace)::Args, unsigned long, ma::Ld)`"""
    return re.sub(r"^\(anonymous namespace\)::", "", name.split("(anonymous namespace)::Args")[0].rstrip("("))


def chain_of(fuse, prime, name, wl, make):
    ch = fuse.Chain(prime, name, wl=wl)
    return make(ch) or ch


def sources(fuse):
    """{key: {keywords: text}}: Chain.source() of TEXT_CHAINS under every keyword set (a workgroup size: word length 32 only; a forced
    product policy: word length 64 only)"""
    out = {}
    for key, prime, name, wl, make, kw in TEXT_CHAINS:
        for extra in KEYWORDS:
            if ("block" in extra and wl == 64) or ("policy" in extra and wl == 32):
                continue
            out.setdefault(key, {})[json.dumps(dict(kw, **extra), sort_keys=True)] = chain_of(fuse, prime, name, wl, make).source(**dict(kw, **extra))
    return out


def figures(fuse, key, prime, name, wl, make, kw, d):
    ch = chain_of(fuse, prime, name, wl, make)
    f = ch.build(plugin_dir=d, force=True, **kw)
    obj = os.path.join(d, "chain_%s_%s%s.o" % (name, prime, "" if wl == 64 else "_w32"))
    code = {short(nm): c for (_, nm), c in isa_mix.kernels(obj, "k_chain").items()}
    mix = {nm: isa_mix.analyse(c)["static"] for nm, c in code.items()}
    ks = {}
    for k in kernel_resources.kernels_of(obj):
        nm = short(k["name"])
        # isa_sha256: the instruction text as isa_mix reads it (mnemonics and operands, no addresses), for "is it the same code" between two trees
        ks[nm] = dict({x: k[x] for x in kernel_resources.KEYS}, instructions=sum(mix[nm].values()), mix=mix[nm],
                      isa_sha256=hashlib.sha256("\n".join(ins for _, ins in code[nm]).encode()).hexdigest())
    nm = subprocess.run(["nm", "-D", f.path], capture_output=True, text=True, check=True).stdout.split("\n")
    syms = sorted(" ".join(l.split()[-2:]) for l in nm if l.strip() and "__hip_cuid_" not in l)
    return {"kernels": ks, "unit_lines": len(ch.source(**kw).splitlines()), "nm_D": syms}


def pair(parent, new):
    """two --out files side by side, in the shape of profiles/chain_one_include.json: per kernel the parent's and the new figures, the
    list of what differs, and the verdicts"""
    assert parent.keys() == new.keys()
    objs, diffs, isa = {}, [], []
    for key in sorted(parent):
        kp, kn = parent[key]["kernels"], new[key]["kernels"]
        objs[key] = {nm: {"parent": kp.get(nm), "new": kn.get(nm)} for nm in sorted(set(kp) | set(kn))}
        for nm in sorted(set(kp) & set(kn)):
            d = {x: [kp[nm][x], kn[nm][x]] for x in list(kernel_resources.KEYS) + ["instructions"] if kp[nm][x] != kn[nm][x]}
            d.update({c: [kp[nm]["mix"].get(c, 0), kn[nm]["mix"].get(c, 0)] for c in sorted(set(kp[nm]["mix"]) | set(kn[nm]["mix"])) if kp[nm]["mix"].get(c, 0) != kn[nm]["mix"].get(c, 0)})
            if d:
                diffs.append({"chain": key, "kernel": nm, "parent_to_new": d})
            if kp[nm].get("isa_sha256") != kn[nm].get("isa_sha256"):
                isa.append("%s %s" % (key, nm))
    return {"code_objects": objs, "differences": diffs, "kernels_whose_instruction_text_differs": isa,
            "every_resource_figure_equal": not any(set(d["parent_to_new"]) & set(kernel_resources.KEYS) for d in diffs),
            "instruction_count_and_mix_equal": not diffs, "instruction_text_equal": not isa,
            "same_kernels_instantiated": all(set(parent[k]["kernels"]) == set(new[k]["kernels"]) for k in parent),
            "nm_D_equal_but_for_hip_cuid": all(parent[k]["nm_D"] == new[k]["nm_D"] for k in parent),
            "unit_lines_parent_to_new": {k: [parent[k]["unit_lines"], new[k]["unit_lines"]] for k in sorted(parent)}}


def pair_sources(parent, new):
    """two --sources files: how many texts are byte-identical, and every line of the others that differs"""
    assert parent.keys() == new.keys() and all(parent[k].keys() == new[k].keys() for k in parent)
    texts = [(k, kw) for k in sorted(parent) for kw in sorted(parent[k])]
    other = {}
    for k, kw in texts:
        if parent[k][kw] != new[k][kw]:
            a, b = parent[k][kw].splitlines(), new[k][kw].splitlines()
            other["%s %s" % (k, kw)] = {"lines_parent_to_new": [len(a), len(b)], "differing_lines": [[x, y] for x, y in zip(a, b) if x != y]}
    return {"texts": len(texts), "byte_identical": len(texts) - len(other), "chains": sorted(parent), "keyword_sets": [json.dumps(k, sort_keys=True) for k in KEYWORDS], "not_identical": other}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--big", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sources", default=None, metavar="FILE", help="write the emitted text of the chains under every build keyword set to FILE and build nothing")
    ap.add_argument("--pair", nargs=2, default=None, metavar=("PARENT", "NEW"), help="two --out files -> the comparison, to --out")
    ap.add_argument("--pair-sources", nargs=2, default=None, metavar=("PARENT", "NEW"), help="two --sources files -> `emitted_text` of the comparison")
    args = ap.parse_args()
    if args.pair or args.pair_sources:
        load = lambda p: json.load(open(p))
        out = pair(*map(load, args.pair)) if args.pair else {}
        if args.pair_sources:
            out["emitted_text"] = pair_sources(*map(load, args.pair_sources))
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1, sort_keys=True)
        return 0
    sys.path.insert(0, os.path.abspath(args.tree))
    from modarith_amd import fuse
    assert os.path.abspath(fuse.__file__).startswith(os.path.abspath(args.tree) + os.sep), fuse.__file__
    if args.sources:
        with open(args.sources, "w") as f:
            json.dump(sources(fuse), f, indent=1, sort_keys=True)
        return 0
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
