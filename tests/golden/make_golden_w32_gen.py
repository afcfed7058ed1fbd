#!/usr/bin/env python3
"""Fixtures of the GENERATED fields of the 32-bit word form (modarith_amd.generate.EXAMPLES_W32) and of the parameter driver at that
word length.

Runs in the BUILD CONTAINER only (needs the reference tree): refgen.py drives the unmodified `pseudo.py 32 <prime>` / `monty.py 32
<prime>`, gcc compiles the C they emit, and the functions are called through ctypes on the element pool of tests/w32_gen_inputs.py.
What is written is data only:

  tests/golden/field_w32gen_<TAG>.json.xz   the record layout of field_w32_<P>.json.xz (make_golden_w32.py): params, the pool, one
                                             record list per emitted function (28: modpro / modinv / modqr / modsqrt need the external
                                             addchain tool and are pinned by value in the tests instead)
  tests/golden/params_w32_named.json.xz     what the reference derives at word length 32 by every name of modarith_amd.params.NAMED
                                             it knows there: N, base, n, Nbytes, xcess, the family flags and the prime limbs

  python tests/golden/make_golden_w32_gen.py [--no-fields] [--no-params]
"""
import ctypes, os, random, sys
from ctypes import c_char, c_int, c_uint, c_uint32

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import refgen  # noqa: E402
import gio  # noqa: E402
from make_golden_w32 import HARNESS, hx  # noqa: E402  (the harness: prop is static in the emitted file)
from tests import w32_gen_inputs as gi  # noqa: E402
from modarith_amd import params as mp  # noqa: E402

KEYS = ("WL", "n", "base", "N", "xcess", "Nbytes", "PM1D2", "PE", "p", "m", "mm", "TW", "EPM", "fred", "overflow", "carry_on",
        "bad_overflow_mul", "bad_overflow_sqr", "E", "R", "ndash", "trin", "PM", "karatsuba")


def derived(ns):
    out = {}
    for k in KEYS:
        if k in ns:
            v = ns[k]
            out[k] = hx(v) if isinstance(v, int) and not isinstance(v, bool) and v > 1 << 20 else v
    if "ppw" in ns:
        out["ppw"] = [int(v) for v in ns["ppw"]]
    return out


def reference_argv(arg, fam, fp):
    """how an example is spelled on the reference's command line"""
    script = "pseudo.py" if fp.family == "pseudo" else "monty.py"
    expr = arg.split("=", 1)[-1]
    return script, (mp.REFERENCE_NAME.get(expr, expr) if expr in mp.NAMED else expr)


class Ref:
    def __init__(self, script, arg):
        self.ns = refgen.load(script, 32, arg)
        self.lib, self.csrc = refgen.build(self.ns, HARNESS, tag="w32gen")
        self.N, self.Nbytes = self.ns["N"], self.ns["Nbytes"]
        for f in ("w32_prop", "flatten", "modfsb"):
            getattr(self.lib, f).restype = c_uint32
        for f in ("modis1", "modis0", "modsign", "modcmp", "modshr", "modimp"):
            getattr(self.lib, f).restype = c_int

    def arr(self, limbs=None):
        return (c_uint32 * self.N)(*(limbs or [0] * self.N))


def field_fixture(tag, arg, fam):
    fp = gi.params(tag)
    script, rarg = reference_argv(arg, fam, fp)
    ref = Ref(script, rarg)
    L, N, NB = ref.lib, ref.N, ref.Nbytes
    R, p = fp.radix, fp.p
    assert (N, R, ref.ns["n"], NB, ref.ns["p"]) == (fp.nlimbs, fp.radix, fp.n, fp.nbytes, fp.p), (tag, N, ref.ns["base"])
    extra = gi.EXTRA[N]
    pool = gi.pool(fp, extra)
    rng = random.Random(gi.seed(fp) + 1)
    P = gi.pack
    rec = {}
    for f in ("modadd", "modsub", "modmul"):
        rows = []
        for i, j in gi.pairs(fp, len(pool)):
            z = ref.arr()
            getattr(L, f)(ref.arr(pool[i]), ref.arr(pool[j]), z)
            rows.append([i, j, P(z)])
        rec[f] = rows
    for f in ("modneg", "modsqr", "modcpy", "nres", "redc"):
        rows = []
        for i, a in enumerate(pool):
            z = ref.arr()
            getattr(L, f)(ref.arr(a), z)
            rows.append([i, P(z)])
        rec[f] = rows
    rows = []
    for i, a in enumerate(pool):
        z = ref.arr(a)
        L.modhaf(z)
        rows.append([i, P(z)])
    rec["modhaf"] = rows
    for f, cf in (("prop", "w32_prop"), ("flatten", "flatten"), ("modfsb", "modfsb")):
        rows = []
        for i, a in enumerate(pool):
            z = ref.arr(a)
            r = getattr(L, cf)(z)
            rows.append([i, P(z), int(r)])
        rec[f] = rows
    rows = []
    for i, a in enumerate(pool):
        k = (0, 1, 2, 3, 5, 17)[i % 6]
        z = ref.arr(a)
        L.modnsqr(z, c_int(k))
        rows.append([i, k, P(z)])
    rec["modnsqr"] = rows
    rows = []
    for i, a in enumerate(pool):
        for b in (gi.MLI_INTS if i % 4 == 0 else gi.MLI_INTS[i % len(gi.MLI_INTS):][:2]):
            z = ref.arr()
            L.modmli(ref.arr(a), c_int(b), z)
            rows.append([i, b, P(z)])
    rec["modmli"] = rows
    for f in ("modis1", "modis0", "modsign"):
        rec[f] = [[i, int(getattr(L, f)(ref.arr(a)))] for i, a in enumerate(pool)]
    one = ref.arr()
    L.modone(one)
    rec["modcmp"] = [[i, j, int(L.modcmp(ref.arr(pool[i]), ref.arr(pool[j])))] for i, j in gi.pairs(fp, len(pool))]
    z = ref.arr([7] * N); L.modzer(z); rec["modzer"] = [[P(z)]]
    rec["modone"] = [[P(one)]]
    rows = []
    for x in (0, 1, 2, 3, 5, 9, 19, 39081, 121665, 0x7FFFFFFF, -1):
        z = ref.arr([7] * N)
        L.modint(c_int(x), z)
        rows.append([x, P(z)])
    rec["modint"] = rows
    rows = []
    for r in range(0, 8 * NB + 2):
        z = ref.arr([7] * N)
        L.mod2r(c_uint(r), z)
        rows.append([r, P(z)])
    rec["mod2r"] = rows
    cm, cs = [], []
    for k, (i, j) in enumerate(gi.pairs(fp, len(pool))[:len(pool)]):
        for d in ((0, 1) if k % 4 == 0 else (k & 1,)):
            g, f = ref.arr(pool[i]), ref.arr(pool[j])
            L.modcmv(c_int(d), g, f)
            cm.append([d, i, j, P(f)])
            g, f = ref.arr(pool[i]), ref.arr(pool[j])
            L.modcsw(c_int(d), g, f)
            cs.append([d, i, j, P(g), P(f)])
    rec["modcmv"], rec["modcsw"] = cm, cs
    sl, sr = [], []
    allones = [t for t, a in enumerate(pool) if a == [gi.M32] * N][0]
    for k in range(0, R + 1):
        for i in sorted({k % len(pool), (7 * k + 3) % len(pool), len(pool) - 1 - k, allones}):
            z = ref.arr(pool[i]); L.modshl(c_uint(k), z); sl.append([k, i, P(z)])
            z = ref.arr(pool[i]); r = L.modshr(c_uint(k), z); sr.append([k, i, P(z), int(r)])
    rec["modshl"], rec["modshr"] = sl, sr
    rows = []
    for i, a in enumerate(pool):
        out = (c_char * NB)()
        L.modexp(ref.arr(a), out)
        rows.append([i, bytes(out).hex()])
    rec["modexp"] = rows
    rows = []
    vals = [v for v in (0, 1, p - 1, p, p + 1, p + 2, 2 * p - 1, 2 * p, (1 << (8 * NB)) - 1, 1 << (8 * NB - 1)) if v < 1 << (8 * NB)]
    while len(vals) < 64:
        vals.append(rng.randrange(0, 1 << (8 * NB)) if len(vals) % 2 else rng.randrange(0, p))
    for v in vals:
        bs = v.to_bytes(NB, "big")
        z = ref.arr([7] * N)
        r = L.modimp((c_char * NB)(*bs), z)
        rows.append([bs.hex(), P(z), int(r)])
    rec["modimp"] = rows
    assert sorted(rec) == sorted(n if n != "flat" else "flatten" for n in refgen._ORDER), sorted(rec)
    return {"tag": tag, "prime": arg, "generator": script, "reference_argument": rarg, "wordlength": 32, "params": derived(ref.ns),
            "pool_extra": extra, "pool": [P(a) for a in pool], "records": rec, "count": sum(len(v) for v in rec.values())}


def named_params():
    """what the reference derives at word length 32 for every name of params.NAMED it knows there.  A name pseudo.py does not know at
    this word length (SECP256K1: `and WL==64`) is looked up in monty.py, as its user would"""
    out = {}
    for name, (p, fam) in mp.NAMED.items():
        script, arg = mp.reference_argv(name)
        tried = []
        for sc in ([script, "monty.py"] if script == "pseudo.py" else [script]):
            try:
                ns = refgen.load(sc, 32, arg)
            except SystemExit:
                tried.append(sc)
                continue
            if ns.get("p") != p:
                tried.append(sc)
                continue
            d = derived(ns)
            d["generator"] = sc
            d["argument"] = arg
            out[name] = d
            break
        print(name, out.get(name, {}).get("generator", "not known at word length 32 (%s)" % ", ".join(tried)), flush=True)
    return out


def main():
    if "--no-fields" not in sys.argv:
        for tag, arg, fam in gi.examples():
            fx = field_fixture(tag, arg, fam)
            path = gio.dump(fx, "field_w32gen_%s.json" % tag)
            print(tag, "pool", len(fx["pool"]), "records", fx["count"], os.path.getsize(path), "bytes", flush=True)
    if "--no-params" not in sys.argv:
        path = gio.dump({"wordlength": 32, "names": named_params()}, "params_w32_named.json")
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
