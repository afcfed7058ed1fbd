#!/usr/bin/env python3
"""Fixtures of the 32-bit word form (`pseudo.py 32 X25519`, `monty.py 32 NIST256`, `monty.py 32 X448`).

Runs in the BUILD CONTAINER only (needs the reference tree): refgen.py drives the unmodified generators at word length 32, gcc compiles
the C they emit, and the functions are called through ctypes on the element pool of tests/w32_inputs.py.  What is written is data only:

  tests/golden/field_w32_<P>.json.xz   params (macro VALUES and derived quantities), the pool, and one record list per emitted
                                        function (28: modpro / modinv / modqr / modsqrt need the external addchain tool and are pinned
                                        by value in the tests instead)
  tests/golden/bulk_digests_w32.json.xz sha256 digests of modmul modsqr modadd modsub nres redc over 2^18 x 3 classes per prime

Elements are fixed-width hex strings (8 digits per limb, limb 0 first); records refer to pool elements by index.
Record layouts (i* = pool index, out = element, ret = integer):
  modadd modsub modmul [ia, ib, out]      modneg modsqr modcpy nres redc modhaf [ia, out]      prop flatten modfsb [ia, out, ret]
  modnsqr [ia, k, out]   modmli [ia, b, out]   modis1 modis0 modsign [ia, ret]   modcmp [ia, ib, ret]   modzer modone [out]
  modint [x, out]   mod2r [r, out]   modcmv [d, ig, if, out_f]   modcsw [d, ig, if, out_g, out_f]   modshl [k, ia, out]
  modshr [k, ia, out, ret]   modexp [ia, bytes]   modimp [bytes, out, ret]

  python tests/golden/make_golden_w32.py [--no-bulk]
"""
import ctypes, os, random, sys
from ctypes import c_char, c_int, c_uint, c_uint32

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
import refgen  # noqa: E402
import gio  # noqa: E402
from tests import w32_inputs as wi  # noqa: E402

U32P = ctypes.POINTER(c_uint32)
# harness (ours): prop is static in the emitted file; element-major loops for the bulk digests
HARNESS = r"""
#include <stddef.h>
spint w32_prop(spint *n) { return prop(n); }
void bulk_bin(int op, const spint *a, const spint *b, spint *c, size_t n) {
    size_t j;
    for (j = 0; j < n; j++) {
        const spint *x = a + j * Nlimbs, *y = b + j * Nlimbs; spint *z = c + j * Nlimbs;
        if (op == 0) modmul(x, y, z); else if (op == 1) modadd(x, y, z); else modsub(x, y, z);
    }
}
void bulk_un(int op, const spint *a, spint *c, size_t n) {
    size_t j;
    for (j = 0; j < n; j++) {
        const spint *x = a + j * Nlimbs; spint *z = c + j * Nlimbs;
        if (op == 0) modsqr(x, z); else if (op == 1) nres(x, z); else redc(x, z);
    }
}
"""
SCRIPTS = {"X25519": "pseudo.py", "NIST256": "monty.py", "X448": "monty.py"}


def hx(v):
    return "0x%x" % v


class Ref:
    def __init__(self, prime):
        self.ns = refgen.load(SCRIPTS[prime], 32, prime)
        self.lib, self.csrc = refgen.build(self.ns, HARNESS, tag="w32")
        self.prime = prime
        self.N, self.Nbytes = self.ns["N"], self.ns["Nbytes"]
        L = self.lib
        for f in ("w32_prop", "flatten", "modfsb"):
            getattr(L, f).restype = c_uint32
        for f in ("modis1", "modis0", "modsign", "modcmp", "modshr", "modimp"):
            getattr(L, f).restype = c_int

    def arr(self, limbs=None):
        return (c_uint32 * self.N)(*(limbs or [0] * self.N))


def params_of(ref):
    """macro VALUES of the emitted header block (name -> value; valueless macros -> true) and what the generator derived"""
    ns = ref.ns
    macros = {}
    for line in ref.csrc.splitlines():
        if line.startswith("#define"):
            parts = line.split()
            if parts[1] in ("Wordlength", "Nlimbs", "Radix", "Nbits", "Nbytes"):
                macros[parts[1]] = int(parts[2])
            elif parts[1] in ("spint", "sspint", "dpint", "sdpint"):
                macros[parts[1]] = parts[2]
            elif len(parts) == 2:
                macros[parts[1]] = True
    out = {"macros": macros}
    for k in ("WL", "n", "base", "N", "xcess", "Nbytes", "PM1D2", "PE", "p", "m", "mm", "TW", "EPM", "fred", "overflow", "carry_on",
              "bad_overflow_mul", "bad_overflow_sqr", "E", "R", "ndash", "trin", "PM", "karatsuba"):
        if k in ns:
            v = ns[k]
            out[k] = hx(v) if isinstance(v, int) and not isinstance(v, bool) and v > 1 << 20 else v
    if "ppw" in ns:
        out["ppw"] = [int(v) for v in ns["ppw"]]
        out["cw"] = [int(v) for v in ns["cw"]]
    out["ROI"] = [int(v) for v in ns["ROI"]]
    return out


def field_fixture(prime, extra):
    ref = Ref(prime)
    L, N, NB = ref.lib, ref.N, ref.Nbytes
    R, p = wi.SHAPES[prime][1], wi.SHAPES[prime][4]
    assert (N, R, ref.ns["n"], NB, ref.ns["p"]) == wi.SHAPES[prime]
    pool = wi.pool(prime, extra)
    rng = random.Random(wi.POOL_SEED[prime] + 1)
    P = wi.pack
    rec = {}
    for f in ("modadd", "modsub", "modmul"):
        rows = []
        for i, j in wi.pairs(prime, len(pool)):
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
        for b in (wi.MLI_INTS if i % 4 == 0 else wi.MLI_INTS[i % len(wi.MLI_INTS):][:2]):
            z = ref.arr()
            L.modmli(ref.arr(a), c_int(b), z)
            rows.append([i, b, P(z)])
    rec["modmli"] = rows
    for f in ("modis1", "modis0", "modsign"):
        rec[f] = [[i, int(getattr(L, f)(ref.arr(a)))] for i, a in enumerate(pool)]
    # modis1 / modis0 of the representatives of 1 and 0 that are not in the pool by value: 1 + p, and (Montgomery) nres(1), nres(1) + p
    one = ref.arr()
    L.modone(one)
    rec["modcmp"] = [[i, j, int(L.modcmp(ref.arr(pool[i]), ref.arr(pool[j])))] for i, j in wi.pairs(prime, len(pool))]
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
    for k, (i, j) in enumerate(wi.pairs(prime, len(pool))[:len(pool)]):
        for d in ((0, 1) if k % 4 == 0 else (k & 1,)):
            g, f = ref.arr(pool[i]), ref.arr(pool[j])
            L.modcmv(c_int(d), g, f)
            cm.append([d, i, j, P(f)])
            g, f = ref.arr(pool[i]), ref.arr(pool[j])
            L.modcsw(c_int(d), g, f)
            cs.append([d, i, j, P(g), P(f)])
    rec["modcmv"], rec["modcsw"] = cm, cs
    sl, sr = [], []
    for k in range(0, R + 1):
        for i in sorted({k % len(pool), (7 * k + 3) % len(pool), len(pool) - 1 - k, [t for t, a in enumerate(pool) if a == [wi.M32] * N][0]}):
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
    fx = {"prime": prime, "generator": SCRIPTS[prime], "wordlength": 32, "params": params_of(ref), "pool_extra": extra,
          "pool": [P(a) for a in pool], "records": rec, "count": sum(len(v) for v in rec.values())}
    return fx, ref


def bulk(refs):
    out = {"n": wi.BULK_N, "block": wi.BULK_BLOCK, "digest": "sha256, first 16 hex digits, of the [Nlimbs, block] little-endian u32 slice of the output",
           "inputs": "tests/w32_inputs.py bulk_inputs(prime, class)", "primes": {}}
    vp = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    BIN, UN = {"modmul": 0, "modadd": 1, "modsub": 2}, {"modsqr": 0, "nres": 1, "redc": 2}
    for P_, ref in refs.items():
        lib = ref.lib
        lib.bulk_bin.argtypes = [c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        lib.bulk_un.argtypes = [c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t]
        per = {}
        for cls in wi.BULK_CLASSES:
            a, b = wi.bulk_inputs(P_, cls)
            A, B = np.ascontiguousarray(a.T), np.ascontiguousarray(b.T)
            C = np.empty_like(A)
            d = {}
            for op in wi.BULK_OPS:
                if op in BIN:
                    lib.bulk_bin(BIN[op], vp(A), vp(B), vp(C), A.shape[0])
                else:
                    lib.bulk_un(UN[op], vp(A), vp(C), A.shape[0])
                d[op] = wi.block_digests(np.ascontiguousarray(C.T))
            per[cls] = d
            print(P_, cls, "done", flush=True)
        out["primes"][P_] = per
    print("wrote", gio.dump(out, "bulk_digests_w32.json"))


# random elements per class after the directed part of the pool: sized so that each file stays below the largest field fixture
EXTRA = {"X25519": 24, "NIST256": 24, "X448": 14}


def main():
    refs = {}
    for P_ in wi.W32_PRIMES:
        fx, refs[P_] = field_fixture(P_, EXTRA[P_])
        path = gio.dump(fx, "field_w32_%s.json" % P_)
        print(P_, "pool", len(fx["pool"]), "records", fx["count"], os.path.getsize(path), "bytes")
    if "--no-bulk" not in sys.argv:
        bulk(refs)


if __name__ == "__main__":
    main()
