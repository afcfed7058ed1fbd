"""Projective-limb fixtures of the curve layer at WORD LENGTH 32, straight from the reference's own edwards.c / weierstrass.c over
the field code `pseudo.py 32` / `monty.py 32` emit -- the recipe of tests/golden/curveref.py with 32 in its two places (curve.py's
argv and refgen.load), its own copy of the build function (curveref.py is not edited), and ctypes.c_uint32 structs.  The three
curves whose fields are built at this word length: ED25519 (9 x 29), NIST256 (9 x 29, Montgomery), ED448 (16 x 28, Montgomery).

Record shape of curveref_*.json (tests/golden/make_curveref.py): `gen`, chained `records` (P, e, f -> M, D, A, S, N, C, R, A+N,
A+A, isinf; scalar edge cases 0, 1, all-ones), `special`, `set_xy` -- plus `wild`: points whose limbs are ARBITRARY 32-bit words
(random words, all-ones, single huge limbs, limbs just past the radix) carried through dbl, add, neg, mul and mul2.  Those are
what separates "every limb pattern" from "in-contract points": the 32-bit field has one exact product policy, so the kernels
must return the reference's limbs for them too.

Nothing here ships: the build goes to a scratch directory, only vectors (tests/golden/curveref_w32_*.json.xz) are committed.
    python tests/golden/make_curveref_w32.py [CURVE ...]
"""
import ast, contextlib, ctypes, io, os, random, shutil, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refgen  # noqa: E402
import gio  # noqa: E402

REF = refgen.REF
WL = 32
CURVES = ("ED25519", "NIST256", "ED448")
KIND = {"ED25519": "edwards", "NIST256": "weierstrass", "ED448": "edwards"}


def build(curve: str):
    """-> (CDLL, prefix 'ecn_<curve>_', Nlimbs, Nbytes, radix, scratch dir): curveref.build at word length 32"""
    scratch = tempfile.mkdtemp(prefix="curveref_w32_")
    for f in ("edwards.c", "weierstrass.c", "curve.h", "testcurve.c"):
        shutil.copy(os.path.join(REF, f), scratch)
    path = os.path.join(REF, "curve.py")
    src = open(path).read()
    tree = ast.parse(src)
    ns = {"__name__": "__curveref__", "__file__": path}
    old_argv, old_cwd = sys.argv, os.getcwd()
    sys.argv = ["curve.py", str(WL), curve]
    os.chdir(scratch)
    log = io.StringIO()
    field_done = False
    try:
        for node in tree.body:
            seg = ast.get_source_segment(src, node) or ""
            if "subprocess.run" in seg and "radix=" in seg.replace(" ", ""):
                # `radix = subprocess.run("python3 pseudo.py 32 <curve>").returncode`: run that generator through refgen instead
                script = "pseudo.py" if ns["prime_type"] == ns["PSEUDO"] else "monty.py"
                g = refgen.load(script, WL, curve)
                ns["radix"] = g["base"]
                open(os.path.join(scratch, "field.c"), "w").write(refgen.emit_c(g, makestatic=False))
                field_done = True
                continue
            if "subprocess" in seg and not isinstance(node, (ast.Import, ast.ImportFrom)):
                continue                      # the group-order generator run (group.c): not needed by the curve layer
            with contextlib.redirect_stdout(log):
                exec(compile(ast.Module([node], []), path, "exec"), ns)
    finally:
        sys.argv = old_argv
        os.chdir(old_cwd)
    assert field_done
    cfile = "edwards.c" if ns["curve_type"] == ns["EDWARDS"] else "weierstrass.c"
    so = os.path.join(scratch, "curve.so")
    subprocess.check_call(["gcc", "-O2", "-fPIC", "-shared", "-w", "-I", scratch, "-o", so, os.path.join(scratch, cfile)])
    assert "#define CONSTANT_X" not in open(os.path.join(scratch, "curve.c")).read(), "generator from a small x: needs a square root"
    return ctypes.CDLL(so, mode=os.RTLD_LAZY), "ecn_%s_" % curve.lower(), ns["limbs"], ns["Nbytes"], ns["radix"], scratch


def fixture(curve, seed, records, wild):
    lib, pre, N, nb, radix, _ = build(curve)

    class Pt(ctypes.Structure):
        _fields_ = [("x", ctypes.c_uint32 * N), ("y", ctypes.c_uint32 * N), ("z", ctypes.c_uint32 * N)]
    PP = ctypes.POINTER(Pt)
    f = lambda name: getattr(lib, pre + name)
    for name, args in (("gen", [PP]), ("inf", [PP]), ("dbl", [PP]), ("neg", [PP]), ("cof", [PP]), ("add", [PP, PP]), ("sub", [PP, PP]), ("cpy", [PP, PP]),
                       ("mul", [ctypes.c_char_p, PP]), ("mul2", [ctypes.c_char_p, PP, ctypes.c_char_p, PP, PP])):
        f(name).argtypes = args
        f(name).restype = None
    f("isinf").argtypes = [PP]
    f("isinf").restype = ctypes.c_int
    H = lambda p: [[hex(v) for v in getattr(p, c)] for c in "xyz"]
    cp = lambda p: Pt.from_buffer_copy(bytes(p))
    ref = ctypes.byref
    rng = random.Random(seed)
    G = Pt()
    f("gen")(ref(G))
    fx = {"curve": curve, "wl": WL, "N": N, "Nbytes": nb, "radix": radix, "seed": seed, "gen": H(G),
          "source": "reference edwards.c / weierstrass.c + curve.py 32 + generator-emitted 32-bit field code, built by tests/golden/make_curveref_w32.py"}
    recs, legit = [], []
    P = cp(G)
    for k in range(records):
        e = bytes(rng.randrange(256) for _ in range(nb))
        g = bytes(rng.randrange(256) for _ in range(nb))
        if k == 1:
            e = (1).to_bytes(nb, "big")
        if k == 2:
            e = (0).to_bytes(nb, "big")
        if k == 3:
            e = b"\xff" * nb
        r = {"e": e.hex(), "f": g.hex(), "P": H(P)}
        M = cp(P); f("mul")(e, ref(M)); r["M"] = H(M)
        D = cp(M); f("dbl")(ref(D)); r["D"] = H(D)
        A = cp(M); f("add")(ref(D), ref(A)); r["A"] = H(A)
        S = cp(A); f("sub")(ref(D), ref(S)); r["S"] = H(S)
        Ng = cp(A); f("neg")(ref(Ng)); r["N"] = H(Ng)
        C = cp(A); f("cof")(ref(C)); r["C"] = H(C)
        R = Pt(); m2, d2 = cp(M), cp(D); f("mul2")(e, ref(m2), g, ref(d2), ref(R)); r["R"] = H(R)
        Z = cp(A); f("add")(ref(Ng), ref(Z)); r["A+N"] = H(Z); r["A+N_isinf"] = f("isinf")(ref(Z))      # P + (-P)
        T = cp(A); T2 = cp(A); f("add")(ref(T2), ref(T)); r["A+A"] = H(T)                                      # doubling through add
        r["isinf"] = [f("isinf")(ref(x)) for x in (M, D, A, R)]
        recs.append(r)
        legit.append(cp(A))
        P = cp(A) if k not in (2,) else cp(R)          # chain on; after the multiplication by zero continue from mul2's result
        if f("isinf")(ref(P)):
            P = cp(G)
    fx["records"] = recs
    O = Pt(); f("inf")(ref(O))
    sp = {"inf": H(O)}
    X = cp(O); f("dbl")(ref(X)); sp["dbl_inf"] = H(X)
    X = cp(G); f("add")(ref(O), ref(X)); sp["gen+inf"] = H(X)
    X = cp(O); f("add")(ref(G), ref(X)); sp["inf+gen"] = H(X)
    X = cp(O); f("mul")(bytes(rng.randrange(256) for _ in range(nb)), ref(X)); sp["mul_inf"] = H(X)
    fx["special"] = sp
    # ecnXXXset with BOTH coordinates: no square root, so the reference's own function runs.  Inputs: the affine points of the
    # big-integer fixtures (edwards_*.json / weierstrass_*.json "set_xy", on and off the curve)
    aff = gio.load("%s_%s.json" % (KIND[curve], curve))
    f("set").argtypes = [ctypes.c_int, ctypes.c_char_p, ctypes.c_char_p, PP]
    f("set").restype = None
    sx = []
    for r in aff["set_xy"]:
        X = Pt(); f("set")(0, bytes.fromhex(r["x"]), bytes.fromhex(r["y"]), ref(X))
        sx.append({"x": r["x"], "y": r["y"], "P": H(X), "isinf": f("isinf")(ref(X))})
        assert f("isinf")(ref(X)) == (0 if r["valid"] else 1), "the big-integer model and the reference disagree on a point's validity"
    fx["set_xy"] = sx

    # wild records: limbs that no field function returns
    ONES = 0xffffffff
    def wild_point(kind):
        p = Pt()
        for c in "xyz":
            for i in range(N):
                if kind == 0:   v = ONES                                            # every limb all-ones
                elif kind == 1: v = rng.getrandbits(32)                             # random 32-bit words
                elif kind == 2: v = rng.getrandbits(radix) | ((i == rng.randrange(N)) << 31)     # a legitimate-looking element with stray top bits
                elif kind == 3: v = rng.getrandbits(radix + 2) + (1 << (radix + 2)) * (i % 2)    # just past the limb budget
                else:           v = rng.choice((0, ONES, 1 << 31, (1 << radix) - 1, 1 << radix, rng.getrandbits(32)))
                getattr(p, c)[i] = v & ONES
        return p
    wl = []
    for k in range(wild):
        Pw = wild_point(k % 5)
        Qw = wild_point((k + 1) % 5) if k % 3 else cp(legit[k % len(legit)])     # a wild point next to a legitimate one, too
        e = bytes(rng.randrange(256) for _ in range(nb))
        g = bytes(rng.randrange(256) for _ in range(nb))
        if k == 0:
            e = b"\xff" * nb
        r = {"e": e.hex(), "f": g.hex(), "P": H(Pw), "Q": H(Qw)}
        D = cp(Pw); f("dbl")(ref(D)); r["D"] = H(D)
        A = cp(Pw); q = cp(Qw); f("add")(ref(q), ref(A)); r["A"] = H(A)
        Ng = cp(Pw); f("neg")(ref(Ng)); r["N"] = H(Ng)
        M = cp(Pw); f("mul")(e, ref(M)); r["M"] = H(M)
        R = Pt(); p2, q2 = cp(Pw), cp(Qw); f("mul2")(e, ref(p2), g, ref(q2), ref(R)); r["R"] = H(R)
        r["isinf"] = f("isinf")(ref(Pw))
        wl.append(r)
    fx["wild"] = wl
    return fx


def main():
    only = [a for a in sys.argv[1:] if not a.startswith("-")]
    for k, c in enumerate(CURVES):
        if only and c not in only:
            continue
        fx = fixture(c, 32000 + k, 6 if c == "ED448" else 8, 10)
        gio.dump(fx, "curveref_w32_%s.json" % c)
        print(c, fx["N"], "x", fx["radix"], len(fx["records"]), "records,", len(fx["wild"]), "wild; gen x limb 0:", fx["gen"][0][0])


if __name__ == "__main__":
    main()
