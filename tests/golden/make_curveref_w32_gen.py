"""Projective-limb fixtures of the curve layer at WORD LENGTH 32 for the curves that are generated there (modarith_amd.generate
generate_curve(..., wl=32)): the eight curves of curve.py's table whose 32-bit form is not built in -- SECP256K1, NUMS256W, NUMS256E,
ED248 (9 x 29), NIST384, ED376 (14 x 28), NIST521, ED500 (18 x 29) -- and CURVE1174, a curve that is not in curve.py's table
(generate.EXAMPLE_CURVES[0]) over the generated field 2^251 - 9 (9 x 28).  Straight from the reference's own edwards.c / weierstrass.c
over the field code `pseudo.py 32` / `monty.py 32` emit.

The recipe of tests/golden/make_curveref_w32.py (its record shape, wild records included) with its own copy of the build function, plus
two things of the 64-bit recipe at ctypes.c_uint32:
  * a generator given by a small x (NUMS256W, NUMS256E, ED248, ED376, ED500): ecnXXXgen would take a square root (addchain), so the
    point comes from the affine coordinates of edwards_*.json / weierstrass_*.json through the reference's own nres and modone
    (make_curveref.py:80-92);
  * custom=: the variables curve.py's "More curves can be added here" block assigns (curveref.build).

Nothing here ships: the build goes to a scratch directory, only vectors (tests/golden/curveref_w32_<CURVE>.json.xz) are committed.
    python tests/golden/make_curveref_w32_gen.py [CURVE ...]
"""
import ast, contextlib, ctypes, io, os, random, shutil, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import refgen  # noqa: E402
import gio  # noqa: E402

REF = refgen.REF
WL = 32
CURVES = ("SECP256K1", "NUMS256W", "NUMS256E", "ED248", "NIST384", "ED376", "NIST521", "ED500")
KIND = {"SECP256K1": "weierstrass", "NUMS256W": "weierstrass", "NUMS256E": "edwards", "ED248": "edwards", "NIST384": "weierstrass",
        "ED376": "edwards", "NIST521": "weierstrass", "ED500": "edwards"}
CUSTOM = "CURVE1174"


def custom_curve(name=CUSTOM):
    """one of modarith_amd.generate.EXAMPLE_CURVES in curve.py's vocabulary, its field resolved at word length 32"""
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from modarith_amd.generate import EXAMPLE_CURVES, EXAMPLES_W32, resolve
    from modarith_amd.params import NAMED
    c = next(c for c in EXAMPLE_CURVES if c["name"] == name)
    if c["field"] in NAMED:
        fp, arg = resolve(c["field"], wl=WL), c["field"]
    else:
        arg, fam = next((a, f) for a, f in EXAMPLES_W32 if resolve(a, f, wl=WL).name == c["field"])
        fp, arg = resolve(arg, fam, wl=WL), arg.split("=", 1)[-1]
    return dict(p=fp.p, q=c["order"], cof=c.get("cof", 0), prime_type=fp.family, curve_type=c["kind"], A=c["a"], B=c["b"], X=c["gx"], Y=c["gy"],
                field_arg=arg)


def affine_multiples(cu, count):
    """[G, 2G, ...] as affine (x, y) by plain integer arithmetic, for the ecnXXXset inputs of a custom curve"""
    p, a, b = cu["p"], cu["A"], cu["B"]
    G = (cu["X"], cu["Y"])
    if cu["curve_type"] == "edwards":
        def add(P, Q):
            t = b * P[0] * Q[0] * P[1] * Q[1] % p
            return ((P[0] * Q[1] + P[1] * Q[0]) * pow(1 + t, -1, p) % p, (P[1] * Q[1] - a * P[0] * Q[0]) * pow(1 - t, -1, p) % p)
    else:
        def add(P, Q):
            if P == Q:
                m = (3 * P[0] * P[0] + a) * pow(2 * P[1], -1, p) % p
            else:
                m = (Q[1] - P[1]) * pow(Q[0] - P[0], -1, p) % p
            x = (m * m - P[0] - Q[0]) % p
            return (x, (m * (P[0] - x) - P[1]) % p)
    out, P = [], G
    for _ in range(count):
        out.append(P)
        P = add(P, G)
    return out


def build(curve: str, custom: dict = None):
    """-> (CDLL, prefix 'ecn_<curve>_', Nlimbs, Nbytes, radix, scratch dir, small_x): curveref.build at word length 32"""
    scratch = tempfile.mkdtemp(prefix="curveref_w32g_")
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
            if custom is not None and isinstance(node, ast.If) and "This curve not supported" in seg:
                assert ns["p"] == 0, "%s is in curve.py's table" % curve
                ns.update(p=custom["p"], q=custom["q"], cof=custom["cof"], A=custom["A"], B=custom["B"], X=custom["X"], Y=custom["Y"],
                          prime_type=ns["PSEUDO"] if custom["prime_type"] == "pseudo" else ns["MONTY"],
                          curve_type=ns["EDWARDS"] if custom["curve_type"] == "edwards" else ns["WEIERSTRASS"])
                continue
            if "subprocess.run" in seg and "radix=" in seg.replace(" ", ""):
                # `radix = subprocess.run("python3 pseudo.py 32 <curve>").returncode`: run that generator through refgen instead
                script = "pseudo.py" if ns["prime_type"] == ns["PSEUDO"] else "monty.py"
                g = refgen.load(script, WL, custom["field_arg"] if custom is not None else curve)
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
    small_x = "#define CONSTANT_X" in open(os.path.join(scratch, "curve.c")).read()
    return ctypes.CDLL(so, mode=os.RTLD_LAZY), "ecn_%s_" % curve.lower(), ns["limbs"], ns["Nbytes"], ns["radix"], scratch, small_x


def fixture(curve, seed, records, wild, custom=None):
    lib, pre, N, nb, radix, _, small_x = build(curve, custom)

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
    if not small_x:
        f("gen")(ref(G))
    else:
        # ecnXXXgen would take a square root (addchain); the same point from its affine coordinates (tests/golden/edwards_*.json /
        # weierstrass_*.json "gen", the reference's sign choice) through the reference's own nres and modone
        gx, gy = gio.load("%s_%s.json" % (KIND[curve], curve))["gen"]
        U = ctypes.c_uint32 * N
        def limbs(v):
            return U(*[(v >> (radix * i)) & ((1 << radix) - 1) for i in range(N)])
        lib.nres.argtypes = [U, U]; lib.nres.restype = None
        lib.modone.argtypes = [U]; lib.modone.restype = None
        lib.nres(limbs(int(gx, 16)), G.x); lib.nres(limbs(int(gy, 16)), G.y); lib.modone(G.z)
    fx = {"curve": curve, "wl": WL, "N": N, "Nbytes": nb, "radix": radix, "seed": seed, "small_x": int(small_x), "gen": H(G),
          "source": "reference edwards.c / weierstrass.c + curve.py 32 + generator-emitted 32-bit field code, built by tests/golden/make_curveref_w32_gen.py"}
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
    # big-integer fixtures (edwards_*.json / weierstrass_*.json "set_xy", on and off the curve); for a custom curve, plain integer
    # multiples of its generator and one point off the curve
    if custom is None:
        aff = gio.load("%s_%s.json" % (KIND[curve], curve))
    else:
        pts = affine_multiples(custom, 6)
        hx = lambda v: v.to_bytes(nb, "big").hex()
        aff = {"set_xy": [{"x": hx(x), "y": hx(y), "valid": 1} for x, y in pts] + [{"x": hx(pts[1][0]), "y": hx((pts[1][1] + 1) % custom["p"]), "valid": 0}]}
        fx["custom"] = {k: (hex(v) if isinstance(v, int) and abs(v) > 1 << 32 else v) for k, v in custom.items()}
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
    for k, c in enumerate(CURVES + (CUSTOM,)):
        if only and c not in only:
            continue
        custom = custom_curve(c) if c == CUSTOM else None
        fx = fixture(c, 33000 + k, 6 if c in ("NIST384", "ED376", "NIST521", "ED500") else 8, 10, custom)      # 8 records at 9 limbs, 6 at 14 and 18
        gio.dump(fx, "curveref_w32_%s.json" % c)
        print(c, fx["N"], "x", fx["radix"], len(fx["records"]), "records,", len(fx["wild"]), "wild; small x:", fx["small_x"], "gen x limb 0:", fx["gen"][0][0], flush=True)


if __name__ == "__main__":
    main()
