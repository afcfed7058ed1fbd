"""Generated curves at word length 32 on the GPU: plug-ins of modarith_amd.generate.generate_curve(..., wl=32), loaded by
Curve(name, wl=32, plugin_dir=...), against the projective limbs of the reference's own edwards.c / weierstrass.c built by
`curve.py 32 <CURVE>` (tests/golden/curveref_w32_<CURVE>.json.xz), limb for limb, wild records in the same batches as legitimate ones.

The six plug-ins cover: Montgomery a = 0 (SECP256K1, 9 limbs); pseudo-Mersenne Edwards with a generator from a small x (NUMS256E);
14 limbs (NIST384); 18-limb pseudo-Mersenne with 66-byte records (NIST521); 18-limb Montgomery Edwards (ED500); and a curve of the
user's own over a generated field (CURVE1174 over 2^251 - 9).  They are generated into a directory of this module's own: nothing here
leaves a 32-bit curve plug-in in the default plug-in directory."""
import concurrent.futures as cf
import ctypes
import random

import numpy as np
import pytest

from tests.conftest import load_golden
from tests.test_gpu_w32_curve import N_LANES, Raw, batch, scalars, unbatch

pytestmark = pytest.mark.gpu
CURVES = ["SECP256K1", "NUMS256E", "NIST384", "NIST521", "ED500", "CURVE1174"]
TABLE = CURVES[:5]                                   # curves of curve.py's table: built in at word length 64
SMALL_X = ("NUMS256E", "ED500")
SHAPE = {"SECP256K1": (9, 32), "NUMS256E": (9, 32), "NIST384": (14, 48), "NIST521": (18, 66), "ED500": (18, 64), "CURVE1174": (9, 32)}


@pytest.fixture(scope="module")
def plugins(tmp_path_factory):
    import torch
    assert torch.cuda.is_available()
    from modarith_amd import generate as gen
    d = str(tmp_path_factory.mktemp("w32_curve_plugins"))
    gen.generate_w32("2**251-9", plugin_dir=d)                                 # CURVE1174's field, by its tag
    specs = [dict(gen.EXAMPLE_CURVES[0]) if c == "CURVE1174" else gen.named_curve(c) for c in CURVES]
    assert specs[-1]["name"] == "CURVE1174"
    with cf.ThreadPoolExecutor(max_workers=4) as ex:                           # four curves x (three parts + the field): at most 16 compiler jobs
        out = list(ex.map(lambda s: gen.generate_curve(**s, wl=32, plugin_dir=d), specs))
    assert [(g.name, g.nlimbs, g.nbytes) for g in out] == [(c,) + SHAPE[c] for c in CURVES]
    assert sorted(m["curve"] for m in gen.installed_curves(d, wl=32)) == sorted(CURVES) and gen.installed_curves(d) == []
    again = gen.generate_curve(**specs[0], wl=32, plugin_dir=d)                # up to date: reused, not compiled again
    assert not again.built and again.lib == out[0].lib
    return d


@pytest.fixture(scope="module", params=CURVES)
def cx(request, plugins):
    import torch
    from modarith_amd.edwards import Curve
    name = request.param
    W = Curve(name, wl=32, plugin_dir=plugins)
    assert (W.N, W.nbytes) == SHAPE[name] and W._sym == name.lower() + "_w32"
    return name, W, load_golden("curveref_w32_%s.json" % name), torch


@pytest.mark.parametrize("ld", [N_LANES, 256])
def test_records_limb_for_limb(cx, ld):
    """every fixture record meets several lane positions (the records are cycled over 200 lanes: three waves and an 8-lane tail); every
    fourth lane carries a WILD record where the function has one; beyond n a guard pattern no function may touch"""
    name, W, g, torch = cx
    R, Wd = g["records"], g["wild"]
    n = N_LANES
    call = Raw(W, torch, n, ld)
    lane = [("w", Wd[(j // 4) % len(Wd)]) if j % 4 == 3 else ("r", R[(j - j // 4) % len(R)]) for j in range(n)]
    assert {id(r) for _, r in lane} == {id(r) for r in R + Wd}

    def col(legit, wild=None):
        return [(r[legit] if k == "r" else r[wild or "P"]) for k, r in lane]

    def check(t, legit, wild, what):
        got = unbatch(t, n)
        want = col(legit, wild)
        bad = [j for j in range(n) if (lane[j][0] == "r" or wild) and got[j] != want[j]]
        assert not bad, "%s %s: lanes %s differ (ld %d)" % (name, what, bad[:8], ld)
        if ld > n:
            assert (t.cpu().numpy().view(np.uint32)[:, :, n:] == 0xA5A5A5A5).all(), what + ": wrote beyond n"

    e, f = scalars(torch, col("e", "e")), scalars(torch, col("f", "f"))
    M = batch(torch, col("P"), ld); call("mul", e, M); check(M, "M", "M", "mul")
    D = batch(torch, col("M"), ld); call("dbl", D); check(D, "D", "D", "dbl")
    A = batch(torch, col("M"), ld); call("add", batch(torch, col("D", "Q"), ld), A); check(A, "A", "A", "add")
    Ng = batch(torch, col("A"), ld); call("neg", Ng); check(Ng, "N", "N", "neg")
    Rr = batch(torch, col("P"), ld)
    call("mul2", e, batch(torch, col("M"), ld), f, batch(torch, col("D", "Q"), ld), Rr); check(Rr, "R", "R", "mul2")
    S = batch(torch, col("A"), ld); call("sub", batch(torch, col("D"), ld), S); check(S, "S", None, "sub")
    C = batch(torch, col("A"), ld); call("cof", C); check(C, "C", None, "cof")
    Z = batch(torch, col("A"), ld); call("add", batch(torch, col("N"), ld), Z); check(Z, "A+N", None, "P + (-P)")
    T = batch(torch, col("A"), ld); call("add", batch(torch, col("A"), ld), T); check(T, "A+A", None, "P + P through add")
    flag = torch.full((ld,), -7, dtype=torch.int32, device="cuda")
    for key, k in (("M", 0), ("D", 1), ("A", 2), ("R", 3)):
        call("isinf", batch(torch, col(key), ld), flag)
        got = flag.cpu().tolist()
        assert [got[j] for j in range(n) if lane[j][0] == "r"] == [r["isinf"][k] for kk, r in lane if kk == "r"], "isinf " + key
    call("isinf", batch(torch, col("A+N"), ld), flag)
    got = flag.cpu().tolist()
    assert [got[j] for j in range(n) if lane[j][0] == "r"] == [r["A+N_isinf"] for kk, r in lane if kk == "r"]
    assert [got[j] for j in range(n) if lane[j][0] == "w"] == [r["isinf"] for kk, r in lane if kk == "w"] and got[n:] == [-7] * (ld - n)
    call("cmp", batch(torch, col("S"), ld), batch(torch, col("M"), ld), flag)                # (M + D) - D is M, by value
    assert [v for j, v in enumerate(flag.cpu().tolist()[:n]) if lane[j][0] == "r"] == [1] * sum(1 for k, _ in lane if k == "r")
    Cp = batch(torch, col("P"), ld); call("cpy", batch(torch, col("A"), ld), Cp); check(Cp, "A", "P", "cpy")

    # generator, special cases, set from both coordinates
    sp, G = g["special"], g["gen"]
    X = batch(torch, [sp["inf"]] * n, ld); call("gen", X)
    if name in SMALL_X:
        # gen() recovers y with the field's square root (a chain of its own): the reference's point by value, z = 1
        call("cmp", X, batch(torch, [G] * n, ld), flag)
        assert flag.cpu().tolist()[:n] == [1] * n and [p[2] for p in unbatch(X, n)] == [G[2]] * n
    else:
        assert unbatch(X, n) == [G] * n
    O = batch(torch, [G] * n, ld); call("inf", O); assert unbatch(O, n) == [sp["inf"]] * n
    X = batch(torch, [sp["inf"]] * n, ld); call("dbl", X); assert unbatch(X, n) == [sp["dbl_inf"]] * n
    X = batch(torch, [G] * n, ld); call("add", O, X); assert unbatch(X, n) == [sp["gen+inf"]] * n
    X = batch(torch, [sp["inf"]] * n, ld); call("add", batch(torch, [G] * n, ld), X); assert unbatch(X, n) == [sp["inf+gen"]] * n
    recs = [g["set_xy"][j % len(g["set_xy"])] for j in range(n)]
    X = batch(torch, [G] * n, ld)
    call("set", None, scalars(torch, [r["x"] for r in recs]), scalars(torch, [r["y"] for r in recs]), X)
    assert unbatch(X, n) == [r["P"] for r in recs]
    call("isinf", X, flag)
    assert flag.cpu().tolist()[:n] == [r["isinf"] for r in recs]


def test_class_methods_return_the_references_limbs(cx):
    """the same records through Curve(name, wl=32, plugin_dir=...): names and argument order of the 64-bit class"""
    name, W, g, torch = cx
    R = g["records"]
    col = lambda k: [r[k] for r in R]
    e, f = scalars(torch, col("e")), scalars(torch, col("f"))
    assert W.empty(3).dtype == torch.int32 and tuple(W.empty(3).shape) == (3, g["N"], 3) and W.nbytes == g["Nbytes"]
    if name in SMALL_X:
        assert W.cmp(W.gen(3), batch(torch, [g["gen"]] * 3)).cpu().tolist() == [1] * 3
    else:
        assert unbatch(W.gen(3)) == [g["gen"]] * 3
    assert unbatch(W.inf(2)) == [g["special"]["inf"]] * 2
    M = W.mul(e, batch(torch, col("P")))
    assert unbatch(M) == col("M")
    D = W.dbl(M.clone())
    A = W.add(D, M.clone())
    assert unbatch(D) == col("D") and unbatch(A) == col("A") and unbatch(W.sub(D, A.clone())) == col("S")
    assert unbatch(W.neg(A.clone())) == col("N") and unbatch(W.cof(A.clone())) == col("C") and unbatch(W.cpy(A)) == col("A")
    assert unbatch(W.mul2(e, M, f, D)) == col("R") and unbatch(W.mul2(e, M, f, D, exact=True)) == col("R")
    assert [list(t) for t in zip(*[W.isinf(x).cpu().tolist() for x in (M, D, A, batch(torch, col("R")))])] == col("isinf")
    assert W.cmp(W.ran(3, A.clone()), A).cpu().tolist() == [1] * len(R)
    assert W.limbs_ok(A).cpu().tolist() == [1] * len(R) and W.limbs_ok(batch(torch, [g["wild"][0]["P"], R[0]["A"]])).cpu().tolist() == [0, 1]
    # get / set / affine: the inversion and square-root chains, by value
    on = [r for r in g["set_xy"] if not r["isinf"]]
    P = W.set(None, scalars(torch, [r["x"] for r in on]), scalars(torch, [r["y"] for r in on]))
    assert unbatch(P) == [r["P"] for r in on]
    Q = W.dbl(P.clone())
    Aq = W.affine(Q.clone())
    assert W.cmp(Aq, Q).cpu().tolist() == [1] * len(on) and all(torch.equal(Aq[2, :, j], P[2, :, 0]) for j in range(len(on)))
    x, y, _ = W.get(P.clone())
    assert [bytes(v).hex() for v in x.cpu().numpy()] == [r["x"] for r in on] and [bytes(v).hex() for v in y.cpu().numpy()] == [r["y"] for r in on]
    xq, _, sg = W.get(Q.clone(), want_y=False)
    back = W.set(sg, xq, None)                              # from x and the sign of y: the same point
    assert W.cmp(back, Q).cpu().tolist() == [1] * len(on)
    with pytest.raises(ValueError):
        W.mul(e, M.to(torch.int64))
    with pytest.raises(ValueError):
        W.mul_get(e, M)                                     # the fused byte-output forms stay refused at this word length


def test_scalar_entry_points(cx):
    """ecn_<c>_w32_* of the plug-in (host pointers, the reference's signatures over uint32_t points, one point through the GPU): every function once"""
    name, W, g, torch = cx
    lib = W.lib
    N, nb, c = g["N"], g["Nbytes"], name.lower()

    class Pt(ctypes.Structure):
        _fields_ = [("x", ctypes.c_uint32 * N), ("y", ctypes.c_uint32 * N), ("z", ctypes.c_uint32 * N)]
    def point(rows):
        p = Pt()
        for k, row in zip("xyz", rows):
            for i, v in enumerate(row):
                getattr(p, k)[i] = int(v, 16)
        return p
    rows = lambda p: [[hex(v) for v in getattr(p, k)] for k in "xyz"]
    f = lambda fn: getattr(lib, "ecn_%s_w32_%s" % (c, fn))
    ref = ctypes.byref
    sp = g["special"]
    X = Pt(); f("gen")(ref(X))
    Gp = point(g["gen"])
    assert f("cmp")(ref(X), ref(Gp)) == 1 and (name in SMALL_X or rows(X) == g["gen"])
    O = Pt(); f("inf")(ref(O)); assert rows(O) == sp["inf"] and f("isinf")(ref(O)) == 1 and f("isinf")(ref(X)) == 0
    r = g["records"][0]
    e, fb = bytes.fromhex(r["e"]), bytes.fromhex(r["f"])
    M = point(r["P"]); f("mul")(e, ref(M)); assert rows(M) == r["M"]
    D = point(r["M"]); f("dbl")(ref(D)); assert rows(D) == r["D"]
    A = point(r["M"]); f("add")(ref(D), ref(A)); assert rows(A) == r["A"]
    S = point(r["A"]); f("sub")(ref(D), ref(S)); assert rows(S) == r["S"]
    Ng = point(r["A"]); f("neg")(ref(Ng)); assert rows(Ng) == r["N"]
    C = point(r["A"]); f("cof")(ref(C)); assert rows(C) == r["C"]
    R = Pt(); f("mul2")(e, ref(M), fb, ref(D), ref(R)); assert rows(R) == r["R"], "scalar mul2"
    Y = Pt(); f("cpy")(ref(A), ref(Y)); assert rows(Y) == r["A"]
    assert f("cmp")(ref(S), ref(M)) == 1 and f("cmp")(ref(A), ref(M)) == (1 if r["isinf"][0] else 0)
    T = point(r["A"]); f("ran")(5, ref(T)); assert f("cmp")(ref(T), ref(A)) == 1
    T = point(r["A"]); f("affine")(ref(T)); assert f("cmp")(ref(T), ref(A)) == 1
    s = next(r for r in g["set_xy"] if not r["isinf"])
    P = Pt(); f("set")(0, bytes.fromhex(s["x"]), bytes.fromhex(s["y"]), ref(P)); assert rows(P) == s["P"]
    x, y = ctypes.create_string_buffer(nb), ctypes.create_string_buffer(nb)
    f("get")(ref(P), x, y)
    assert (x.raw.hex(), y.raw.hex()) == (s["x"], s["y"])


@pytest.mark.parametrize("name", TABLE)
def test_by_value_across_word_lengths(plugins, name):
    """get(mul(e, gen)) at word length 32 returns the bytes of the built-in 64-bit curve for the same 200 scalars, 0, 1 and all-ones among them"""
    import torch
    from modarith_amd.edwards import Curve
    W32, W64 = Curve(name, wl=32, plugin_dir=plugins), Curve(name)
    nb = W32.nbytes
    assert nb == W64.nbytes
    rng = random.Random(3264)
    n = N_LANES
    es = [rng.getrandbits(8 * nb - 3) for _ in range(n)]
    es[0], es[1], es[2] = 0, 1, (1 << (8 * nb)) - 1
    e = torch.tensor([list(k.to_bytes(nb, "big")) for k in es], dtype=torch.uint8, device="cuda")
    x32, y32, _ = W32.get(W32.mul(e, W32.gen(n)))
    x64, y64, _ = W64.get(W64.mul(e, W64.gen(n)))
    assert torch.equal(x32, x64) and torch.equal(y32, y64)
    assert W32.isinf(W32.mul(e, W32.gen(n))).cpu().tolist() == W64.isinf(W64.mul(e, W64.gen(n))).cpu().tolist()


def test_refusals_and_aliasing(cx):
    name, W, g, torch = cx
    from modarith_amd import _lib
    R = g["records"]
    n = len(R)
    col = lambda k: [r[k] for r in R]
    e, f = scalars(torch, col("e")), scalars(torch, col("f"))
    sym = lambda fn: getattr(W.lib, "ecn_%s_%s_batch" % (W._sym, fn))
    need = int(getattr(W.lib, "ecn_%s_mul_workspace_bytes" % W._sym)(n))
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    P, M, D = batch(torch, col("P")), batch(torch, col("M")), batch(torch, col("D"))
    Rr = batch(torch, col("P"))
    # workspace too small / missing: error status, outputs untouched
    assert sym("mul")(e.data_ptr(), P.data_ptr(), n, n, ws.data_ptr(), need - 1, None) != 0
    assert sym("mul")(e.data_ptr(), P.data_ptr(), n, n, None, need, None) != 0
    assert sym("mul2")(e.data_ptr(), M.data_ptr(), f.data_ptr(), D.data_ptr(), Rr.data_ptr(), n, n, ws.data_ptr(), need - 1, None) != 0
    assert b"workspace" in _lib.load().modarith_amd_last_error()           # (the plug-in records its errors in the main library)
    if g["Nbytes"] % 8 == 0:
        # mis-aligned scalar records (records that move as 64-bit words): error status, outputs untouched
        raw = torch.zeros(e.numel() + 8, dtype=torch.uint8, device="cuda")
        off = next(k for k in range(1, 8) if (raw.data_ptr() + k) % 8)
        raw[off:off + e.numel()] = e.flatten()
        assert sym("mul")(raw.data_ptr() + off, P.data_ptr(), n, n, ws.data_ptr(), need, None) != 0
        assert sym("mul2")(e.data_ptr(), M.data_ptr(), raw.data_ptr() + off, D.data_ptr(), Rr.data_ptr(), n, n, ws.data_ptr(), need, None) != 0
        assert b"aligned" in _lib.load().modarith_amd_last_error()
    else:
        assert name == "NIST521"                           # 66-byte records move byte by byte: no alignment to refuse
    torch.cuda.synchronize()
    assert unbatch(P) == col("P") and unbatch(Rr) == col("P") and unbatch(M) == col("M")
    # the same calls with what they need succeed
    _lib.check(sym("mul")(e.data_ptr(), P.data_ptr(), n, n, ws.data_ptr(), need, None), "mul")
    assert unbatch(P) == col("M")
    # aliasing: add(P, P) and cpy in place
    A = batch(torch, col("A"))
    _lib.check(sym("add")(A.data_ptr(), A.data_ptr(), n, n, None), "add")
    assert unbatch(A) == col("A+A")
    A = batch(torch, col("A"))
    _lib.check(sym("cpy")(A.data_ptr(), A.data_ptr(), n, n, None), "cpy")
    assert unbatch(A) == col("A")


def test_nothing_is_left_in_the_default_plug_in_directory(plugins):
    from modarith_amd import generate as gen
    assert plugins != gen.PLUGIN_DIR
    assert not {m["curve"] for m in gen.installed_curves(wl=32)} & {"SECP256K1", "NIST384", "ED248", "NUMS256W"}
