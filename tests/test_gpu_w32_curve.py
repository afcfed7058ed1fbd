"""The curve layer at word length 32 on the GPU (include/modarith_amd_w32_curve.h, Curve(name, wl=32)) against the projective limbs of the
reference's own edwards.c / weierstrass.c built by `curve.py 32` (tests/golden/curveref_w32_<CURVE>.json.xz), limb for limb, wild
records -- arbitrary 32-bit limb patterns -- in the same batches as legitimate ones; the scalar entry points; more points than the
resident grid; by value against the 64-bit curve layer and the big-integer fixtures; refusals and aliasing."""
import ctypes

import numpy as np
import pytest

from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
CURVES = ["ED25519", "NIST256", "ED448"]
KIND = {"ED25519": "edwards", "NIST256": "weierstrass", "ED448": "edwards"}
N_LANES = 200           # three full waves and an 8-lane tail (the scalar multiplications run one wave per workgroup with a tail guard)


@pytest.fixture(scope="module", params=CURVES)
def cx(request):
    import torch
    assert torch.cuda.is_available()
    from modarith_amd.edwards import Curve
    name = request.param
    return name, Curve(name, wl=32), load_golden("curveref_w32_%s.json" % name), torch


def rows_np(points):
    """list of [[x limbs], [y limbs], [z limbs]] (hex) -> uint32 [3, N, n]"""
    a = np.array([[[int(v, 16) for v in row] for row in p] for p in points], dtype=np.uint32)          # [n, 3, N]
    return np.ascontiguousarray(a.transpose(1, 2, 0))


def batch(torch, points, ld=None):
    """-> int32 device tensor [3, N, ld] whose first n columns are the points (the rest: a pattern no function may touch)"""
    a = rows_np(points)
    n = a.shape[2]
    if ld is not None and ld > n:
        pad = np.full(a.shape[:2] + (ld - n,), 0xA5A5A5A5, dtype=np.uint32)
        a = np.ascontiguousarray(np.concatenate([a, pad], axis=2))
    return torch.from_numpy(a.view(np.int32)).cuda()


def unbatch(t, n=None):
    a = t.cpu().numpy().view(np.uint32)
    return [[[hex(int(v)) for v in a[c, :, j]] for c in range(3)] for j in range(a.shape[2] if n is None else n)]


def scalars(torch, hexes):
    return torch.tensor([list(bytes.fromhex(h)) for h in hexes], dtype=torch.uint8, device="cuda")


class Raw:
    """the batched entry points with n and ld given separately (the Curve class always passes ld = n)"""

    def __init__(self, W, torch, n, ld):
        self.W, self.torch, self.n, self.ld = W, torch, n, ld
        self.ws = torch.empty(int(getattr(W.lib, "ecn_%s_mul_workspace_bytes" % W._sym)(n)), dtype=torch.uint8, device="cuda")

    def __call__(self, fn, *args):
        from modarith_amd import _lib
        p = lambda a: a.data_ptr() if hasattr(a, "data_ptr") else a
        tail = (self.ws.data_ptr(), self.ws.numel(), None) if fn in ("mul", "mul2") else (None,)
        _lib.check(getattr(self.W.lib, "ecn_%s_%s_batch" % (self.W._sym, fn))(*[p(a) for a in args], self.n, self.ld, *tail), fn)
        self.torch.cuda.synchronize()


@pytest.mark.parametrize("ld", [N_LANES, 256])
def test_records_limb_for_limb(cx, ld):
    """every fixture record meets several lane positions (the records are cycled over 200 lanes); every fourth lane carries a WILD
    record where the function has one, so that arbitrary limbs sit next to legitimate points: neighbours must be unaffected"""
    name, W, g, torch = cx
    R, Wd = g["records"], g["wild"]
    n = N_LANES
    call = Raw(W, torch, n, ld)
    lane = [("w", Wd[(j // 4) % len(Wd)]) if j % 4 == 3 else ("r", R[(j - j // 4) % len(R)]) for j in range(n)]
    assert {id(r) for _, r in lane} == {id(r) for r in R + Wd}

    def col(legit, wild=None):
        """per lane: the legitimate record's entry, or the wild record's (where the function has wild records; else the wild point P)"""
        return [(r[legit] if k == "r" else r[wild or "P"]) for k, r in lane]

    def check(t, legit, wild, what):
        got = unbatch(t, n)
        want = col(legit, wild)
        bad = [j for j in range(n) if (lane[j][0] == "r" or wild) and got[j] != want[j]]
        assert not bad, "%s: lanes %s differ (ld %d)" % (what, bad[:8], ld)
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
    X = batch(torch, [sp["inf"]] * n, ld); call("gen", X); assert unbatch(X, n) == [G] * n
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
    """the same records through Curve(name, wl=32): names and argument order of the 64-bit class"""
    name, W, g, torch = cx
    R = g["records"]
    col = lambda k: [r[k] for r in R]
    e, f = scalars(torch, col("e")), scalars(torch, col("f"))
    assert W.empty(3).dtype == torch.int32 and tuple(W.empty(3).shape) == (3, g["N"], 3) and W.nbytes == g["Nbytes"]
    assert unbatch(W.gen(3)) == [g["gen"]] * 3 and unbatch(W.inf(2)) == [g["special"]["inf"]] * 2
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
    with pytest.raises(ValueError):
        W.mul(e, M.to(torch.int64))
    with pytest.raises(ValueError):
        W.mul_get(e, M)


@pytest.mark.parametrize("name", CURVES)
def test_scalar_entry_points(name):
    """ecn_<c>_w32_* (host pointers, the reference's signatures over uint32_t points, one point through the GPU): every function once"""
    from modarith_amd import _lib
    lib = _lib.load()
    g = load_golden("curveref_w32_%s.json" % name)
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
    X = Pt(); f("gen")(ref(X)); assert rows(X) == g["gen"]
    O = Pt(); f("inf")(ref(O)); assert rows(O) == sp["inf"] and f("isinf")(ref(O)) == 1 and f("isinf")(ref(X)) == 0
    for r in g["records"][:2] + g["records"][3:4]:
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
    w = g["wild"][0]
    M = point(w["P"]); f("mul")(bytes.fromhex(w["e"]), ref(M)); assert rows(M) == w["M"]
    s = next(r for r in g["set_xy"] if not r["isinf"])
    P = Pt(); f("set")(0, bytes.fromhex(s["x"]), bytes.fromhex(s["y"]), ref(P)); assert rows(P) == s["P"]
    D = point(s["P"]); f("dbl")(ref(D)); D2 = point(rows(D))
    x, y = ctypes.create_string_buffer(nb), ctypes.create_string_buffer(nb)
    f("get")(ref(P), x, y)
    assert (x.raw.hex(), y.raw.hex()) == (s["x"], s["y"])
    f("get")(ref(D), x, y)                                   # a projective point: get makes it affine in place, same point
    assert f("cmp")(ref(D), ref(D2)) == 1


def test_more_points_than_the_resident_grid():
    """ED25519: MUL_MAX_LANES + 70 points -- the pass loop of k_ed_mul and the reuse of a wave's table slab -- compared on the device"""
    import torch
    from modarith_amd.edwards import Curve
    W = Curve("ED25519", wl=32)
    g = load_golden("curveref_w32_ED25519.json")
    wsb = getattr(W.lib, "ecn_ed25519_w32_mul_workspace_bytes")
    per_lane = int(wsb(64)) // 64
    max_lanes = int(wsb(1 << 30)) // per_lane
    assert max_lanes % 64 == 0 and int(wsb(max_lanes + 70)) == max_lanes * per_lane
    n = max_lanes + 70
    recs = g["records"] + g["wild"]
    idx = torch.arange(n, device="cuda") % len(recs)
    P = batch(torch, [r["P"] for r in recs])[:, :, idx].contiguous()
    want = batch(torch, [r["M"] for r in recs])[:, :, idx].contiguous()
    e = scalars(torch, [r["e"] for r in recs])[idx].contiguous()
    got = W.mul(e, P)
    assert int((got != want).any(dim=0).any(dim=0).sum()) == 0


@pytest.mark.parametrize("name", CURVES)
def test_by_value_across_word_lengths(name):
    """get(mul(e, gen)) at word length 32 returns the bytes of the 64-bit curve layer for the same 200 random scalars; get / affine / set
    from one coordinate and its sign (inversion and square-root chains: by value, as everywhere) agree with the big-integer fixtures"""
    import random
    import torch
    from modarith_amd.edwards import Curve
    W32, W64 = Curve(name, wl=32), Curve(name)
    nb = W32.nbytes
    assert nb == W64.nbytes
    rng = random.Random(3232)
    n = N_LANES
    es = [rng.getrandbits(8 * nb - 3) for _ in range(n)]
    es[0], es[1], es[2] = 0, 1, (1 << (8 * nb)) - 1
    e = torch.tensor([list(k.to_bytes(nb, "big")) for k in es], dtype=torch.uint8, device="cuda")
    x32, y32, _ = W32.get(W32.mul(e, W32.gen(n)))
    x64, y64, _ = W64.get(W64.mul(e, W64.gen(n)))
    assert torch.equal(x32, x64) and torch.equal(y32, y64)
    x32b, _, s32 = W32.get(W32.mul(e, W32.gen(n)), want_y=False)
    _, _, s64 = W64.get(W64.mul(e, W64.gen(n)), want_y=False)
    assert torch.equal(x32b, x64) and torch.equal(s32, s64)

    g = load_golden("%s_%s.json" % (KIND[name], name))
    recs = g["compress"]
    xs, ys = scalars(torch, [r["x"] for r in recs]), scalars(torch, [r["y"] for r in recs])
    valid = [int(r["valid"]) for r in recs]
    xy_of = lambda P: [[bytes(a).hex(), bytes(b).hex()] for a, b in zip(*[t.cpu().numpy() for t in W32.get(P.clone())[:2]])]
    forms = [(W32.set(torch.tensor([int(r["sy"]) for r in recs], dtype=torch.int32, device="cuda"), xs, None), "sy", (True, False))]
    if KIND[name] == "edwards":
        forms.append((W32.set(torch.tensor([int(r["sx"]) for r in recs], dtype=torch.int32, device="cuda"), None, ys), "sx", (False, True)))
    else:
        with pytest.raises(Exception):
            W32.set(None, None, ys)                          # weierstrass.c needs x
    for P, skey, (gx, gy) in forms:
        assert W32.isinf(P).cpu().tolist() == [1 - v for v in valid]
        for r, xy in zip(recs, xy_of(P)):
            if int(r["valid"]):
                assert xy == [r["x"], r["y"]]
        _, _, sign = W32.get(P.clone(), want_x=gx, want_y=gy)
        assert [s for s, v in zip(sign.cpu().tolist(), valid) if v] == [int(r[skey]) for r in recs if int(r["valid"])]
        Q = W32.dbl(P.clone())                               # affine of a projective point: the same point, z = 1
        Aq = W32.affine(Q.clone())
        assert W32.cmp(Aq, Q).cpu().tolist() == [1] * len(recs)
        one = W32.set(None, xs[:1].contiguous(), ys[:1].contiguous())[2, :, 0]
        assert all(torch.equal(Aq[2, :, j], one) for j in range(len(recs)) if valid[j])
    # the fixture's multiplications e*P = eP, affine in and out
    m = g["mul"]
    P = W32.set(None, scalars(torch, [r["P"][0] for r in m]), scalars(torch, [r["P"][1] for r in m]))
    out = W32.mul(scalars(torch, [r["e"] for r in m]), P)
    inf = W32.isinf(out).cpu().tolist()
    for r, xy, i in zip(m, xy_of(out), inf):
        if not i:
            assert xy == list(r["eP"])
    assert sum(inf) < len(m)


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
    assert b"workspace" in W.lib.modarith_amd_last_error()
    # mis-aligned scalar records: error status, outputs untouched
    raw = torch.zeros(e.numel() + 8, dtype=torch.uint8, device="cuda")
    off = next(k for k in range(1, 8) if (raw.data_ptr() + k) % 8)
    raw[off:off + e.numel()] = e.flatten()
    assert sym("mul")(raw.data_ptr() + off, P.data_ptr(), n, n, ws.data_ptr(), need, None) != 0
    assert sym("mul2")(e.data_ptr(), M.data_ptr(), raw.data_ptr() + off, D.data_ptr(), Rr.data_ptr(), n, n, ws.data_ptr(), need, None) != 0
    assert b"aligned" in W.lib.modarith_amd_last_error()
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


@pytest.mark.parametrize("name", ["SECP256K1", "NIST384", "ED248", "NUMS256W"])
def test_unbuilt_curves_are_refused_at_word_length_32(name):
    from modarith_amd.edwards import Curve, Edwards
    for cls in (Curve, Edwards):
        with pytest.raises(ValueError) as ei:
            cls(name, wl=32)
        assert all(c in str(ei.value) for c in CURVES)
    with pytest.raises(ValueError):
        Curve("ED25519", wl=16)
