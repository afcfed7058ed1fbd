"""Generated curves at word length 32 (modarith_amd.generate.generate_curve(..., wl=32)) against the reference's emitted C
(`curve.py 32 <CURVE>`), on the HOST, limb for limb.

tools/curve_w32_gen_host.hip compiles the classes the kernels of a generated plug-in wrap -- ma32::Edwards / ma32::Weierstrass over the
emitted w32_curve_<CURVE>.h and params_<TAG>_w32.h (emit_only: the texts, no device compile) -- for the CPU;
tests/golden/curveref_w32_<CURVE>.json.xz holds what the reference's own edwards.c / weierstrass.c return for the eight curves of
curve.py's table that are not built in at this word length and for CURVE1174 over the generated field 2^251 - 9
(tests/golden/make_curveref_w32_gen.py).  Every record of every fixture runs -- chained, wild, special, set from both coordinates --
with no tolerance, and the number of records compared is the number in the fixture.  The generator is compared limb for limb, except
on the five curves whose generator is given by a small x: there gen() takes the field's square root (a chain of its own), and the
point is compared by cmp against the fixture's generator, as tests/test_gpu_curveref.py does at 64 bits.  set from one coordinate and
affine are pinned by value, as in tests/test_w32_curve_host.py."""
import os
import shutil
import subprocess

import pytest

from modarith_amd import generate as gen
from tests.golden import gio
from tests.test_w32_curve_host import Host

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
KIND = {"SECP256K1": "weierstrass", "NUMS256W": "weierstrass", "NUMS256E": "edwards", "ED248": "edwards", "NIST384": "weierstrass",
        "ED376": "edwards", "NIST521": "weierstrass", "ED500": "edwards", "CURVE1174": "edwards"}
CURVES = tuple(KIND)
SMALL_X = ("NUMS256W", "NUMS256E", "ED248", "ED376", "ED500")
RECORDS = {c: (6 if c in ("NIST384", "ED376", "NIST521", "ED500") else 8) for c in CURVES}

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (host compile of the HIP headers)")


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("w32cg"))
    gen.generate_w32("2**251-9", plugin_dir=tmp, emit_only=True)
    for c in CURVES:
        spec = dict(gen.EXAMPLE_CURVES[0]) if c == "CURVE1174" else gen.named_curve(c)
        gen.generate_curve(**spec, wl=32, plugin_dir=tmp, emit_only=True)
    with open(os.path.join(tmp, "curves.inc"), "w") as f:
        f.write("".join('#include "w32_curve_%s.h"\n' % c for c in CURVES))
        f.write("#define W32CG_CURVES(X) " + " ".join("X(%s, %s)" % (c, KIND[c].capitalize()) for c in CURVES) + "\n")
    cc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "modarith_amd", "csrc")
    exe = os.path.join(tmp, "curve_w32_gen_host")
    cmd = [cc, "-O1", "-std=c++17", "-w", "--offload-host-only", "-I", os.path.join(csrc, "generated"), "-I", csrc, "-I", tmp, "-I", gen.PLUGIN_DIR,
           '-DW32CG_LIST="curves.inc"', os.path.join(ROOT, "tools", "curve_w32_gen_host.hip"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    return Host(exe)


@pytest.mark.parametrize("curve", CURVES)
def test_chained_records_limb_for_limb(host, curve):
    g = gio.load("curveref_w32_%s.json" % curve)
    assert g["wl"] == 32 and len(g["records"]) == RECORDS[curve]
    reqs, want = [], []
    def ask(tag, fn, P=None, Q=None, e=None, f=None, s=0, rows=None, ret=None):
        reqs.append((fn, P, Q, e, f, s)); want.append((tag, rows, ret))
    for k, r in enumerate(g["records"]):
        t = "record %d " % k
        ask(t + "mul", "mul", r["P"], e=r["e"], rows=r["M"])
        ask(t + "dbl", "dbl", r["M"], rows=r["D"])
        ask(t + "add", "add", r["M"], r["D"], rows=r["A"])
        ask(t + "sub", "sub", r["A"], r["D"], rows=r["S"])
        ask(t + "neg", "neg", r["A"], rows=r["N"])
        ask(t + "cof", "cof", r["A"], rows=r["C"])
        ask(t + "mul2", "mul2", r["M"], r["D"], r["e"], r["f"], rows=r["R"])
        ask(t + "A+N", "add", r["A"], r["N"], rows=r["A+N"])
        ask(t + "A+N isinf", "isinf", r["A+N"], ret=r["A+N_isinf"])
        ask(t + "A+A", "add", r["A"], r["A"], rows=r["A+A"])
        for nm, fl in zip("MDAR", r["isinf"]):
            ask(t + "isinf " + nm, "isinf", r[nm], ret=fl)
        ask(t + "cpy", "cpy", r["P"], r["A"], rows=r["A"])
        ask(t + "cmp", "cmp", r["S"], r["M"], ret=1)                                  # (M + D) - D is M, by value
    assert {g["records"][k]["e"] for k in (1, 2, 3)} == {"%0*x" % (2 * g["Nbytes"], 1), "00" * g["Nbytes"], "ff" * g["Nbytes"]}      # the scalar edge cases
    got = host.run(curve, reqs)
    assert len(got) == 16 * len(g["records"])                                         # none skipped
    bad = [(tag, rows, gr) for (tag, rows, ret), (gret, gr) in zip(want, got) if (rows is not None and gr != rows) or (ret is not None and gret != ret)]
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(reqs), bad[0])


@pytest.mark.parametrize("curve", CURVES)
def test_wild_records_limb_for_limb(host, curve):
    """arbitrary 32-bit limb patterns: what separates `every limb pattern` from `in-contract points`"""
    g = gio.load("curveref_w32_%s.json" % curve)
    W = g["wild"]
    assert len(W) == 10 and any(all(v == "0xffffffff" for row in r["P"] for v in row) for r in W)
    reqs, want = [], []
    for k, r in enumerate(W):
        for tag, fn, Q, key in (("dbl", "dbl", None, "D"), ("add", "add", r["Q"], "A"), ("neg", "neg", None, "N"), ("mul", "mul", None, "M"), ("mul2", "mul2", r["Q"], "R")):
            reqs.append((fn, r["P"], Q, r["e"], r["f"], 0)); want.append(("wild %d %s" % (k, tag), r[key]))
        reqs.append(("isinf", r["P"], None, None, None, 0)); want.append(("wild %d isinf" % k, r["isinf"]))
    got = host.run(curve, reqs)
    assert len(got) == 6 * len(W)
    bad = [(tag, w, gr) for (tag, w), (gret, gr) in zip(want, got) if (gret != w if isinstance(w, int) else gr != w)]
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(reqs), bad[0])


@pytest.mark.parametrize("curve", CURVES)
def test_generator_special_cases_and_set(host, curve):
    g = gio.load("curveref_w32_%s.json" % curve)
    sp, G = g["special"], g["gen"]
    assert bool(g["small_x"]) == (curve in SMALL_X)
    reqs = [("gen", None, None, None, None, 0), ("inf", None, None, None, None, 0), ("dbl", sp["inf"], None, None, None, 0),
            ("add", G, sp["inf"], None, None, 0), ("add", sp["inf"], G, None, None, 0), ("isinf", sp["inf"], None, None, None, 0), ("isinf", G, None, None, None, 0)]
    got = host.run(curve, reqs)
    assert [r for _, r in got[1:5]] == [sp["inf"], sp["dbl_inf"], sp["gen+inf"], sp["inf+gen"]]
    assert [got[5][0], got[6][0]] == [1, 0]
    if curve in SMALL_X:
        # gen() recovers y with the field's square root: the reference's point (its sign choice included), by value, z = 1
        assert host.run(curve, [("cmp", got[0][1], G, None, None, 0)])[0][0] == 1 and got[0][1][2] == G[2]
    else:
        assert got[0][1] == G
    recs = g["set_xy"]
    assert any(r["isinf"] for r in recs) and not all(r["isinf"] for r in recs)          # on- and off-curve input
    got = host.run(curve, [("setxy", None, None, r["x"], r["y"], 0) for r in recs])
    assert len(got) == len(recs) and [r for _, r in got] == [r["P"] for r in recs]
    got = host.run(curve, [("isinf", r["P"], None, None, None, 0) for r in recs])
    assert [v for v, _ in got] == [r["isinf"] for r in recs]


@pytest.mark.parametrize("curve", CURVES)
def test_set_from_one_coordinate_and_affine_by_value(host, curve):
    """the functions that run the square-root / inversion chains, by value: set from x (and, on the Edwards curves, from y) with either
    sign is the fixture's point or its negative; affine(k * P) equals P scaled back (cmp), with z = 1"""
    g = gio.load("curveref_w32_%s.json" % curve)
    on = [r for r in g["set_xy"] if not r["isinf"]]
    modes = ("setx", "sety") if KIND[curve] == "edwards" else ("setx",)
    for mode in modes:
        got = [host.run(curve, [(mode, None, None, r["x"], r["y"], s) for r in on]) for s in (0, 1)]
        cmp0 = host.run(curve, [("cmp", a[1], r["P"], None, None, 0) for a, r in zip(got[0], on)])
        cmp1 = host.run(curve, [("cmp", a[1], r["P"], None, None, 0) for a, r in zip(got[1], on)])
        assert [a[0] + b[0] for a, b in zip(cmp0, cmp1)] == [1] * len(on), mode              # exactly one sign gives the point itself
        assert [v for v, _ in host.run(curve, [("isinf", a[1], None, None, None, 0) for a in got[0] + got[1]])] == [0] * (2 * len(on)), mode
    A = [r["A"] for r in g["records"] if not r["isinf"][2]]
    aff = host.run(curve, [("affine", a, None, None, None, 0) for a in A])
    one = host.run(curve, [("setxy", None, None, on[0]["x"], on[0]["y"], 0)])[0][1][2]       # z of a point set from coordinates: the field's 1
    assert all(r[2] == one for _, r in aff)
    assert [v for v, _ in host.run(curve, [("cmp", a[1], b, None, None, 0) for a, b in zip(aff, A)])] == [1] * len(A)
