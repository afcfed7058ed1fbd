"""CPU-side checks of the boundary of the curve layer at word length 32 (include/modarith_amd_w32_curve.h) and of its driver: the library
exports every declared symbol; _lib's curve tables of that word length cover the header exactly; the header compiles as C; the ABI
version is unchanged; the emitted constants (csrc/generated/w32_curve_<CURVE>.h) are what emit.py emits, carry the reference's
generator limbs (tests/golden/curveref_w32_<CURVE>.json.xz "gen") and the curve's b by value."""
import os
import re
import subprocess

import pytest

from modarith_amd import curves, emit
from modarith_amd.params import derive
from tests.golden import gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
CURVES = ("ED25519", "NIST256", "ED448")


@pytest.fixture(scope="module")
def lib():
    from modarith_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _declared():
    text = open(os.path.join(INC, "modarith_amd_w32_curve.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    macro = text[text.index("#define MODARITH_AMD_DECLARE_W32_CURVE(c, NL)"):text.index("MODARITH_AMD_DECLARE_W32_CURVE(ed25519")]
    fns = re.findall(r"\becn_##c##_w32_(\w+)\s*\(", macro)
    inst = re.findall(r"^MODARITH_AMD_DECLARE_W32_CURVE\((\w+), (\d+)\)", text, flags=re.M)
    return fns, inst


def test_every_declared_symbol_is_exported(lib):
    fns, inst = _declared()
    assert [c for c, _ in inst] == [c.lower() for c in CURVES] and tuple(CURVES) == emit.W32_CURVES
    assert len(fns) == len(set(fns)) == 16 + 17
    missing = ["ecn_%s_w32_%s" % (c, f) for c, _ in inst for f in fns if not hasattr(lib, "ecn_%s_w32_%s" % (c, f))]
    assert not missing, missing
    assert lib.modarith_amd_abi_version() == 2
    for c, nl in inst:
        assert int(nl) == derive(_field(c.upper()), wl=32).nlimbs


def _field(name):
    return (curves.CURVES[name] if name in curves.CURVES else curves.W_CURVES[name]).field


def test_binding_tables_cover_header():
    from modarith_amd import _lib
    fns, inst = _declared()
    bound = {f + "_batch" for f in _lib.W32_ED_BATCH_FUNCS} | set(_lib.W32_ED_SCALAR_FUNCS)
    assert bound == set(fns)
    assert sorted(_lib.W32_CURVES) == sorted(c for c, _ in inst)
    for c, nl in inst:
        fp = derive(_field(c.upper()), wl=32)
        assert _lib.W32_CURVES[c] == (int(nl), fp.nbytes) == (fp.nlimbs, fp.nbytes)
    assert "mul2_exact" not in _lib.W32_ED_BATCH_FUNCS and "mul2_exact" in _lib.ED_BATCH_FUNCS
    # nothing of this header went into the tables tests/test_abi_w32_cpu.py counts
    assert not any(n.startswith("ecn") for n in _lib.W32_BATCH_FUNCS + _lib.W32_SCALAR_FUNCS + _lib.W32_UTIL_FUNCS)


def test_header_compiles_as_c(tmp_path):
    src = tmp_path / "use.c"
    src.write_text('#include "modarith_amd_w32_curve.h"\n'
                   "int use(void) { ma_point_ed25519_w32_t p; ma_point_ed448_w32_t q; ma_point_nist256_w32_t r; ecn_ed25519_w32_gen(&p); ecn_ed448_w32_inf(&q); ecn_nist256_w32_dbl(&r);\n"
                   "  return (int)(sizeof p.x / sizeof p.x[0] + sizeof q.z / sizeof q.z[0] + sizeof r) + ecn_ed25519_w32_isinf(&p); }\n")
    subprocess.run(["gcc", "-std=c99", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(src)], check=True)


@pytest.mark.parametrize("name", CURVES)
def test_emitted_constants(name):
    text = emit.w32_curve_header_text(name)
    assert open(os.path.join(emit.GEN_DIR, "w32_curve_%s.h" % name)).read() == text          # the committed header is what the driver emits
    g = gio.load("curveref_w32_%s.json" % name)
    edw = name in curves.CURVES
    c = curves.CURVES[name] if edw else curves.W_CURVES[name]
    fp = derive(c.field, wl=32)
    assert (g["N"], g["radix"], g["Nbytes"]) == (fp.nlimbs, fp.radix, fp.nbytes)
    assert "struct C_%s_W32 {" % name in text and "using FieldParams = P_%s_W32;" % c.field in text and "namespace ma32 {" in text

    def limbs(member):
        body = re.search(r"\b%s\(int i\) \{ switch \(i\) \{(.*?)default" % member, text).group(1)
        return [int(v, 16) for v in re.findall(r"return (0x[0-9a-f]+)ull", body)]
    assert [hex(v) for v in limbs("gx")] == g["gen"][0] and [hex(v) for v in limbs("gy")] == g["gen"][1]
    # b, lifted into the field, is the curve constant by value (Montgomery form where the field has one)
    lift = lambda ls: sum(v << (fp.radix * i) for i, v in enumerate(ls)) * (pow(fp.R, -1, fp.p) if fp.montgomery else 1) % fp.p
    bval = c.d if edw else c.b
    if edw and c.small_b:
        assert "B_SMALL = true" in text and ("B_INT = %d;" % bval) in text
    else:
        assert len(limbs("b")) == fp.nlimbs and lift(limbs("b")) == bval % fp.p
        if not edw:
            assert lift(limbs("b3")) == 3 * bval % fp.p
    assert lift(limbs("gx")) == c.gx and lift(limbs("gy")) == c.gy
    assert ("A = %d" % c.a) in text and "SMALL_X = 0;" in text
