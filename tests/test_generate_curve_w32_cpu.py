"""generate_curve(..., wl=32), CPU side: the texts the driver emits for a curve on uint32_t points (emit_only: no compiler) -- the eight
curves of curve.py's table that are not built in at word length 32 and CURVE1174 over the generated field 2^251 - 9 -- checked against
modarith_amd/curves.py and plain integers; the refusals; the listings of the two word lengths; what Curve(name, wl=32) says without a
plug-in.  The limbs are checked on the host in tests/test_w32_curve_gen_host.py, the kernels on the GPU in tests/test_gpu_w32_curve_gen.py."""
import json
import os
import re

import pytest

from modarith_amd import curves, emit, generate as gen

# curve -> (limbs, radix, family, Nbytes, generator from a small x): what `curve.py 32 <CURVE>` over `pseudo.py 32` / `monty.py 32` prints
SHAPES = {"SECP256K1": (9, 29, "monty", 32, False), "NUMS256W": (9, 29, "pseudo", 32, True), "NUMS256E": (9, 29, "pseudo", 32, True),
          "ED248": (9, 29, "monty", 32, True), "NIST384": (14, 28, "monty", 48, False), "ED376": (14, 28, "monty", 48, True),
          "NIST521": (18, 29, "pseudo", 66, False), "ED500": (18, 29, "monty", 64, True), "CURVE1174": (9, 28, "pseudo", 32, False)}
CUSTOM = gen.EXAMPLE_CURVES[0]


def spec_of(name):
    return dict(CUSTOM) if name == "CURVE1174" else gen.named_curve(name)


@pytest.fixture(scope="module")
def emitted(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("w32curves"))
    gen.generate_w32("2**251-9", plugin_dir=d, emit_only=True)              # CURVE1174's field, by its tag
    out = {name: gen.generate_curve(**spec_of(name), wl=32, plugin_dir=d, emit_only=True) for name in SHAPES}
    return d, out


def switch_values(text, fn):
    m = re.search(r"static constexpr unsigned long long %s\(int i\) \{ switch \(i\) \{(.*?)default" % fn, text)
    assert m, fn
    return [int(v, 16) for v in re.findall(r"case \d+: return (0x[0-9a-f]+)ull;", m.group(1))]


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_emitted_texts(emitted, name):
    d, out = emitted
    g, spec = out[name], spec_of(name)
    N, radix, family, nbytes, small_x = SHAPES[name]
    field = spec["field"]
    fp = gen.resolve("2**251-9", wl=32) if name == "CURVE1174" else gen.resolve(field, wl=32)
    assert (fp.nlimbs, fp.radix, fp.family, fp.nbytes) == (N, radix, family, nbytes)
    assert (g.name, g.kind, g.field, g.nlimbs, g.nbytes, g.built) == (name, spec["kind"], field, N, nbytes, False)
    assert not os.path.exists(g.lib) and g.lib == gen.curve_plugin_path(name, d, 32) and g.lib.endswith("libmodarith_amd_curve_%s_w32.so" % name.lower())
    hdr = open(os.path.join(d, "w32_curve_%s.h" % name)).read()
    assert "namespace ma32 {" in hdr and "struct C_%s_W32 {" % name in hdr and "using FieldParams = P_%s_W32;" % field in hdr
    # the field's struct: emitted next to the curve, unless the field is already generated in the default directory (then it is read there)
    assert '#include "params_%s_w32.h"' % field in hdr
    where = next(w for w in (d, gen.PLUGIN_DIR) if os.path.exists(os.path.join(w, "params_%s_w32.h" % field)))
    assert "struct P_%s_W32 {" % field in open(os.path.join(where, "params_%s_w32.h" % field)).read()
    gx, gy, b, a = spec["gx"], spec["gy"], spec["b"], spec["a"]
    assert (abs(gx) < 1 << 28) == small_x
    assert "static constexpr int SMALL_X = %d;" % (gx if small_x else 0) in hdr
    internal = lambda v: fp.to_limbs((v * fp.R if fp.montgomery else v) % fp.p, masked_top=True)
    assert switch_values(hdr, "gx") == internal(gx) and switch_values(hdr, "gy") == internal(gy)
    for limbs in (switch_values(hdr, "gx"), switch_values(hdr, "gy")):
        assert len(limbs) == N and all(v < 1 << radix for v in limbs)
    if spec["kind"] == "edwards":
        assert "static constexpr int A = %d, COF = %d;" % (a, spec["cof"]) in hdr
        assert abs(b) < 1 << 28 and "static constexpr bool B_SMALL = true;" in hdr and "static constexpr int B_INT = %d;" % b in hdr
        cls = "ma32::Edwards<ma32::C_%s_W32>" % name
    else:
        assert "static constexpr int A = %d, COF = 0;" % a in hdr
        assert "static constexpr int SMALL_B = %d;" % (b if abs(b) < 1 << 28 else 0) in hdr
        assert switch_values(hdr, "b") == internal(b) and switch_values(hdr, "b3") == internal(3 * b)
        cls = "ma32::Weierstrass<ma32::C_%s_W32>" % name
    unit = open(os.path.join(d, "capi_curve_%s_w32.hip" % name)).read()
    # resident waves per SIMD, per limb count, family and curve form: 9 limbs 4 (pseudo-Mersenne Edwards) or 3, 14 limbs 2, 18 limbs 2
    # (ED500: no scratch; NIST521: the measured choice between two waves with a prologue-only spill and one wave, docs/curve_layer.md)
    wps = {"SECP256K1": 3, "NUMS256W": 3, "NUMS256E": 4, "ED248": 3, "NIST384": 2, "ED376": 2, "NIST521": 2, "ED500": 2, "CURVE1174": 4}[name]
    assert emit.W32_MUL_WPS_18_WEIERSTRASS == 2
    for line in ("MODARITH_AMD_DECLARE_W32_CURVE(%s, %d)" % (name.lower(), N), "#define MA_MUL_WPS %d" % wps, '#include "w32_curve_%s.h"' % name,
                 "#define MA_CURVE_CLASS %s" % cls, "#define MA_CNAME %s_w32" % name.lower(), '#include "capi_curve.inc"'):
        assert line + "\n" in unit, line
    assert unit.index("#define MA_MUL_WPS") < unit.index('#include "w32_curve_')          # curve.h reads it
    # the digit arrays of the resident grid fit the LDS of a CU (the static_assert of k_ed_mul), 521-bit scalars included
    assert 4 * wps * 2 * (2 * nbytes + 1) * 64 <= 160 * 1024


def test_launch_width_rule():
    """the built-in three keep what their hand-written units define; 14 limbs run two waves per SIMD"""
    csrc = os.path.join(os.path.dirname(emit.__file__), "csrc")
    for c, key in (("ED25519", (9, False, "edwards")), ("NIST256", (9, True, "weierstrass")), ("ED448", (16, True, "edwards"))):
        text = open(os.path.join(csrc, "capi_%s_w32_ecn.hip" % c)).read()
        assert "#define MA_MUL_WPS %d\n" % emit.w32_curve_mul_wps(*key) in text
    assert emit.w32_curve_mul_wps(14, True, "weierstrass") == 2 and emit.w32_curve_mul_wps(14, True, "edwards") == 2
    assert emit.W32_CURVES == ("ED25519", "NIST256", "ED448")                  # the eight others are plug-ins, not part of the main library


def test_refusals(tmp_path):
    d = str(tmp_path)
    for name in emit.W32_CURVES:                                               # built in at THIS word length
        with pytest.raises(gen.GenerateError, match="built-in curve at word length 32"):
            gen.generate_named_curve(name, wl=32, plugin_dir=d, emit_only=True)
    spec = gen.named_curve("NIST384")
    with pytest.raises(gen.GenerateError, match="not on the curve"):
        gen.generate_curve(**dict(spec, gy=spec["gy"] + 1), wl=32, plugin_dir=d, emit_only=True)
    with pytest.raises(gen.GenerateError, match="a = -3 and a = 0"):
        gen.generate_curve(**dict(spec, a=-2), wl=32, plugin_dir=d, emit_only=True)
    e = gen.named_curve("ED500")
    with pytest.raises(gen.GenerateError, match="a = 1 and a = -1"):
        gen.generate_curve(**dict(e, a=2), wl=32, plugin_dir=d, emit_only=True)
    c = dict(CUSTOM)
    gen.generate_w32("2**251-9", plugin_dir=d, emit_only=True)
    with pytest.raises(gen.GenerateError, match="not on the curve"):
        gen.generate_curve(**dict(c, gx=c["gx"] + 1), wl=32, plugin_dir=d, emit_only=True)
    with pytest.raises(gen.GenerateError, match="neither built in at word length 32"):
        gen.generate_curve(**dict(c, field="NOSUCHFIELD"), wl=32, plugin_dir=d, emit_only=True)
    with pytest.raises(gen.GenerateError, match="kind must be"):
        gen.generate_curve(**dict(c, kind="montgomery"), wl=32, plugin_dir=d, emit_only=True)
    with pytest.raises(gen.GenerateError, match="_w32"):
        gen.generate_curve(**dict(c, name="MINE_w32"), wl=32, plugin_dir=d, emit_only=True)
    with pytest.raises(gen.GenerateError):
        gen.generate_curve(**spec, wl=16, plugin_dir=d)
    with pytest.raises(gen.GenerateError, match="built-in curve"):             # the 64-bit path is what it was: all eleven are built in there
        gen.generate_curve(**spec, plugin_dir=d)
    assert not [f for f in os.listdir(d) if f.endswith(".so")]


def test_listings_keep_the_word_lengths_apart(tmp_path):
    """installed_curves() lists one word length: a plug-in counts where its shared object is present and its metadata carries that `wl`"""
    d = str(tmp_path)

    def install(name, wl):
        open(gen.curve_plugin_path(name, d, wl), "wb").close()
        meta = {"curve": name, "kind": "weierstrass", "field": name, "a": -3, "b": "0x1", "nlimbs": 14, "nbytes": 48}
        if wl == 32:
            meta["wl"] = 32
        json.dump(meta, open(os.path.join(d, "curve_%s%s.json" % (name, "" if wl == 64 else "_w32")), "w"))
    assert gen.curve_plugin_path("NIST384", d) != gen.curve_plugin_path("NIST384", d, 32)
    install("NIST384", 32)
    assert gen.installed_curves(d) == [] and [m["curve"] for m in gen.installed_curves(d, wl=32)] == ["NIST384"]
    install("MINE", 64)
    assert [m["curve"] for m in gen.installed_curves(d)] == ["MINE"] and [m["curve"] for m in gen.installed_curves(d, wl=32)] == ["NIST384"]
    assert gen.installed(d) == [] and gen.installed(d, wl=32) == []            # curves are not fields


def test_curve_without_a_plug_in_names_the_built_in_three(tmp_path):
    from modarith_amd.edwards import Curve
    with pytest.raises(ValueError) as ei:
        Curve("NIST384", wl=32, plugin_dir=str(tmp_path))
    msg = str(ei.value)
    assert all(c in msg for c in ("ED25519", "NIST256", "ED448")) and "generated: none" in msg


def test_command_line_verb_refuses_a_built_in_name():
    assert gen.main(["curve32", "ED25519"]) == 2 and gen.main(["curve32"]) == 2 and gen.main(["curve32", "NOSUCHCURVE"]) == 2
