"""Generator mode at word length 32 (modarith_amd.generate.generate_w32), CPU side: tags and refusals are resolve()'s at that word
length, a plug-in cross-compiles, exports the whole 32-bit per-prime C-ABI, depends on the main library only, is reused, and lives
next to the 64-bit plug-in of the same tag; the CLI verb; the shim header; the driver's closure computation for the shared
inversion against the hand-derived bounds of csrc/kernels.h; and the register budget of the streaming kernels of every example.
No compute (no GPU here): the words are checked on the host in tests/test_w32_gen_host.py and on the GPU in tests/test_gpu_w32_gen.py."""
import math
import os
import subprocess
import sys

import pytest

from modarith_amd import _lib, emit, generate as gen
from modarith_amd.params import derive, w32_inv_closure, w32_inv_in_contract
from tests import w32_gen_inputs as gi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BP256 = "BP256=0xa9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377"


@pytest.fixture
def main_library():
    """the tests that cross-compile a plug-in link it against the built library: a tree without it is a broken build, not a reason to skip"""
    assert os.path.exists(_lib.LIB_PATH), "%s is missing: run __graft_entry__.build() first" % _lib.LIB_PATH


def test_tags_and_shapes_at_word_length_32():
    assert gen.resolve("2**255-19", wl=32).name == "25519"
    fp = gen.resolve("2**251-9", wl=32)
    assert (fp.name, fp.family, fp.nlimbs, fp.radix, fp.wl) == ("2519", "pseudo", 9, 28, 32)
    fp = gen.resolve("2**130-5", wl=32)
    assert (fp.name, fp.nlimbs, fp.radix) == ("1305", 5, 26)
    fp = gen.resolve(BP256, wl=32)
    assert (fp.name, fp.family, fp.nlimbs, fp.radix) == ("BP256", "monty", 9, 29) and fp.ndash != 1
    with pytest.raises(gen.GenerateError, match="must have a name"):
        gen.resolve(BP256.split("=")[1], wl=32)
    assert gen.resolve("GM240", wl=32).radix == 29 and gen.resolve("NIST521", wl=32).radix == 29      # params.RADIX_32
    assert gen.resolve("GM240", wl=32, radix=27).radix == 27                                          # an explicit radix wins
    assert gen.resolve("SECP256K1", wl=32).family == "monty"                                          # as `monty.py 32 SECP256K1`
    with pytest.raises(gen.GenerateError, match="exploitable pseudo-Mersenne"):
        gen.resolve("SECP256K1", family="pseudo", wl=32)
    assert gen.resolve("M2519=2**251-9", family="monty", wl=32).family == "monty"
    q = 2**252 + 27742317777372353535851937790883648493
    assert gen.resolve("Q25519=00%d" % q, wl=32).p == q
    assert gen.resolve("2**251-9").radix == 51                                                        # the 64-bit resolution is untouched


def test_refusals():
    with pytest.raises(gen.GenerateError, match="sensible modulus"):
        gen.generate_w32("2**89-1")
    with pytest.raises(gen.GenerateError, match="sensible modulus"):
        gen.generate_w32("2**255-21")
    with pytest.raises(gen.GenerateError, match="starts with a digit"):
        gen.generate_w32("NOSUCHPRIME")
    with pytest.raises(gen.GenerateError, match="C identifier"):
        gen.generate_w32("a-b=2**255-19")
    with pytest.raises(gen.GenerateError, match="built-in field"):
        gen.generate_w32("X25519=2**251-9")
    for wl in (64, 32):                                                        # <TAG>_w32 names the 32-bit plug-in of <TAG>
        with pytest.raises(gen.GenerateError, match="cannot end in _w32"):
            gen.resolve("FOO_w32=2**255-19", wl=wl)
    for name in ("SIDH610", "SIDH751"):                                        # 22 and 26 limbs at this word length
        assert derive(name, wl=32).nlimbs > emit.MAX_GENERATED_LIMBS_W32 >= 18
        with pytest.raises(gen.GenerateError, match="at most 18 limbs"):
            gen.generate_w32(name)
    for name in ("NIST521", "PM512", "GM512"):                                 # the 18-limb named moduli are inside the cap
        assert derive(name, wl=32).nlimbs == 18
    # the three built-in primes need no plug-in; the 64-bit entry keeps refusing this word length, and says where to go
    for name in _lib.W32_PRIMES:
        g = gen.generate_w32(name)
        assert g.tag == name and not g.built and g.lib == _lib.LIB_PATH and g.params.wl == 32
    with pytest.raises(gen.GenerateError, match="64-bit.*generate_w32"):
        gen.generate("2**255-19", wl=32)


def test_plugin_cross_compiles_exports_the_abi_is_reused_and_coexists(main_library, tmp_path):
    d = str(tmp_path)
    g = gen.generate_w32("2**130-5", plugin_dir=d)
    assert g.built and g.tag == "1305" and (g.params.nlimbs, g.params.radix, g.params.wl) == (5, 26, 32)
    assert g.lib == gen.plugin_path("1305", d, wl=32) and os.path.basename(g.lib) == "libmodarith_amd_1305_w32.so"
    for f in ("params_1305_w32.h", "capi_1305_w32.hip", "field_1305_w32.h", "libmodarith_amd_1305_w32.so", "1305_w32.json"):
        assert os.path.exists(os.path.join(d, f)), f
    assert open(os.path.join(d, "params_1305_w32.h")).read() == emit.header_text(g.params, generated=True)
    assert open(os.path.join(d, "field_1305_w32.h")).read() == emit.field_shim_text(g.params)
    unit = open(os.path.join(d, "capi_1305_w32.hip")).read()
    assert '#include "capi_w32.inc"' in unit and "#define MA_P ma32::P_1305_W32" in unit and "#define MA_W32_EPT_MAX 4" in unit
    lib = _lib.load_plugin("1305", g.lib, wl=32)
    for fn in _lib.W32_BATCH_FUNCS:
        assert hasattr(lib, "%s_1305_w32_batch" % fn), fn
    for fn in _lib.W32_SCALAR_FUNCS:
        assert hasattr(lib, "%s_1305_w32_ct" % fn), fn
    needed = [l for l in subprocess.run(["readelf", "-d", g.lib], capture_output=True, text=True).stdout.splitlines() if "NEEDED" in l]
    assert any("libmodarith_amd.so" in l for l in needed) and not any("libmodarith_amd_" in l for l in needed)
    assert not gen.generate_w32("2**130-5", plugin_dir=d).built                 # reused
    # the default listing stays the 64-bit one; wl=32 lists and reads the new plug-ins
    assert gen.installed(d) == [] and [m["tag"] for m in gen.installed(d, wl=32)] == ["1305"]
    m = gen.installed(d, wl=32)[0]
    assert m["wl"] == 32 and (m["nlimbs"], m["radix"], m["ept_max"]) == (5, 26, 4)
    fp = gen.params_of_plugin("1305", d, wl=32)
    assert (fp.p, fp.family, fp.wl, fp.nlimbs) == (2**130 - 5, "pseudo", 32, 5)
    # ... next to the 64-bit plug-in of the same tag
    g64 = gen.generate("2**130-5", plugin_dir=d)
    assert g64.built and g64.lib != g.lib and os.path.exists(g.lib)
    assert [m["tag"] for m in gen.installed(d)] == ["1305"] and [m["tag"] for m in gen.installed(d, wl=32)] == ["1305"]
    assert gen.params_of_plugin("1305", d).nlimbs == 3 and gen.params_of_plugin("1305", d, wl=32).nlimbs == 5
    assert not gen.generate_w32("2**130-5", plugin_dir=d).built and not gen.generate("2**130-5", plugin_dir=d).built


def test_cli_verb(main_library, tmp_path):
    env = dict(os.environ, MA_PLUGIN_DIR=str(tmp_path))
    run = lambda *a: subprocess.run([sys.executable, "-m", "modarith_amd.generate"] + list(a), capture_output=True, text=True, cwd=ROOT, env=env)
    p = run("w32", "2**130-5")
    assert p.returncode == 0, p.stdout + p.stderr
    assert "Chosen radix is 26 bits, using 5 limbs" in p.stdout and "built" in p.stdout and "1305_w32_batch" in p.stdout and "Field('1305', wl=32)" in p.stdout
    assert "at most 4 elements per lane" in p.stdout and "closure shown" in p.stdout
    assert os.path.exists(os.path.join(str(tmp_path), "libmodarith_amd_1305_w32.so"))
    p = run("w32", "2**130-5")
    assert p.returncode == 0 and "up to date" in p.stdout
    p = run("--list")
    assert p.returncode == 0 and "1305" in p.stdout and "32-bit words" in p.stdout
    p = run("w32", "X448")
    assert p.returncode == 0 and "Chosen radix is 28 bits, using 16 limbs" in p.stdout and "up to date" in p.stdout
    p = run("w32", "SIDH751")
    assert p.returncode == 2 and "at most 18 limbs" in p.stdout
    p = run("w32", BP256.split("=")[1])
    assert p.returncode == 2 and "must have a name" in p.stdout
    p = run("w32", "SECP256K1", "--pseudo")
    assert p.returncode == 2 and "exploitable pseudo-Mersenne" in p.stdout
    p = run("w32")
    assert p.returncode == 2 and "Syntax error" in p.stdout
    # python -m modarith_amd.fuse 32 <generated tag>: the chain over the plug-in's parameter struct, cross-compiled next to it
    fuse = lambda *a: subprocess.run([sys.executable, "-m", "modarith_amd.fuse"] + list(a), capture_output=True, text=True, cwd=ROOT, env=env)
    text = "in x, y; out modsqr(modmul(modadd(x, y), modsub(x, y)))"
    p = fuse("32", "1305", "cli", text, "--source")
    assert p.returncode == 0, p.stdout + p.stderr
    assert '#include "params_1305_w32.h"' in p.stdout and "using P = ma32::P_1305_W32;" in p.stdout and "chain_cli_1305_w32_batch" in p.stdout
    p = fuse("32", "1305", "cli", text)
    assert p.returncode == 0 and "built" in p.stdout and "chain_cli_1305_w32_batch" in p.stdout, p.stdout + p.stderr
    assert os.path.exists(os.path.join(str(tmp_path), "libmodarith_amd_chain_cli_1305_w32.so"))
    p = fuse("32", "1305", "cli", text)
    assert p.returncode == 0 and "up to date" in p.stdout
    p = fuse("32", "NIST521", "cli", text)                                     # not generated at this word length
    assert p.returncode == 2 and "32-bit word form is built for" in p.stdout


def test_shim_header_of_a_generated_field():
    fp = gen.resolve(BP256, wl=32)
    text = emit.field_shim_text(fp)
    assert '#include "modarith_amd_w32.h"' in text and "MODARITH_AMD_DECLARE_W32(BP256)" in text
    assert "#define Wordlength 32" in text and "#define Nlimbs 9" in text and "#define Radix 29" in text and "#define Nbits 256" in text and "#define Nbytes 32" in text
    assert "#define spint uint32_t" in text and "#define dpint uint64_t" in text and "#define MONTGOMERY" in text and "#define BP256\n" in text
    for fn in emit.FIELD_C_NAMES:
        assert "#define %s %s_BP256_w32_ct\n" % (fn, fn) in text
    t2 = emit.field_shim_text(gen.resolve("2**251-9", wl=32))
    assert "#define MERSENNE" in t2 and "#define modmul modmul_2519_w32_ct" in t2 and "#define 2519" not in t2
    # the shims of the built-in primes declare nothing themselves (modarith_amd_w32.h does) and are unchanged
    for P in emit.W32_PRIMES:
        assert "MODARITH_AMD_DECLARE_W32" not in emit.field_shim_text(derive(P, wl=32))
        assert open(os.path.join(ROOT, "include", "field_%s_w32.h" % P)).read() == emit.field_shim_text(derive(P, wl=32))
        # ... and their parameter structs do not carry the verdict: csrc/capi_w32.inc detects the member
        assert "INV_CLOSED" not in emit.header_text(derive(P, wl=32))
        assert open(os.path.join(ROOT, "modarith_amd", "csrc", "generated", "w32_%s.h" % P)).read() == emit.header_text(derive(P, wl=32))
    assert "static constexpr bool INV_CLOSED = true;" in emit.header_text(fp, generated=True)
    assert "static constexpr bool INV_CLOSED = false;" in emit.header_text(gen.resolve("PM512", wl=32), generated=True)


def test_inversion_closure_reproduces_the_hand_derived_bounds():
    """the comment above inv_in_contract in csrc/kernels.h: X25519 -- TOPB 24, row 0 folds below 6.1 * 2^58 so the carried high part
    is below 6.1 * 2^29, at most 2^15 reaches limb 1, columns below 2^62; NIST256 -- TOPB 25, columns below 2^62; X448 -- TOPB 29,
    columns below 2^61"""
    c = {P: w32_inv_closure(derive(P, wl=32)) for P in _lib.W32_PRIMES}
    assert all(v["closed"] and not v["why"] for v in c.values())
    assert [c[P]["topb"] for P in ("X25519", "NIST256", "X448")] == [24, 25, 29]
    x = c["X25519"]
    assert 6.0 * 2**29 < x["hi"] < 6.1 * 2**29 and 2**13 <= x["slack"] < 2**15 and 2**60 < x["column"] < 2**62
    assert 2**61 < c["NIST256"]["column"] < 2**62 and c["NIST256"]["slack"] == 0
    assert 2**60 < c["X448"]["column"] < 2**61 and c["X448"]["slack"] == 0
    for v in c.values():
        assert abs(v["column_bits"] - math.log2(v["column"])) < 0.01
    # what a single limb at 2^31 - 1 breaks is outside the predicate; the predicate is the restatement, the closure the proof
    fp = derive("X25519", wl=32)
    assert not w32_inv_in_contract(fp, [(1 << 31) - 1] + [0] * 8) and w32_inv_in_contract(fp, [(1 << 29) - 1] * 8 + [(1 << 24) - 1])
    with pytest.raises(ValueError):
        w32_inv_closure(derive("X25519"))


def test_closure_bounds_the_scratch_word_of_the_reduction():
    """monty_reduce keeps the +-1-limb digits of the columns past the negative limb in one 32-bit word that starts at the mask: with
    eleven +1 limbs behind a -1 limb at radix 29 it would wrap, and the driver must not call such a prime closed (a made-up limb
    pattern on GM360's shape: the computation reads the limbs, not the prime)"""
    import dataclasses
    fp = derive("GM360", wl=32)
    assert (fp.nlimbs, fp.radix) == (13, 29) and w32_inv_closure(fp)["closed"]
    c = w32_inv_closure(dataclasses.replace(fp, ppw=[1, -1] + [1] * 11))
    assert not c["closed"] and "scratch word" in c["why"]
    assert w32_inv_closure(dataclasses.replace(fp, ppw=[1, -1] + [1] * 6 + [0] * 5))["closed"]      # 7 mask-sized words still fit


def test_closure_verdicts_of_the_examples():
    """closed for every example but PM512, whose bad_overflow form the proof does not cover: that field keeps one inversion per element.
    Two spare bits without a virtual limb are not enough for (a b + q p) / R < 2p on operands below 2^(Nbits+1)"""
    got = {t: w32_inv_closure(gi.params(t))["closed"] for t, _, _ in gi.examples()}
    assert got == {"2519": True, "1305": True, "BP256": True, "NIST384": True, "GM240": True, "PM512": False, "Q25519": True, "M2519": True}
    assert "bad_overflow" in w32_inv_closure(gi.params("PM512"))["why"]
    tight = gen.resolve("NIST224", wl=32)
    assert tight.E and w32_inv_closure(tight)["closed"]                       # no spare bits, but the virtual limb: R = 2^(Nbits+28)


@pytest.mark.parametrize("tag,arg,fam", gi.examples())
def test_streaming_kernels_of_every_example_stay_in_registers(main_library, tag, arg, fam):
    """from the code object of the example's plug-in (cross-compiled here; reused when build() made it): no k_binary / k_unary / k_mli /
    k_cond has scratch or accumulation registers, at any width the unit compiles -- and it compiles no width beyond MA_W32_EPT_MAX"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    g = gen.generate_w32(arg, family=fam)
    obj = os.path.join(os.path.dirname(g.lib), "capi_%s_w32.o" % tag)
    ks = [k for k in kernel_resources.kernels_of(obj) if any(s in k["name"] for s in ("::k_binary<", "::k_unary<", "::k_mli<", "::k_cond<"))]
    assert len(ks) >= 20, [k["name"] for k in ks]
    bad = [(k["name"][:100], k["vgpr_count"], k["agpr_count"], k["private_segment_fixed_size"]) for k in ks
           if k["private_segment_fixed_size"] or k["agpr_count"] or k["vgpr_spill_count"]]
    assert not bad, bad
    emax = emit.w32_ept_max(g.params.nlimbs)
    widths = {int(k["name"].split(">(")[0].rsplit(",", 1)[1]) for k in ks if "::k_binary<" in k["name"]}
    assert widths == {w for w in (1, 2, 4) if w <= emax}, widths
    assert any("k_inv_simul" in k["name"] for k in kernel_resources.kernels_of(obj)) == w32_inv_closure(g.params)["closed"]
