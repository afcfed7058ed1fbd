"""CPU-side checks of the 32-bit word form's boundary (include/modarith_amd_w32.h): the library loads without a GPU and exports every
declared symbol; _lib's 32-bit tables cover the header exactly; the emitted paste-marker shims are what the driver emits, compile as C,
define all 32 names and carry the macro values the reference prints at word length 32; field_info agrees with derive(P, wl=32)."""
import ctypes
import os
import re
import subprocess

import pytest

from modarith_amd import emit
from modarith_amd.params import derive
from tests.golden import gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
W32 = ("X25519", "NIST256", "X448")


@pytest.fixture(scope="module")
def lib():
    from modarith_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _declared():
    text = open(os.path.join(INC, "modarith_amd_w32.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    names = set(re.findall(r"\b(modarith_amd_w32_\w+)\s*\(", text))
    macro = text[text.index("#define MODARITH_AMD_DECLARE_W32(P)"):text.index("MODARITH_AMD_DECLARE_W32(X25519)")]
    per_prime = re.findall(r"\b(\w+)_##P##_w32_(ct|batch)\s*\(", macro)
    primes = re.findall(r"^MODARITH_AMD_DECLARE_W32\((\w+)\)", text, flags=re.M)
    for fn, kind in per_prime:
        for P in primes:
            names.add("%s_%s_w32_%s" % (fn, P, kind))
    return sorted(names), primes, per_prime


def test_every_declared_symbol_is_exported(lib):
    names, primes, per_prime = _declared()
    assert tuple(primes) == W32 == emit.W32_PRIMES
    assert sorted(f for f, k in per_prime if k == "ct") == sorted(emit.FIELD_C_NAMES) and len(emit.FIELD_C_NAMES) == 32
    assert set(emit.FIELD_C_NAMES) <= {f for f, k in per_prime if k == "batch"}
    assert len(names) == 3 * (32 + 34) + 4
    missing = [n for n in names if not hasattr(lib, n)]
    assert not missing, missing
    assert "typedef uint32_t ma_spint32;" in open(os.path.join(INC, "modarith_amd_w32.h")).read()
    assert lib.modarith_amd_abi_version() == 2


def test_binding_tables_cover_header(lib):
    from modarith_amd import _lib
    names, _, _ = _declared()
    bound = {"%s_%s_w32_batch" % (f, P) for f in _lib.W32_BATCH_FUNCS for P in _lib.W32_PRIMES}
    bound |= {"%s_%s_w32_ct" % (f, P) for f in _lib.W32_SCALAR_FUNCS for P in _lib.W32_PRIMES}
    bound |= set(_lib.W32_UTIL_FUNCS)
    assert bound == set(names)
    assert _lib.W32_PRIMES == W32 and not set(_lib.W32_ABSENT) & set(_lib.W32_BATCH_FUNCS)
    # the 64-bit tables are what they were
    assert _lib.PRIMES == emit.BUILT_PRIMES and "modmuls" in _lib.BATCH_FUNCS


def test_field_info_matches_driver(lib):
    for P in W32:
        vals = [ctypes.c_int() for _ in range(5)]
        assert lib.modarith_amd_w32_field_info(P.encode(), *[ctypes.byref(v) for v in vals]) == 1
        fp = derive(P, wl=32)
        assert [v.value for v in vals] == [fp.nlimbs, fp.radix, fp.n, fp.nbytes, int(fp.montgomery)]
    assert lib.modarith_amd_w32_field_info(b"NIST521", None, None, None, None, None) == 0
    words = lib.modarith_amd_w32_batch_words
    assert words(1000, 9, 1000) == 9000 and words(8192, 9, 4096) == 2 * 9 * 4096 and words(8193, 16, 4096) == 3 * 16 * 4096
    assert words(5, 0, 5) == 0


@pytest.mark.parametrize("P", W32)
def test_shim_header(P, tmp_path):
    fp = derive(P, wl=32)
    path = os.path.join(INC, "field_%s_w32.h" % P)
    text = open(path).read()
    assert text == emit.field_shim_text(fp)
    c = tmp_path / "use.c"
    c.write_text('#include "field_%s_w32.h"\nint main(void) { spint a[Nlimbs] = {0}, b[Nlimbs] = {0}; dpint t = 0; sspint s = 0; modmul(a, b, a); modsqr(a, a); (void)t; (void)s; '
                 'return modis0(a) + (int)sizeof(spint) + Wordlength; }\n' % P)
    r = subprocess.run(["gcc", "-fsyntax-only", "-Wall", "-Werror", "-I", INC, str(c)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    defs = dict(re.findall(r"^#define (\w+) ?(.*)$", text, flags=re.M))
    for fn in emit.FIELD_C_NAMES:
        assert defs[fn] == "%s_%s_w32_ct" % (fn, P)
    # the macro block of the reference's field.c at word length 32 (values only, tests/golden/field_w32_<P>.json.xz)
    m = gio.load("field_w32_%s.json" % P)["params"]["macros"]
    for k in ("Wordlength", "Nlimbs", "Radix", "Nbits", "Nbytes"):
        assert int(defs[k]) == m[k], k
    for k in ("spint", "sspint", "dpint", "sdpint"):
        assert defs[k] == m[k], k
    for k in ("MERSENNE", "MONTGOMERY", "MULBYINT", P):
        assert (k in defs) == (k in m), k
    assert set(m) - {"Wordlength", "Nlimbs", "Radix", "Nbits", "Nbytes", "spint", "sspint", "dpint", "sdpint"} <= set(defs)
    # the 64-bit shim of the same prime is untouched
    assert open(os.path.join(INC, "field_%s.h" % P)).read() == emit.field_shim_text(derive(P))
