"""derive(P, wl=32) against what the reference generators derive at word length 32 (tests/golden/field_w32_<P>.json.xz "params":
values captured from `pseudo.py 32 X25519`, `monty.py 32 NIST256`, `monty.py 32 X448`), field for field; and derive(P) with no word
length is the 64-bit derivation, unchanged."""
import dataclasses

import pytest

from modarith_amd import emit
from modarith_amd.params import NAMED, derive
from tests.golden import gio

W32 = ("X25519", "NIST256", "X448")


def _int(v):
    return int(v, 16) if isinstance(v, str) else v


@pytest.mark.parametrize("P", W32)
def test_derive_w32_equals_the_reference(P):
    ref = gio.load("field_w32_%s.json" % P)["params"]
    fp = derive(P, wl=32)
    m = ref["macros"]
    assert ref["WL"] == 32 == fp.wl and m["Wordlength"] == 32
    assert (m["spint"], m["sspint"], m["dpint"]) == ("uint32_t", "int32_t", "uint64_t")
    assert (fp.nlimbs, fp.radix, fp.n, fp.nbytes) == (ref["N"], ref["base"], ref["n"], ref["Nbytes"]) == (m["Nlimbs"], m["Radix"], m["Nbits"], m["Nbytes"])
    assert fp.xcess == ref["xcess"] and fp.pm1d2 == ref["PM1D2"] and fp.pe == _int(ref["PE"]) and fp.p == _int(ref["p"])
    assert fp.m == _int(ref["m"])
    assert fp.roi == ref["ROI"]
    assert fp.montgomery == ("MONTGOMERY" in m) and (not fp.montgomery) == ("MERSENNE" in m)
    assert ("MULBYINT" in m) == ((not fp.montgomery) or fp.trin > 0)
    assert ref["karatsuba"] is False
    if fp.montgomery:
        assert fp.ppw == ref["ppw"] and fp.r2 == ref["cw"]
        assert (fp.E, fp.trin, fp.ndash, fp.pm) == (ref["E"], ref["trin"], ref["ndash"], ref["PM"])
        assert fp.R == 1 << (fp.radix * (fp.nlimbs + (1 if fp.E else 0)))
    else:
        assert (fp.mm, fp.tw) == (_int(ref["mm"]), _int(ref["TW"]))
        assert (fp.epm, fp.fred, fp.carry_on, fp.overflow) == (ref["EPM"], ref["fred"], ref["carry_on"], ref["overflow"])
        assert fp.bad_overflow == ref["bad_overflow_mul"] == ref["bad_overflow_sqr"]


def test_the_values_the_generators_choose():
    x, n, g = derive("X25519", wl=32), derive("NIST256", wl=32), derive("X448", wl=32)
    assert (x.nlimbs, x.radix, x.xcess, x.overflow, x.epm, x.fred, x.mm) == (9, 29, 6, True, False, False, 19 << 6)
    assert (n.nlimbs, n.radix, n.xcess, n.ndash) == (9, 29, 5, 1)
    assert (g.nlimbs, g.radix, g.xcess, g.E, g.trin, g.ndash) == (16, 28, 0, True, 8, 1)


@pytest.mark.parametrize("P", sorted(NAMED))
def test_default_word_length_is_64_and_unchanged(P):
    try:
        a = derive(P)
    except ValueError:
        with pytest.raises(ValueError):
            derive(P, wl=64)
        return
    assert a.wl == 64 and dataclasses.asdict(a) == dataclasses.asdict(derive(P, wl=64))


def test_other_word_lengths_are_refused():
    with pytest.raises(ValueError):
        derive("X25519", wl=16)


@pytest.mark.parametrize("P", W32)
def test_w32_header_text(P):
    """the parameter struct of the 32-bit form: a name and a namespace of its own, no split products, the progenitor chain with the
    32-bit limb count; the 64-bit struct of the same prime is untouched by the word-length parameter"""
    fp = derive(P, wl=32)
    t = emit.header_text(fp)
    assert "struct P_%s_W32 {" % P in t and "namespace ma32 {" in t and "#define MA_WL 32" in t
    assert "static constexpr int SPLIT = 0;" in t and "CHAIN = false" in t
    assert "spint x[%d]" % fp.nlimbs in t
    assert P in emit.W32_PRIMES and emit.W32_PRIMES == emit.CORE_PRIMES
    t64 = emit.header_text(derive(P))
    assert "struct P_%s {" % P in t64 and "namespace ma {" in t64 and "MA_WL" not in t64
    import os
    assert open(os.path.join(emit.GEN_DIR, "params_%s.h" % P)).read() == t64
    assert open(os.path.join(emit.GEN_DIR, "w32_%s.h" % P)).read() == t
