"""Fused chains with ints computed inside them -- the predicates modis0 / modis1 / modsign / modcmp / modqr, the 0/1 expressions lnot /
land / lor / lxor, computed selectors of modcmv / modcsw, the optional progenitor of modsqrt / modinv / modqr, int32 outputs --, CPU
side: what is emitted, that the text form gives the same unit, what is refused, the byte counts, and that the units cross-compile for
gfx950 at both word lengths.  No compute (no GPU here)."""
import json
import os
import re
import sys

import pytest

from modarith_amd import _lib
from modarith_amd.fuse import Chain, Pred, decompress_chain, oncurve_chain, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ONCURVE = "in x, y; shared b; out modcmp(modsqr(y), modadd(modsub(modmul(modsqr(x), x), modmli(x, 3)), b))"
DECOMPRESS = ("in y; shared d; sel s; one = modone(); Y = modsqr(y); U = modsub(one, Y); V = modsub(modneg(one), modmul(Y, d)); O = modsqr(U); "
              "W = modmul(modmul(U, O), V); H = modpro(W); ok = modqr(W, H); R = modsqrt(W, H); X = modmul(modmul(modinv(W, H), R), O); "
              "X2 = modcmv(modsign(X) ^ s, modneg(X), X); bad = not ok; out modcmv(bad, modzer(), X2), modcmv(bad, one, y), modcpy(one), ok")
SELECT = "in u, v; sel s; d = (modsign(u) ^ s) & (not modis0(v)); w = modcmv(d, modneg(u), u); g2, f2 = modcsw(modcmp(u, v), u, v); out w, g2, f2, d"


def _body(src):
    """the lines of body<F> of a unit"""
    lines = src.splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith("template <class F> MA_DEV void body("))
    return lines[k + 1:lines.index("}", k)]


def _no_decision_in(src):
    """selection stays by lane predication: no branch, conditional expression or loop in the chain's own text"""
    for l in _body(src):
        assert not re.search(r"\b(if|for|while|do|switch|goto)\b|\?", l), l


@pytest.mark.parametrize("wl", [64, 32])
def test_predicate_only_chain(wl):
    ch, (b,) = oncurve_chain("NIST256", wl)
    src = ch.source()
    body = [l.strip() for l in _body(src)]
    assert body == ["F::modsqr(v1, v3);", "F::modsqr(v0, v4);", "F::modmul(v4, v0, v5);", "F::modmli(v0, 3, v6);", "F::modsub(v5, v6, v7);",
                    "F::modadd(v7, v2, v8);", "s0 = F::modcmp(v3, v8);"]
    _no_decision_in(src)
    assert "opaque" not in src                                   # (no value is read by two predicates)
    lines = src.splitlines()
    assert "constexpr int NIN = 2, NOUT = 0, NSEL = 0;" in lines and "constexpr bool HEAVY = false;" in src
    assert sum(l.startswith("#define CHAIN_NPRED 1 ") for l in lines) == 1 and src.count("CHAIN_NPRED") == 1
    assert "int& s0) {" in src and "    int s0[EPT];" in lines and "    io.pred(0, s0);" in lines and "io.store(" not in src and "io.sel(" not in src
    assert src.count("#include \"chain.inc\"") == 1
    assert parse("NIST256", "oncurve", ONCURVE, wl=wl).source() == src
    assert (ch.nin, ch.nshared, ch.nsel, len(ch.outs), len(ch.pouts)) == (2, 1, 0, 0, 1)
    assert len(b) == ch.params.nlimbs
    N, w = ch.params.nlimbs, wl // 8
    assert ch.traffic_bytes() == 2 * N * w + 4
    # modsqr, modmli, modsqr: 2 arrays each; modmul, modsub, modadd: 3; modcmp: two arrays in and 4 bytes out
    assert ch.unfused_traffic_bytes() == (3 * 2 + 3 * 3 + 2) * N * w + 4


@pytest.mark.parametrize("wl", [64, 32])
def test_decompression_chain(wl):
    ch, (d,) = decompress_chain("ED25519", wl)
    src = ch.source()
    _no_decision_in(src)
    body = [l.strip() for l in _body(src)]
    preds = [l for l in body if re.match(r"s\d+ = F::", l)]
    assert preds == ["s1 = F::modqr(v11, v10);", "s2 = F::modsign(v15);"]               # one F:: line per predicate; the progenitor v11 is passed
    assert [l for l in body if re.match(r"s\d+ = ", l) and "F::" not in l] == ["s3 = s2 ^ s0;", "s4 = 1 - s1;"]
    assert body.count("F::modpro(v10, v11);") == 1 and sum("modpro" in l for l in body) == 1
    assert "F::modsqrt(v10, v11, v12);" in body and "F::modinv(v10, v11, v13); inv_normalise<F>(v13);" in body and "nullptr" not in src
    assert "F::modcpy(v15, v17); F::modcmv(s3, v16, v17);" in body                      # a computed selector is still the first argument of F::modcmv
    assert sum("F::modcmv(s4, " in l for l in body) == 2
    assert "constexpr bool HEAVY = true;" in src and "constexpr int NIN = 1, NOUT = 3, NSEL = 1;" in src
    assert "#define CHAIN_NPRED 1 " in src and "#define CHAIN_NSHARED 1 " in src
    assert "int s0, int& s1, int& s2, int& s3, int& s4) {" in src
    lines = src.splitlines()
    assert "    int s0[EPT]; io.sel(0, s0);" in lines and all("    int s%d[EPT];" % k in lines for k in (1, 2, 3, 4))
    assert "    io.pred(0, s1);" in lines and src.count("io.pred(") == 1 and src.count("io.store(") == 3
    assert parse("X25519", "decompress", DECOMPRESS, wl=wl).source() == src
    N, w = ch.params.nlimbs, wl // 8
    assert len(d) == N
    assert ch.traffic_bytes() == 4 * N * w + 4 + 4                                      # y in, x y z out, the selector in, ok out


@pytest.mark.parametrize("wl", [64, 32])
def test_computed_selectors_and_int_expressions(wl):
    ch = parse("X448", "select", SELECT, wl=wl)
    src = ch.source()
    _no_decision_in(src)
    body = [l.strip() for l in _body(src)]
    assert body == ["s1 = F::modsign(v0);", "s2 = s1 ^ s0;", "s3 = F::modis0(v1);", "s4 = 1 - s3;", "s5 = s2 & s4;", "F::modneg(v0, v2);",
                    "F::modcpy(v0, v3); F::modcmv(s5, v2, v3);",
                    "spint t6_0[P::N]; opaque(v0, t6_0); spint t6_1[P::N]; opaque(v1, t6_1); s6 = F::modcmp(t6_0, t6_1);",
                    "F::modcpy(v0, v4); F::modcpy(v1, v5); F::modcsw(s6, v4, v5);"]
    # (a value that a second predicate reads goes through a copy the compiler cannot see through: the two redc of it would otherwise share
    # their products and hold them in registers in between; one F:: call per predicate all the same)
    assert src.count("MA_DEV void opaque(") == 1 and sum(len(re.findall(r"F::mod(sign|is0|is1|cmp|qr)\(", l)) for l in body) == 3
    assert "HEAVY = false" in src and "    io.pred(0, s5);" in src.splitlines()
    py = Chain("X448", "select", wl=wl)
    u, v = py.inputs(2)
    s = py.selector()
    d = py.land(py.lxor(py.modsign(u), s), py.lnot(py.modis0(v)))
    assert isinstance(d, Pred)
    w = py.modcmv(d, py.modneg(u), u)
    g2, f2 = py.modcsw(py.modcmp(u, v), u, v)
    for o in (w, g2, f2, d):
        py.output(o)
    assert py.source() == src
    N, wb = ch.params.nlimbs, wl // 8
    assert ch.traffic_bytes() == 5 * N * wb + 4 + 4
    # modsign, modis0: one array in and 4 out; modcmp: two in and 4 out; modneg: 2 arrays; modcmv: 3 arrays and its selector; modcsw: 4 and its selector
    assert ch.unfused_traffic_bytes() == (1 + 1 + 2) * N * wb + 3 * 4 + (2 + 3 + 4) * N * wb + 2 * 4
    other = parse("X448", "ors", "in a; sel s; out modcmv(s | modis1(a), modhaf(a), a), modis1(a) | s", wl=wl).source()
    assert "s2 = s0 | s1;" in other and "s4 = s3 | s0;" in other


def test_chains_without_ints_do_not_name_them():
    ch = Chain("X25519", "plain")
    x = ch.input()
    ch.output(ch.modsqrt(ch.modinv(x)))
    src = ch.source()
    assert "CHAIN_NPRED" not in src and "io.pred" not in src and "int&" not in src and "opaque" not in src
    assert "F::modinv(v0, nullptr, v1); inv_normalise<F>(v1);" in src and "F::modsqrt(v1, nullptr, v2);" in src
    qr = Chain("X25519", "qr")
    qr.output(qr.modqr(qr.input()))
    assert "s0 = F::modqr(nullptr, v0);" in qr.source() and "HEAVY = true" in qr.source()
    shared_h = parse("X25519", "sh", "in x; shared h; out modinv(x, h), modqr(x, h)").source()          # a shared value is a legal progenitor
    assert "F::modinv(v0, v1, v2);" in shared_h and "s0 = F::modqr(v1, v0);" in shared_h


def test_refusals():
    ch = Chain("X25519", "r")
    x, y = ch.inputs(2)
    s = ch.selector()
    p = ch.modis0(x)
    other = Chain("X25519", "o")
    ox = other.input()
    os_ = other.selector()
    op = other.modis0(ox)
    for f in (lambda: ch.lnot(x), lambda: ch.land(p, x), lambda: ch.lor(y, s), lambda: ch.lxor(x, y), lambda: ch.lnot(1)):
        with pytest.raises(ValueError, match="int expressions take predicates and selectors"):
            f()                                                  # an int operation on an element value
    for f in (lambda: ch.modmul(p, x), lambda: ch.modsqr(p), lambda: ch.modis0(p), lambda: ch.modcmp(x, s), lambda: ch.modcmv(s, p, x),
              lambda: ch.modinv(x, p), lambda: ch.modqr(p), lambda: ch.modcsw(p, x, s)):
        with pytest.raises(ValueError, match="not an element operand"):
            f()                                                  # an element operation on an int
    for f in (lambda: ch.modis0(ox), lambda: ch.modcmp(x, ox), lambda: ch.modqr(x, ox), lambda: ch.modsqrt(x, ox), lambda: ch.output(op)):
        with pytest.raises(ValueError, match="values of this chain"):
            f()
    for f in (lambda: ch.lnot(op), lambda: ch.land(p, os_), lambda: ch.modcmv(op, x, y), lambda: ch.modcsw(os_, x, y)):
        with pytest.raises(ValueError, match="this chain"):
            f()
    for f in (lambda: ch.modcmv(x, x, y), lambda: ch.modcmv(1, x, y), lambda: ch.modcsw(y, x, y)):
        with pytest.raises(ValueError, match="selector must come from"):
            f()                                                  # a selector that is not an int of the chain
    with pytest.raises(ValueError, match="caller's own array"):
        ch.output(s)
    none = Chain("X25519", "none")
    none.modis0(none.input())
    with pytest.raises(ValueError, match="at least one input and one output"):
        none.source()
    only = Chain("X25519", "only")
    only.output(only.modis0(only.shared()))
    with pytest.raises(ValueError, match="at least one input and one output"):
        only.source()                                            # int outputs alone are a chain, but not without an element input
    for bad, msg in (("in x; out not x", "int expressions"), ("in x; out modsqr(modis0(x))", "not an element operand"),
                     ("in x; out modis0(x) + modis1(x)", "cannot parse"), ("in x; sel s; out s", "caller's own array")):
        with pytest.raises(ValueError, match=msg):
            parse("X25519", "bad", bad)


def test_progenitor_counts_as_an_operand_array_call_by_call():
    a = parse("X25519", "a", "in x; out modinv(x)")
    b = parse("X25519", "b", "in x; h = modpro(x); out modinv(x, h), modqr(x, h), modsqrt(x, h)")
    assert a.unfused_traffic_bytes() == 2 * 40 and a.traffic_bytes() == 80
    assert b.unfused_traffic_bytes() == 2 * 40 + 3 * 40 + (2 * 40 + 4) + 3 * 40 and b.traffic_bytes() == 3 * 40 + 4


@pytest.mark.parametrize("wl", [64, 32])
def test_units_cross_compile(tmp_path, wl):
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    sfx = "" if wl == 64 else "_w32"
    ch, _ = oncurve_chain("NIST256", wl)
    f = ch.build(plugin_dir=str(tmp_path))
    assert f.built and hasattr(f.lib, "chain_oncurve_NIST256%s_batch" % sfx) and hasattr(f.lib, "chain_oncurve_NIST256_aos") == (wl == 64)
    rec = json.load(open(str(tmp_path / ("chain_oncurve_NIST256%s.json" % sfx))))
    assert rec["preds"] == 1 and rec["outputs"] == 0 and rec["ops"][-1] == "modcmp"
    ks = kernel_resources.kernels_of(str(tmp_path / ("chain_oncurve_NIST256%s.o" % sfx)))
    assert len(ks) == (3 if wl == 64 else 1), [k["name"] for k in ks]
    for k in ks:                                                 # a streaming chain: nothing in scratch
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    with pytest.raises(ValueError, match="2 element batches followed by 1 shared operands"):
        f(1, 2)
    dc, _ = decompress_chain("ED25519", wl)
    g = dc.build(plugin_dir=str(tmp_path))
    assert g.built and hasattr(g.lib, "chain_decompress_X25519%s_batch" % sfx)
    assert json.load(open(str(tmp_path / ("chain_decompress_X25519%s.json" % sfx))))["preds"] == 1
    sel = parse("X448", "select", SELECT, wl=wl).build(plugin_dir=str(tmp_path))
    assert sel.built and not parse("X448", "select", SELECT, wl=wl).build(plugin_dir=str(tmp_path)).built
    # four predicates, two of them on values another has read, at two elements per lane: inside the register file, nothing in scratch
    # (the opaque copies and the build without the SLP vectoriser: 472 registers and 8 spilled ones for this kernel without them)
    ks = kernel_resources.kernels_of(str(tmp_path / ("chain_select_X448%s.o" % sfx)))
    assert len(ks) == (3 if wl == 64 else 1)
    for k in ks:
        assert k["vgpr_count"] <= 256 and k["agpr_count"] == 0 and k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, k
