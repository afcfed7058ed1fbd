"""Fused chains with little-endian records, sign bits, the shifts and modfsb -- Chain.input_bytes(little=, sign=), Chain.output_bytes(v,
little=, sign=), modshl / modshr / mod2r / modfsb / flatten, and the library chains written with them --, CPU side: what is emitted
(and that a chain using none of it emits what it did), what is refused, the exact-products rule for modshl, the byte counts, the text
form, and that the units cross-compile for gfx950 without spills.  No compute (no GPU here)."""
import json
import os
import sys

import pytest

from modarith_amd import _lib
from modarith_amd.fuse import (Chain, Pred, Val, bench_chain, decompress_chain, edwards_to_montgomery_chain, oncurve_chain, parse, pubkey_chain,
                               rfc8032_decode_chain, rfc8032_encode_chain)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LMUL = "lebytes a, b; outlebytes modmul(a, b)"
LMULS = "lesbytes a, b; outlesbytes (modmul(a, b), sign(a) ^ sign(b))"


def _lmuls(prime, wl=64, name="lmuls"):
    ch = Chain(prime, name, wl=wl)
    (a, _, sa), (b, _, sb) = ch.input_bytes(little=True, sign=True), ch.input_bytes(little=True, sign=True)
    ch.output_bytes(ch.modmul(a, b), little=True, sign=ch.lxor(sa, sb))
    return ch


# ---------------------------------------------------------------------------------------------------------------- emitted text
@pytest.mark.parametrize("wl", [64, 32])
def test_emitted_text(wl):
    ch = _lmuls("X25519", wl)
    src = ch.source()
    lines = src.splitlines()
    for define in ("#define CHAIN_NBIN 2 ", "#define CHAIN_NBOUT 1 ", "#define CHAIN_BIN_LE 0x3 ", "#define CHAIN_BIN_SIGN 0x3 ", "#define CHAIN_BOUT_LE 0x1 ", "#define CHAIN_BOUT_SIGN 0x1 "):
        assert sum(l.startswith(define) for l in lines) == 1, define
    assert lines.index('#include "chain.inc"') > max(k for k, l in enumerate(lines) if l.startswith("#define CHAIN_B"))
    # ints: flag and sign of a, flag and sign of b, the xor
    k = lines.index("template <class F> MA_DEV void body(spint* v0, spint* v1, spint* v2, spint* v3, int& s0, int& s1, int& s2, int& s3, int& s4) {")
    assert [l.strip() for l in lines[k + 1:lines.index("}", k)]] == ["F::nres(v0, v0);", "F::nres(v1, v1);", "F::modmul(v0, v1, v2);", "s4 = s1 ^ s3;", "F::redc(v2, v3);"]
    io = [l.strip() for l in lines if l.startswith("    io.") or "body<Field<P" in l]
    assert io[:2] == ["io.imp(0, v0, s0, s1);", "io.imp(1, v1, s2, s3);"] and io[-1] == "io.exp(0, v3, s4);" and all("body<" in l for l in io[2:-1]) and len(io) > 3
    assert parse("X25519", "lmuls", LMULS, wl=wl).source() == src
    # byte order alone: the calls of a big-endian chain, and only the LE masks
    le = parse("X25519", "lmul", LMUL, wl=wl).source()
    assert "#define CHAIN_BIN_LE 0x3 " in le and "#define CHAIN_BOUT_LE 0x1 " in le and "_SIGN" not in le
    assert "    io.imp(0, v0, s0);" in le and "    io.imp(1, v1, s1);" in le and "    io.exp(0, v3);" in le
    # per array: the masks name the arrays that differ, each side counted from 0
    mixed = Chain("NIST256", "mixed", wl=wl)
    a, _ = mixed.input_bytes()
    b, _, sb = mixed.input_bytes(sign=True)
    c, _ = mixed.input_bytes(little=True)
    d = mixed.selector()
    mixed.output_bytes(a, sign=d)
    mixed.output_bytes(mixed.modmul(b, c), little=True)
    mixed.output(sb)
    msrc = mixed.source()
    assert "#define CHAIN_BIN_LE 0x4 " in msrc and "#define CHAIN_BIN_SIGN 0x2 " in msrc and "#define CHAIN_BOUT_LE 0x2 " in msrc and "#define CHAIN_BOUT_SIGN 0x1 " in msrc
    # (the selector is s0: the computed ints follow it)
    assert "    io.imp(1, v1, s2, s3);" in msrc and "    io.exp(0, v3, s0);" in msrc and "    io.exp(1, v5);" in msrc and "    io.pred(0, s3);" in msrc


def _old_kinds(wl):
    """one chain of each existing kind, built through the calls that existed before"""
    out = []
    if wl == 64:
        out.append(bench_chain("X25519"))
    plain = Chain("X25519", "plain", wl=wl)
    x, y = plain.inputs(2)
    plain.output(plain.modinv(plain.modmul(x, y)))
    plain.output(plain.modis0(x))
    out.append(plain)
    out.append(oncurve_chain("NIST256", wl)[0])
    out.append(pubkey_chain("NIST256", wl)[0])
    out.append(decompress_chain("ED25519", wl)[0])
    by = Chain("X448", "by", wl=wl)
    a, fa = by.input_bytes()
    s = by.selector()
    e = by.input()
    by.output_bytes(by.modcmv(by.land(s, fa), e, a))
    by.output(by.lnot(fa))
    out.append(by)
    return out


@pytest.mark.parametrize("wl", [64, 32])
def test_chains_that_use_none_of_it_emit_what_they_did(wl):
    """the new keywords at their defaults are the old calls; nothing of the new text appears"""
    by = Chain("X448", "by", wl=wl)
    a, fa = by.input_bytes(little=False, sign=False)
    s = by.selector()
    e = by.input()
    by.output_bytes(by.modcmv(by.land(s, fa), e, a), little=False, sign=None)
    by.output(by.lnot(fa))
    olds = _old_kinds(wl)
    assert by.source() == olds[-1].source()
    for ch in olds:
        src = ch.source()
        for word in ("_LE", "_SIGN", "little", "sign", "modshl", "modshr", "mod2r", "modfsb", "flatten"):
            assert word not in src.replace("modsign", ""), (ch.name, word)
    txt = parse("X448", "by", "bytes a; sel s; in e; outbytes modcmv(s & flag(a), e, a); out not flag(a)", wl=wl)
    assert txt.source() == olds[-1].source()


def test_decode_shares_the_body_of_decompress():
    """the same operations in the same order, plus the `&` with the record's flag"""
    dec, (d,) = rfc8032_decode_chain()
    ref, (d2,) = decompress_chain()
    assert d == d2
    ops, want = [o.op for o in dec.ops], [o.op for o in ref.ops]
    k = want.index("modqr") + 1
    assert ops == want[:k] + ["land"] + want[k:]
    assert dec.layout() == ({"elements": 0, "bytes": 1, "shared": 1, "selectors": 0}, {"elements": 3, "bytes": 0, "ints": 1})
    assert dec.bins[0].little and dec.bins[0].sign >= 0 and dec._long()


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    ch = Chain("X25519", "r")                                    # radix 51
    v, ok, s = ch.input_bytes(little=True, sign=True)
    assert isinstance(v, Val) and isinstance(ok, Pred) and isinstance(s, Pred)
    sh = ch.shared()
    for k in (0, -1, 32, 51, 1.0, True):
        with pytest.raises(ValueError, match="shift count"):
            ch.modshl(v, k)
        with pytest.raises(ValueError, match="shift count"):
            ch.modshr(v, k)
    n256 = Chain("NIST256", "r", wl=32)                          # radix 29 at word length 32: k < 29
    w = n256.input()
    with pytest.raises(ValueError, match="shift count"):
        n256.modshl(w, 29)
    n256.modshr(w, 28)
    with pytest.raises(ValueError, match="mod2r takes"):
        ch.mod2r(-1)
    with pytest.raises(ValueError, match="sign of a byte output is an int of this chain"):
        ch.output_bytes(v, sign=v)
    other = Chain("X25519", "o")
    with pytest.raises(ValueError, match="sign of a byte output is an int of this chain"):
        ch.output_bytes(v, sign=other.input_bytes(sign=True)[2])
    with pytest.raises(ValueError, match="sign of a byte output is an int of this chain"):
        ch.output_bytes(v, sign=other.selector())
    with pytest.raises(ValueError, match="shared operand is not a per-element array"):
        ch.output_bytes(sh, little=True)
    with pytest.raises(ValueError, match="not an element operand"):
        ch.modfsb(s)
    r = ch.modshl(v, 1)
    for late in (lambda: ch.input_bytes(little=True), lambda: ch.input_bytes(sign=True)):
        with pytest.raises(ValueError, match="declare every input before the first operation"):
            late()
    with pytest.raises(ValueError, match="declare every input"):
        parse("X25519", "late", "in x; y = modsqr(x); lesbytes b; out modmul(y, b)")
    with pytest.raises(ValueError, match="declare every input"):                 # (the output has fixed the place of sign(a) among the ints)
        parse("X25519", "late", "sbytes a; outsbytes (a, sign(a)); sel d; out flag(a)")
    with pytest.raises(ValueError, match="sign\\(\\) takes the name of a byte input declared with sbytes or lesbytes"):
        parse("X25519", "f", "lebytes a; outlesbytes (a, sign(a))")
    with pytest.raises(ValueError, match="sign\\(\\) takes the name of a byte input"):
        parse("X25519", "f", "in x; out sign(x)")
    with pytest.raises(ValueError, match="outsbytes takes pairs"):
        parse("X25519", "f", "sbytes a; outsbytes a")
    with pytest.raises(ValueError, match="unknown value"):
        parse("X25519", "f", "sbytes a; outsbytes (b, sign(a))")
    with pytest.raises(ValueError, match="does not produce"):
        parse("X25519", "f", "in a; v, r = modshl(a, 1); out v")
    with pytest.raises(ValueError, match="shift count"):
        parse("X25519", "f", "in a; v, r = modshr(a, 0); out v")
    assert r.chain is ch


# ---------------------------------------------------------------------------------------------------------------- the product policy
def test_modshl_takes_the_exact_products():
    """modshl leaves the limb contract (the top limb grows by k bits): a 64-bit chain with one runs the exact products throughout, the
    vote disabled; the other new operations leave the vote as it is"""
    sh = parse("X25519", "shl", "in a, b; out modmul(modshl(a, 3), b)").source()
    assert "    bool fast = false;" in sh and "    if constexpr (P::SPLIT > 0 && false) {" in sh
    for text in ("in a, b; v, r = modshr(a, 1); out modmul(v, b), r", "in a, b; v, f = modfsb(a); out modmul(v, b), f",
                 "in a, b; v, f = flatten(a); out modmul(v, mod2r(7)), f", "lesbytes a, b; outlesbytes (modmul(a, b), sign(a))"):
        src = parse("X25519", "vote", text).source()
        assert "    bool fast = false;" in src and "    if constexpr (P::SPLIT > 0 && true) {" in src and "fast = __all(ok);" in src, text
    assert "fast" not in parse("X25519", "shl", "in a, b; out modmul(modshl(a, 3), b)", wl=32).source()       # (one policy at word length 32)


def test_shift_lines():
    ch = parse("X25519", "sh", "in D, x; one = modone(); d = modadd(D, one); d, f = modfsb(d); d, r = modshr(d, 1); out modmul(x, d), r")
    src = ch.source()
    assert "    F::modcpy(v3, v4); s0 = (int)F::modfsb(v4);" in src and "    F::modcpy(v4, v5); s1 = F::modshr(1, v5);" in src
    assert "int& s0, int& s1) {" in src and "    io.pred(0, s1);" in src
    k = parse("X25519", "k", "in a; sel c; v, r = modshr(a, 1); w, g = flatten(modshl(v, 2)); out modcmv(r ^ c, w, mod2r(255)), g").source()
    assert "s1 = F::modshr(1, v1);" in k and "F::modcpy(v1, v2); F::modshl(2, v2);" in k and "s2 = (int)F::flatten(v3);" in k and "F::mod2r(255, v4);" in k and "s3 = s1 ^ s0;" in k


# ---------------------------------------------------------------------------------------------------------------- traffic
def test_traffic():
    lm = parse("X25519", "lmul", LMUL)
    assert lm.traffic_bytes() == 96                              # 32 + 32 in, 32 out: what the big-endian chain moves
    assert lm.unfused_traffic_bytes() == 344 + 3 * 64            # the four calls, and a reversal (32 in, 32 out) per record array
    ls = _lmuls("X25519")
    assert ls.traffic_bytes() == 96 and ls.unfused_traffic_bytes() == 344 + 3 * 64 + 3 * 4       # and an int array per sign
    lm32 = parse("X25519", "lmul", LMUL, wl=32)
    assert lm32.traffic_bytes() == 96 and lm32.unfused_traffic_bytes() == 2 * (32 + 36 + 4) + 3 * 36 + (36 + 32) + 3 * 64
    dec, _ = rfc8032_decode_chain()
    ref, _ = decompress_chain()
    assert dec.traffic_bytes() == 32 + 3 * 40 + 4
    # the calls of decompress_chain; modimp, the reversal and the sign array on top
    assert dec.unfused_traffic_bytes() == ref.unfused_traffic_bytes() + (32 + 40 + 4) + 64 + 4
    enc = rfc8032_encode_chain()
    assert enc.traffic_bytes() == 2 * 40 + 32
    assert enc.unfused_traffic_bytes() == (40 + 4) + (40 + 32) + 64 + 4          # modsign, modexp, the reversal, the sign
    e2m = edwards_to_montgomery_chain()
    assert e2m.traffic_bytes() == 32 + 32 + 4
    # modimp + reversal + sign; modone, modadd, modsub, modinv, modmul; modexp + reversal
    assert e2m.unfused_traffic_bytes() == (76 + 64 + 4) + 40 + 120 + 120 + 80 + 120 + (72 + 64)
    sh = parse("X25519", "sh", "in a; v, r = modshr(modshl(a, 1), 1); w, f = modfsb(v); out modadd(w, mod2r(3)), r")
    assert sh.unfused_traffic_bytes() == 80 + (80 + 4) + (80 + 4) + 40 + 120 and sh.traffic_bytes() == 80 + 4


# ---------------------------------------------------------------------------------------------------------------- the text front end
def _same(a: Chain, b: Chain):
    assert a.ops == b.ops and a.layout() == b.layout() and a.bins == b.bins and a.bouts == b.bouts and a.outs == b.outs and a.pouts == b.pouts
    assert a.source() == b.source()


@pytest.mark.parametrize("wl", [64, 32])
def test_text_front_end(wl):
    py = Chain("NIST256", "t", wl=wl)
    a, fa = py.input_bytes(little=True)
    b, fb, sb = py.input_bytes(sign=True)
    c, fc, sc = py.input_bytes(little=True, sign=True)
    m = py.modmul(py.modmul(a, b), c)
    py.output_bytes(m, little=True)
    py.output_bytes(m, sign=sb)
    py.output_bytes(py.modsqr(m), little=True, sign=py.lxor(sb, sc))
    py.output(py.land(py.land(fa, fb), fc))
    _same(py, parse("NIST256", "t", "lebytes a; sbytes b; lesbytes c; m = modmul(modmul(a, b), c); outlebytes m; outsbytes (m, sign(b)); "
                                    "outlesbytes (modsqr(m), sign(b) ^ sign(c)); out flag(a) & flag(b) & flag(c)", wl=wl))
    py = Chain("NIST256", "t", wl=wl)
    a = py.input()
    v, r = py.modshr(a, 1)
    w, f = py.modfsb(py.modshl(v, 2))
    u, g = py.flatten(py.modadd(w, py.mod2r(200)))
    py.output(py.modcmv(r, u, a))
    py.output(f)
    py.output(g)
    _same(py, parse("NIST256", "t", "in a; v, r = modshr(a, 1); w, f = modfsb(modshl(v, 2)); u, g = flatten(modadd(w, mod2r(200))); out modcmv(r, u, a), f, g", wl=wl))
    _same(_lmuls("X25519", wl), parse("X25519", "lmuls", LMULS, wl=wl))


# ---------------------------------------------------------------------------------------------------------------- cross-compilation
def _kernels(obj, heavy=False):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels_of(obj)
    for k in ks:
        assert k["vgpr_spill_count"] == 0 and k["group_segment_fixed_size"] <= 65536, k
        if not heavy:                                            # a streaming chain: nothing in scratch
            assert k["private_segment_fixed_size"] == 0, k
    return ks


def _both_ways(ks, widths):
    names = " ".join(k["name"] for k in ks)
    assert len(ks) == 2 * len(widths), names
    for w in widths:
        assert "k_chain_direct<%d>" % w in names and "k_chain_staged<%d>" % w in names, names
    staged = [k for k in ks if "k_chain_staged" in k["name"]]
    assert all(k["group_segment_fixed_size"] > 0 for k in staged) and all(k["group_segment_fixed_size"] == 0 for k in ks if k not in staged)


@pytest.mark.parametrize("prime,wl,ept", [("X25519", 64, None), ("X25519", 32, None), ("X448", 32, 4), ("NIST521", 64, None)])
def test_units_cross_compile(tmp_path, prime, wl, ept):
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    tag = prime + ("" if wl == 64 else "_w32")
    f = _lmuls(prime, wl).build(plugin_dir=str(tmp_path), ept=ept)
    assert f.built and hasattr(f.lib, "chain_lmuls_%s_batch" % tag)
    rec = json.load(open(str(tmp_path / ("chain_lmuls_%s.json" % tag))))
    assert rec["bytes_in"] == 2 and rec["bytes_out"] == 1 and rec["inputs"] == 0 and rec["outputs"] == 0
    _both_ways(_kernels(str(tmp_path / ("chain_lmuls_%s.o" % tag))), (1, 2) if wl == 64 else tuple(w for w in (1, 2, 4) if w <= (ept or 1)))
    with pytest.raises(ValueError, match="no element-major entry"):
        f.aos(1, 2)


@pytest.mark.parametrize("wl", [64, 32])
@pytest.mark.parametrize("which", ["decode", "encode", "to_montgomery"])
def test_library_chains_cross_compile(tmp_path, which, wl):
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    made = {"decode": rfc8032_decode_chain, "encode": rfc8032_encode_chain, "to_montgomery": edwards_to_montgomery_chain}[which]("ED25519", wl)
    ch = made[0] if isinstance(made, tuple) else made
    heavy = which != "encode"
    assert ch._long() == heavy and ch.default_ept() == (1 if heavy or wl == 32 else 2)
    f = ch.build(plugin_dir=str(tmp_path))
    assert f.built
    ks = _kernels(str(tmp_path / ("chain_%s_X25519%s.o" % (ch.name, "" if wl == 64 else "_w32"))), heavy)
    _both_ways(ks, (1, 2) if wl == 64 else (1,))
