"""Fused chains that speak bytes -- Chain.input_bytes() / Chain.output_bytes(): modimp at the head and modexp at the tail of the chain,
inside the kernel --, CPU side: what is refused, what is emitted (and that a chain without byte records does not name any of it), that
the text form gives the same unit, the byte counts, and that the units cross-compile for gfx950 without scratch and inside 64 KB of
LDS.  No compute (no GPU here)."""
import json
import os
import sys

import pytest

from modarith_amd import _lib
from modarith_amd.fuse import Chain, Pred, Val, parse, pubkey_chain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BMUL = "bytes a, b; outbytes modmul(a, b)"
PUBKEY = "bytes x, y; shared b; on = modcmp(modsqr(y), modadd(modsub(modmul(modsqr(x), x), modmli(x, 3)), b)); out flag(x) & flag(y) & on"


def _bmul(prime, wl=64, name="bmul"):
    ch = Chain(prime, name, wl=wl)
    (a, _), (b, _) = ch.input_bytes(), ch.input_bytes()
    ch.output_bytes(ch.modmul(a, b))
    return ch


def test_refusals():
    ch = Chain("X25519", "r")
    v, ok = ch.input_bytes()
    assert isinstance(v, Val) and isinstance(ok, Pred)
    s = ch.shared()
    ch.modsqr(v)
    with pytest.raises(ValueError, match="declare every input before the first operation"):
        ch.input_bytes()
    with pytest.raises(ValueError, match="shared operand is not a per-element array"):
        ch.output_bytes(s)
    with pytest.raises(ValueError, match="not an element operand"):
        ch.output_bytes(ok)
    with pytest.raises(ValueError, match="values of this chain"):
        ch.output_bytes(Chain("X25519", "o").input())
    with pytest.raises(ValueError, match="at least one input and one output"):
        ch.source()                                              # nothing is output yet
    with pytest.raises(ValueError, match="declare every input"):
        parse("X25519", "late", "in x; y = modsqr(x); bytes b; out modmul(y, b)")
    with pytest.raises(ValueError, match="flag\\(\\) takes the name of a byte input"):
        parse("X25519", "f", "in x; out flag(x)")
    # (FusedChain.aos of a byte chain: test_units_cross_compile, on a built one)


@pytest.mark.parametrize("wl", [64, 32])
def test_emitted_text(wl):
    ch = _bmul("X25519", wl)
    src = ch.source()
    lines = src.splitlines()
    assert sum(l.startswith("#define CHAIN_NBIN 2 ") for l in lines) == 1 and sum(l.startswith("#define CHAIN_NBOUT 1 ") for l in lines) == 1
    assert "constexpr int NIN = 0, NOUT = 0, NSEL = 0;" in lines and "CHAIN_AOS_IMAGES" not in src
    k = lines.index("template <class F> MA_DEV void body(spint* v0, spint* v1, spint* v2, spint* v3, int& s0, int& s1) {")
    assert [l.strip() for l in lines[k + 1:lines.index("}", k)]] == ["F::nres(v0, v0);", "F::nres(v1, v1);", "F::modmul(v0, v1, v2);", "F::redc(v2, v3);"]
    assert "    io.imp(0, v0, s0);" in lines and "    io.imp(1, v1, s1);" in lines and "    io.exp(0, v3);" in lines
    assert "io.load(" not in src and "io.store(" not in src and "io.pred(" not in src
    if wl == 64:                                                 # the imported values vote with the wave
        assert "ok = ok && in_split_contract<P>(v0[E]) && in_split_contract<P>(v1[E]);" in src
    assert parse("X25519", "bmul", BMUL, wl=wl).source() == src
    # an input of only one kind leaves the other define out; flags are ints like any other
    imp = parse("NIST256", "imp", "bytes a; out a, flag(a)", wl=wl)
    isrc = imp.source()
    assert "#define CHAIN_NBIN 1 " in isrc and "CHAIN_NBOUT" not in isrc and "#define CHAIN_NPRED 1 " in isrc
    assert "    io.store(0, v0);" in isrc and "    io.pred(0, s0);" in isrc
    exp = parse("NIST256", "exp", "in a; outbytes modcpy(a)", wl=wl)
    esrc = exp.source()
    assert "#define CHAIN_NBOUT 1 " in esrc and "CHAIN_NBIN" not in esrc and "    io.exp(0, v2);" in esrc and "F::redc(v1, v2);" in esrc
    # the flag's place among the ints follows the selectors, wherever the selector is declared
    mixed = parse("X25519", "mixed", "bytes a; sel s; in e; outbytes modcmv(s & flag(a), e, a); out not flag(a)", wl=wl)
    msrc = mixed.source()
    assert "    int s0[EPT]; io.sel(0, s0);" in msrc and "    io.imp(0, v0, s1);" in msrc and "s2 = s0 & s1;" in msrc and "s3 = 1 - s1;" in msrc
    assert "void body(spint* v0, const spint* v1, " in msrc      # the imported value is written by its nres, the element input only read
    py = Chain("X25519", "mixed", wl=wl)
    a, fa = py.input_bytes()
    s = py.selector()
    e = py.input()
    py.output_bytes(py.modcmv(py.land(s, fa), e, a))
    py.output(py.lnot(fa))
    assert py.source() == msrc


@pytest.mark.parametrize("wl", [64, 32])
def test_chains_without_byte_records_do_not_name_them(wl):
    ch = Chain("X25519", "plain", wl=wl)
    x, y = ch.inputs(2)
    ch.output(ch.modmul(x, y))
    ch.output(ch.modis0(x))
    src = ch.source()
    for word in ("CHAIN_NBIN", "CHAIN_NBOUT", "io.imp", "io.exp", "byte-record", "CHAIN_BYTES"):
        assert word not in src, word


def test_traffic():
    ch = _bmul("X25519")
    assert ch.traffic_bytes() == 96                              # 32 + 32 in, 32 out
    assert ch.unfused_traffic_bytes() == 344                     # 2 x (32 + 40 + 4) modimp, 120 modmul, 72 modexp
    ch32 = _bmul("X25519", 32)
    assert ch32.traffic_bytes() == 96 and ch32.unfused_traffic_bytes() == 2 * (32 + 36 + 4) + 3 * 36 + (36 + 32)
    pk, (b,) = pubkey_chain("NIST256")
    assert pk.traffic_bytes() == 64 + 4 and len(b) == 5
    assert (pk.nin, len(pk.bins), pk.nshared, len(pk.outs), len(pk.bouts), len(pk.pouts)) == (0, 2, 1, 0, 0, 1)
    assert parse("NIST256", "pubkey", PUBKEY).source() == pk.source()
    for wl in (64, 32):
        assert parse("NIST256", "pubkey", PUBKEY, wl=wl).source() == pubkey_chain("NIST256", wl)[0].source()


def _resources(obj):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = kernel_resources.kernels_of(obj)
    for k in ks:                                                 # a streaming chain: nothing in scratch, the images inside 64 KB of LDS
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["group_segment_fixed_size"] <= 65536, k
    return ks


@pytest.mark.parametrize("prime,wl,ept", [("X448", 64, None), ("X448", 32, 4), ("NIST521", 64, None), ("X25519", 32, None)])
def test_units_cross_compile(tmp_path, prime, wl, ept):
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    tag = prime + ("" if wl == 64 else "_w32")
    f = _bmul(prime, wl).build(plugin_dir=str(tmp_path), ept=ept)
    assert f.built and hasattr(f.lib, "chain_bmul_%s_batch" % tag) and hasattr(f.lib, "chain_bmul_%s_aos" % prime) == (wl == 64)
    rec = json.load(open(str(tmp_path / ("chain_bmul_%s.json" % tag))))
    assert rec["bytes_in"] == 2 and rec["bytes_out"] == 1 and rec["inputs"] == 0 and rec["outputs"] == 0
    ks = _resources(str(tmp_path / ("chain_bmul_%s.o" % tag)))
    names = " ".join(k["name"] for k in ks)
    # both ways to the bytes at every built width: at 64 bits one and two elements per lane, at 32 bits up to the width asked for
    widths = (1, 2) if wl == 64 else tuple(w for w in (1, 2, 4) if w <= (ept or 1))
    assert len(ks) == 2 * len(widths), names
    for w in widths:
        assert "k_chain_direct<%d>" % w in names and "k_chain_staged<%d>" % w in names, names
    staged = [k for k in ks if "k_chain_staged" in k["name"]]
    assert all(k["group_segment_fixed_size"] > 0 for k in staged) and all(k["group_segment_fixed_size"] == 0 for k in ks if k not in staged)
    if prime == "X448" and wl == 32:                             # 256 lanes x 4 records at a pitch of 56 bytes: one image, the two inputs in turn
        assert max(k["group_segment_fixed_size"] for k in staged) == 256 * 4 * 56
    with pytest.raises(ValueError, match="no element-major entry"):
        f.aos(1, 2)
    with pytest.raises(ValueError, match="0 element batches, 2 arrays of byte records"):
        f(1)


@pytest.mark.parametrize("wl", [64, 32])
def test_pubkey_chain_cross_compiles(tmp_path, wl):
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    ch, _ = pubkey_chain("NIST256", wl)
    f = ch.build(plugin_dir=str(tmp_path))
    assert f.built and not pubkey_chain("NIST256", wl)[0].build(plugin_dir=str(tmp_path)).built
    sfx = "" if wl == 64 else "_w32"
    assert json.load(open(str(tmp_path / ("chain_pubkey_NIST256%s.json" % sfx))))["bytes_in"] == 2
    _resources(str(tmp_path / ("chain_pubkey_NIST256%s.o" % sfx)))
