"""Fused chains with batch-wide operands (Chain.shared()) and field constants (modint / modone / modzer), CPU side: what is emitted,
that chains without them emit the text they always did, what is refused, the byte counts, and that the units cross-compile for gfx950
at both word lengths without scratch.  No compute (no GPU here)."""
import hashlib
import os
import sys

import pytest

from modarith_amd import _lib
from modarith_amd.fuse import Chain, MAX_SHARED, parse

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDADD = "in x, y, t; shared d; out modadd(modmul(modmul(x, y), d), t)"


def _edadd(P, name="edadd", **kw):
    """the product of two coordinates times the curve's d, plus a third (the shape of edwards.c's addition): d is one element for the batch"""
    ch = Chain(P, name, **kw)
    x, y, t = ch.inputs(3)
    d = ch.shared()
    ch.output(ch.modadd(ch.modmul(ch.modmul(x, y), d), t))
    return ch


@pytest.mark.parametrize("wl", [64, 32])
def test_shared_operand_is_an_argument_of_body_and_not_a_load(wl):
    ch = _edadd("X25519", wl=wl)
    src = ch.source()
    lines = src.splitlines()
    assert sum(l.startswith("#define CHAIN_NSHARED 1 ") for l in lines) == 1 and src.count("CHAIN_NSHARED") == 1
    body = next(l for l in lines if l.startswith("template <class F> MA_DEV void body("))
    assert body == ("template <class F> MA_DEV void body(const spint* v0, const spint* v1, const spint* v2, const spint* v3, "
                    "spint* v4, spint* v5, spint* v6) {")
    calls = [l.strip() for l in lines if l.strip().startswith("F::")]
    assert calls == ["F::modmul(v0, v1, v4);", "F::modmul(v4, v3, v5);", "F::modadd(v5, v2, v6);"]
    assert [l.strip() for l in lines if "io.load(" in l] == ["io.load(0, v0);", "io.load(1, v1);", "io.load(2, v2);"] and "v3[" not in src
    assert src.count("    const spint* v3 = io.shared(0);") == 1 and src.count("io.shared(") == 1
    assert "spint v3[EPT][P::N];" not in src and "spint v2[EPT][P::N]; spint v4[EPT][P::N];" in src
    vote = [l for l in lines if "in_split_contract" in l]
    if wl == 64:
        assert vote[0].strip() == "bool ok = in_split_contract<P>(v3);" and len(vote) == 2
        assert "in_split_contract<P>(v0[E]) && in_split_contract<P>(v1[E]) && in_split_contract<P>(v2[E]);" in vote[1] and "v3" not in vote[1]
        assert src.count("body<Field<P, true>>(v0[E], v1[E], v2[E], v3, v4[E], v5[E], v6[E]);") == 1
    else:
        assert not vote and "__all" not in src
        assert src.count("body<Field<P>>(v0[E], v1[E], v2[E], v3, v4[E], v5[E], v6[E]);") == 1
    assert parse("X25519", "edadd", EDADD, wl=wl).source() == src
    assert (ch.nin, ch.nshared, ch.nsel, len(ch.outs)) == (3, 1, 0, 1)


@pytest.mark.parametrize("wl", [64, 32])
def test_constants_are_the_functions_of_the_field(wl):
    ch = Chain("NIST256", "consts", wl=wl)
    x = ch.input()
    ch.output(ch.modadd(ch.modmul(x, ch.modint(5)), ch.modsub(ch.modone(), ch.modzer())))
    src = ch.source()
    calls = [l.strip() for l in src.splitlines() if l.strip().startswith("F::")]
    assert calls == ["F::modint(5, v1);", "F::modmul(v0, v1, v2);", "F::modone(v3);", "F::modzer(v4);", "F::modsub(v3, v4, v5);", "F::modadd(v2, v5, v6);"]
    assert "CHAIN_NSHARED" not in src and "body(const spint* v0, spint* v1," in src
    text = parse("NIST256", "consts", "in x; out modadd(modmul(x, modint(5)), modsub(modone(), modzer()))", wl=wl)
    assert text.source() == src
    assert "F::modint(-7, v1);" in parse("NIST256", "neg", "in x; out modmul(x, modint(-7))", wl=wl).source()
    # a negative int is the word (spint)k, outside the limb contract of the split products: such a chain does not vote for them
    if wl == 64:
        assert "P::SPLIT > 0 && false" in parse("NIST256", "neg", "in x; out modmul(x, modint(-7))").source()
        assert "P::SPLIT > 0 && true" in src


# sha256 of Chain.source() as the commit before shared operands emits it (tests/test_fuse_cpu.py: _accept and _prod): a chain that uses
# none of the new things is the text it was, byte for byte
_RECORDED = {
    ("accept", "X25519", 64): "c70338e007fcb7e01fd6c5537ce8c0e4196993b259f964a95334ac6c53ea13e1",
    ("accept", "X25519", 32): "96bf7cdfe981074cafa5fdefb4ae68499356a97eb736022e8c9ce9f115225bf8",
    ("accept", "X448", 64): "5848bcc5825685f6de3a7e4425a98286c8d0e72ad20d5245c0d59c73f08dbc25",
    ("accept", "X448", 32): "3b424a06790c75b47fceaacdcef25cea5fd120c002b4a8eee56aa486b0d8f580",
    ("prod", "X25519", 64): "c28e97e997474fdc0ac0c160495ec234ed070bad69cf1d7ac6ecd160a8fecf1c",
    ("prod", "X25519", 32): "f6d52d603f82c6789e729b92ec9ab2edf5ad2c2b78c297a380a31f3285db7ea9",
    ("prod", "X448", 64): "32580239b61f39c80f5a360db877787d70e1e13f62009f20dc5f86f0da9dbffb",
    ("prod", "X448", 32): "61aa1ff6ec84b5ecc17b4c85428adc3063c09af957b39dc96804be6121e40b44",
}


@pytest.mark.parametrize("key", sorted(_RECORDED), ids=lambda k: "%s-%s-%d" % k)
def test_text_of_chains_without_shared_operands_is_unchanged(key):
    from tests.test_fuse_cpu import _accept, _prod
    which, P, wl = key
    src = {"accept": _accept, "prod": _prod}[which](P, wl=wl).source()
    assert hashlib.sha256(src.encode()).hexdigest() == _RECORDED[key]


def test_refusals():
    ch = Chain("X25519", "r")
    x = ch.input()
    b = ch.shared()
    with pytest.raises(ValueError, match="shared operand is not a per-element array"):
        ch.output(b)
    ch.modmul(x, b)
    with pytest.raises(ValueError, match="before the first operation"):
        ch.shared()
    with pytest.raises(ValueError, match="before the first operation"):
        parse("X25519", "late", "in x; y = modsqr(x); shared b; out modmul(y, b)")
    many = Chain("X25519", "many")
    many.input()
    for _ in range(MAX_SHARED):
        many.shared()
    assert MAX_SHARED == 8
    with pytest.raises(ValueError, match="at most 8 shared operands"):
        many.shared()
    only = Chain("X25519", "only")
    c = only.shared()
    only.output(only.modadd(only.modcpy(c), only.modone()))
    with pytest.raises(ValueError, match="at least one input and one output"):
        only.source()
    for bad in (1 << 40, -(1 << 31) - 1, 5.0, "5", True):
        with pytest.raises(ValueError, match="C int"):
            ch.modint(bad)
    with pytest.raises(ValueError, match="C int"):
        parse("X25519", "big", "in x; out modmul(x, modint(%d))" % (1 << 40))
    other = Chain("X25519", "other")
    y = other.input()
    with pytest.raises(ValueError, match="values of this chain"):
        other.modmul(y, b)
    with pytest.raises(ValueError, match="values of this chain"):
        other.modadd(y, ch.modone())
    lazy32 = Chain("X25519", "l", wl=32)
    with pytest.raises(ValueError, match="not offered at word length 32"):
        lazy32.modadd_lazy(lazy32.input(), lazy32.shared())
    lazy = Chain("X25519", "l")
    u, s = lazy.input(), lazy.shared()
    w = lazy.modadd_lazy(u, s)                                 # one level: a shared operand is a reduced element like an input
    with pytest.raises(ValueError, match="generic=False result"):
        lazy.modsub_lazy(w, s)


def test_traffic_counts_a_shared_operand_only_call_by_call():
    ch = _edadd("X25519")
    assert ch.traffic_bytes() == 160                           # three arrays in, one out
    assert ch.unfused_traffic_bytes() == 3 * 3 * 40            # three calls of two operands and a result: d is an array there
    four = Chain("X25519", "edadd4")
    x, y, t, d = four.inputs(4)
    four.output(four.modadd(four.modmul(four.modmul(x, y), d), t))
    assert four.traffic_bytes() == 200 and four.unfused_traffic_bytes() == ch.unfused_traffic_bytes()
    assert _edadd("X25519", wl=32).traffic_bytes() == 4 * 4 * 9 and _edadd("X448").traffic_bytes() == 4 * 8 * 8


@pytest.mark.parametrize("wl", [64, 32])
def test_shared_chain_cross_compiles_without_scratch(tmp_path, wl):
    import json
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ch = _edadd("X25519", wl=wl)
    f = ch.build(plugin_dir=str(tmp_path))
    tag = "X25519" if wl == 64 else "X25519_w32"
    assert f.built and hasattr(f.lib, "chain_edadd_%s_batch" % tag)
    assert hasattr(f.lib, "chain_edadd_X25519_aos") == (wl == 64)
    assert json.load(open(str(tmp_path / ("chain_edadd_%s.json" % tag))))["shared"] == 1
    ks = kernel_resources.kernels_of(str(tmp_path / ("chain_edadd_%s.o" % tag)))
    assert len(ks) == (3 if wl == 64 else 1), [k["name"] for k in ks]          # k_chain<1>, k_chain<2>, k_chain_aos | k_chain<1>
    for k in ks:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0, k
    with pytest.raises(ValueError, match="3 element batches followed by 1 shared operands .* and 0 int32 selector arrays"):
        f(1, 2, 3)
