"""Fused chains (modarith_amd/fuse.py), CPU side: what is emitted, that it cross-compiles for gfx950 and exports its entry
point.  No compute (no GPU here)."""
import ctypes
import os

import pytest

from modarith_amd import _lib
from modarith_amd.fuse import Chain


def _accept(P, name="accept", **kw):
    ch = Chain(P, name, **kw)
    x, y = ch.inputs(2)
    s = ch.modsqr(ch.modmul(ch.modadd(x, y), ch.modsub(x, y)))
    ch.output(ch.modinv(s))
    return ch


def test_source_is_the_call_sequence_on_registers():
    ch = _accept("X25519")
    src = ch.source()
    body = src[src.index("void body("):src.index("template <int EPT, class IO>")]
    calls = [l.strip() for l in body.splitlines() if l.strip().startswith("F::")]
    assert calls == ["F::modadd(v0, v1, v2);", "F::modsub(v0, v1, v3);", "F::modmul(v2, v3, v4);", "F::modsqr(v4, v5);",
                     "F::modinv(v5, nullptr, v6); inv_normalise<F>(v6);"]
    assert "HEAVY = true" in src and src.count("io.load(1, v1);") == src.count("io.load(1,") == 1 and src.count("io.store(0, v6);") == src.count("io.store(0,") == 1
    assert ch.traffic_bytes() == 120 and ch.unfused_traffic_bytes() == 520          # two arrays in, one out; five round trips
    assert ch.symbol == "chain_accept_X25519_batch"


def test_builder_refusals():
    with pytest.raises(ValueError, match="C identifier"):
        Chain("X25519", "9lives")
    with pytest.raises(ValueError, match="neither built in nor generated"):
        Chain("NOSUCH", "c")
    a, b = Chain("X25519", "a"), Chain("X25519", "b")
    x = a.input()
    with pytest.raises(ValueError, match="values of this chain"):
        b.modsqr(x)
    a.modsqr(x)
    with pytest.raises(ValueError, match="before the first operation"):
        a.input()
    with pytest.raises(ValueError, match="at least one input and one output"):
        a.source()
    with pytest.raises(ValueError, match="C int"):
        a.modmli(x, 1 << 40)


def test_chain_cross_compiles_and_exports(tmp_path):
    if not os.path.exists(_lib.LIB_PATH):
        pytest.skip("libmodarith_amd.so not built")
    ch = Chain("NIST256", "twoout")
    x, y = ch.inputs(2)
    t, w = ch.modadd(x, y), ch.modsub(x, y)
    ch.output(ch.modmul(t, w))
    ch.output(ch.modmli(ch.modsqr(t), 121665))
    f = ch.build(plugin_dir=str(tmp_path))
    assert f.built and os.path.exists(f.path) and hasattr(f.lib, "chain_twoout_NIST256_batch")
    assert "HEAVY = false" in ch.source()
    assert not ch.build(plugin_dir=str(tmp_path)).built          # cached by content


def _prod(P, name="prod", **kw):
    ch = Chain(P, name, **kw)
    u, v = ch.inputs(2)
    ch.output(ch.modsqr(ch.modmul(ch.modadd(u, v), ch.modsub(u, v))))
    return ch


@pytest.mark.parametrize("wl", [64, 32])
def test_unit_holds_the_chain_and_includes_the_frame_once(wl):
    """the kernels and entry bodies are csrc/chain.inc's: the unit has one step function, one include of the frame, and no kernel of its own"""
    src = _accept("X25519", wl=wl).source()
    assert src.count('#include "chain.inc"') == 1 and src.count("MA_DEV void chain_step(IO io) {") == 1 and src.count("void body(") == 1
    assert "__global__" not in src and "<<<" not in src and "__syncthreads" not in src
    assert len(src.splitlines()) <= (50 if wl == 64 else 45)
    from modarith_amd import build
    inc = open(os.path.join(build.CSRC, "chain.inc")).read()
    assert inc.count("void k_chain(Args A, size_t nthreads, Ld L)") == 1 and inc.count("void k_chain_aos(Args A, size_t n)") == 1
    assert inc.count("int chain_batch(") == 1 and inc.count("void aos_in(") == 1
    # one entry body for chains with and without byte records, and one check of the tiled stride in it
    assert "chain_bytes_batch" not in inc and inc.count("must be a power of two >= 128") == 1
    by = Chain("X25519", "by", wl=wl)
    v, _ = by.input_bytes()
    by.output_bytes(by.modsqr(v))
    bsrc = by.source()
    assert "chain_bytes_batch" not in bsrc and bsrc.count("{ return chain_batch(in, out, n, ld, stream); }") == 1


class _Arr:
    """stands for an array where only the count of a call's arrays is looked at"""


def test_layout_is_the_one_order_of_a_calls_arrays(tmp_path):
    """Chain.layout() against what FusedChain demands and makes and what prototype() (the line `python -m modarith_amd.fuse` prints)
    says, on a chain with every kind of array -- two of every kind but the element input, so that no two counts are equal by chance --;
    every wrong count is refused with the message it always had"""
    import re
    from modarith_amd.fuse import FusedChain
    ch = Chain("X25519", "kinds")
    a, b, c = ch.inputs(3)
    (r, ok), (q, _) = ch.input_bytes(), ch.input_bytes()
    k, k2 = ch.shared(), ch.shared()
    d, d2 = ch.selector(), ch.selector()
    t = ch.modmul(ch.modadd(a, b), ch.modmul(k, k2))
    u = ch.modadd(ch.modadd(t, r), ch.modadd(q, c))
    for v in (ch.modcmv(d, t, u), ch.modcmv(d2, u, t)):
        ch.output(v)
    for v in (u, t):
        ch.output_bytes(v)
    for p in (ch.land(ok, ch.lnot(ch.modis0(u))), ch.modis0(t)):
        ch.output(p)
    ins, outs = ch.layout()
    assert list(ins.items()) == [("elements", 3), ("bytes", 2), ("shared", 2), ("selectors", 2)]
    assert list(outs.items()) == [("elements", 2), ("bytes", 2), ("ints", 2)]
    assert (ch.nin, len(ch.bins), ch.nshared, ch.nsel, len(ch.outs), len(ch.bouts), len(ch.pouts)) == (3, 2, 2, 2, 2, 2, 2)
    # the printed prototype: the numbers inside the two comments, in order
    proto = ch.prototype()
    cin, cout = re.findall(r"/\* (.*?) \*/", proto)
    assert proto.startswith("int chain_kinds_X25519_batch(const void *const *in /* 3 element batches, then 2 arrays of n records of 32 bytes, then 2 host pointers")
    assert [int(x) for x in re.findall(r"\d+", cin)] == [3, 2, 32, 2, 5, 2, 32] and "then 2 int32 selector arrays" in cin          # (32 bytes, 5 limbs, int32)
    assert cout == "2 element batches, then 2 arrays of n records of 32 bytes, then 2 int32 arrays of n entries"
    plain = Chain("X25519", "plain")
    x, y = plain.inputs(2)
    plain.output(plain.modmul(x, y))
    assert "/* 2 element batches */, void *const *out /* 1 */" in plain.prototype()
    # what a built chain demands of a call and makes for it (nothing is built or loaded here)
    f = FusedChain.__new__(FusedChain)
    f.chain = ch
    limbs = [1, 2, 3, 4, 5]
    good = [_Arr() for _ in range(5)] + [limbs, limbs] + [_Arr(), _Arr()]
    elems, recs, shared, sels = f._split(good, "batches")
    assert (elems, recs, sels) == (good[:3], good[3:5], good[7:]) and [list(s) for s in shared] == [limbs, limbs]
    assert sum(ins.values()) == len(good) == 9
    for bad in (good[:-1], good + [_Arr()], []):
        with pytest.raises(ValueError, match=r"chain kinds takes 3 element batches, 2 arrays of byte records \(uint8 \[n, 32\]\) followed by 2 shared operands "
                                             r"\(5 limbs each, on the host\) and 2 int32 selector arrays"):
            f._split(bad, "batches")
    import torch
    like = torch.empty(0)
    eouts, brecs, ints = f._outs(None, 7, like, lambda: "element batch")
    made = eouts + brecs + ints
    assert len(made) == sum(outs.values()) == 6 and eouts == ["element batch"] * 2
    assert [(t.dtype, tuple(t.shape)) for t in brecs + ints] == [(torch.uint8, (7, 32))] * 2 + [(torch.int32, (7,))] * 2
    assert f._outs(made, 7, like, None) == [eouts, brecs, ints]
    for bad in (made[:-1], made + [made[-1]], []):
        with pytest.raises(ValueError, match="chain kinds has 2 outputs followed by 2 byte-record outputs followed by 2 int32 outputs"):
            f._outs(bad, 7, like, None)
    f.chain = plain
    with pytest.raises(ValueError, match=r"chain plain takes 2 element arrays followed by 0 shared operands \(5 limbs each, on the host\) and 0 int32 selector arrays"):
        f._split([_Arr()], "arrays")
    with pytest.raises(ValueError, match="chain plain has 1 outputs$"):
        f._outs([], 7, like, None)


@pytest.mark.parametrize("wl", [64, 32])
def test_two_chains_differ_only_in_what_depends_on_the_chain(wl):
    """the same name over the same prime, two different chains: every differing line is the header comment, a constant, or inside
    body / chain_step"""
    import difflib
    a, b = _accept("X448", "c", wl=wl).source().splitlines(), _prod("X448", "c", wl=wl).source().splitlines()

    def allowed(lines):
        ok, inside = set(), False
        for k, l in enumerate(lines):
            if l.startswith("template <class F> MA_DEV void body(") or l.startswith("template <int EPT, class IO> MA_DEV void chain_step("):
                inside = True
            if inside or l.startswith(("// GENERATED", "constexpr ", "#define CHAIN_AOS_IMAGES")):
                ok.add(k)
            if l == "}":
                inside = False
        return ok

    oka, okb = allowed(a), allowed(b)
    for tag, i1, i2, j1, j2 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag != "equal":
            assert set(range(i1, i2)) <= oka and set(range(j1, j2)) <= okb, (tag, a[i1:i2], b[j1:j2])
    assert a != b


def test_editing_the_frame_rebuilds_every_chain(tmp_path, monkeypatch):
    """generate.key_of hashes every file under csrc/ (build._stamp): one changed byte of chain.inc is another key.  On a copy of csrc/"""
    import shutil
    from modarith_amd import build, generate
    copy = str(tmp_path / "csrc")
    shutil.copytree(build.CSRC, copy, ignore=shutil.ignore_patterns("*.o"))
    monkeypatch.setattr(build, "CSRC", copy)
    text = _accept("X25519").source()
    k0 = generate.key_of(text)
    assert k0 == generate.key_of(text)
    with open(os.path.join(copy, "chain.inc"), "r+b") as f:
        c = f.read(1)
        f.seek(0)
        f.write(b"/" if c != b"/" else b" ")
    k1 = generate.key_of(text)
    os.remove(os.path.join(copy, "chain.inc"))
    assert len({k0, k1, generate.key_of(text)}) == 3


def test_stub_of_the_element_major_entry_compiles_without_its_kernel(tmp_path):
    """more than 14 limbs: the unit says CHAIN_AOS_IMAGES 0 and csrc/chain.inc then defines the refusing chain_aos and no k_chain_aos.
    The text for a 15-limb field is emitted here; the branch is compiled with that constant over a built-in field (seconds; no 15-limb
    field is built in), and the object holds both entry symbols and the two k_chain widths only"""
    import subprocess
    import sys
    from modarith_amd import build, plugin
    ch = _prod("X25519", "stub")
    src = ch.source()
    assert "#define CHAIN_AOS_IMAGES 2 " in src
    big = _prod("X25519", "stub")
    big.params = type("FifteenLimbs", (), {"nlimbs": 15})()
    assert "#define CHAIN_AOS_IMAGES 0 " in big.source() and big.source().replace("IMAGES 0 ", "IMAGES 2 ") == src
    unit, obj = str(tmp_path / "stub.hip"), str(tmp_path / "stub.o")
    with open(unit, "w") as f:
        f.write(big.source())
    subprocess.run([build.HIPCC] + build.FLAGS + [a for i in plugin.include_dirs(str(tmp_path)) for a in ("-I", i)] + ["-c", unit, "-o", obj], check=True, timeout=600)
    syms = subprocess.run(["nm", obj], capture_output=True, text=True, check=True).stdout
    assert " T chain_stub_X25519_batch" in syms and " T chain_stub_X25519_aos" in syms
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import chain_objects
    import kernel_resources
    assert sorted(chain_objects.short(k["name"]) for k in kernel_resources.kernels_of(obj)) == ["k_chain<1>", "k_chain<2>"]


_RES = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size")


@pytest.mark.parametrize("key", ["bench_prod/X25519", "twoout/NIST256/w32"])
def test_kernels_keep_the_recorded_resources(tmp_path, key):
    """registers, LDS and scratch of the kernels of two chains equal profiles/chain_one_include.json (taken when the frame moved into
    csrc/chain.inc, where they equalled the units that carried their own frame): a change to the frame that moves them shows here"""
    import json
    import sys
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import chain_objects
    import kernel_resources
    want = json.load(open(os.path.join(root, "profiles", "chain_one_include.json")))["code_objects"][key]
    _, prime, name, wl, make, kw = next(c for c in chain_objects.CHAINS if c[0] == key)
    ch = Chain(prime, name, wl=wl)
    make(ch)
    ch.build(plugin_dir=str(tmp_path), **kw)
    obj = str(tmp_path / ("chain_%s_%s%s.o" % (name, prime, "" if wl == 64 else "_w32")))
    got = {chain_objects.short(k["name"]): {x: k[x] for x in _RES} for k in kernel_resources.kernels_of(obj)}
    assert got == {k: {x: v["new"][x] for x in _RES} for k, v in want.items()}


def test_text_front_end():
    """python -m modarith_amd.fuse <prime> <name> "<statements>": the same chain as the builder calls"""
    from modarith_amd.fuse import parse
    a = _accept("X25519").source()
    b = parse("X25519", "accept", "in x, y; t = modadd(x, y); w = modsub(x, y); s = modsqr(modmul(t, w)); out modinv(s)").source()
    assert a == b
    c = parse("X448", "sw", "in g, f; sel d; g2, f2 = modcsw(d, g, f); out modmli(g2, 39081), f2")
    assert (c.nin, c.nsel, len(c.outs)) == (2, 1, 2) and "F::modcsw(s0, v2, v3);" in c.source() and "F::modmli(v2, 39081, v4);" in c.source()
    for bad, msg in (("in x; out nosuch(x)", "unknown operation"), ("in x; out y", "unknown value"), ("in x; x + 1", "expected"),
                     ("in x; a, b = modsqr(x); out a", "does not produce")):
        with pytest.raises(ValueError, match=msg):
            parse("X25519", "bad", bad)
