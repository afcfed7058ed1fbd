"""The shared inversion and the fused chains of the 32-bit word form, CPU side: what fuse.py emits at wl=32, that it cross-compiles
for gfx950 inside the register file, that the built library holds ma32::k_inv_simul without spills, and that the in-contract predicate
of the shared inversion (csrc/kernels.h inv_in_contract, restated in modarith_amd/params.py) admits what the field functions return
-- so that the shared path is the path a real batch takes -- and is safe at the edge of what it admits (host build of csrc/field.h)."""
import os
import random
import sys

import pytest

from modarith_amd import _lib
from modarith_amd.fuse import Chain, W32_EPT_DEFAULT, parse
from modarith_amd.params import derive, w32_inv_in_contract
from tests import w32_inputs as wi
from tests.test_w32_host import host  # noqa: F401  (fixture: csrc/field.h at MA_WL = 32 compiled for the CPU)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402


def _accept(P, name="accept", **kw):
    ch = Chain(P, name, **kw)
    x, y = ch.inputs(2)
    s = ch.modsqr(ch.modmul(ch.modadd(x, y), ch.modsub(x, y)))
    ch.output(ch.modinv(s))
    return ch


def test_w32_source_is_the_call_sequence_on_registers():
    ch = _accept("X25519", wl=32)
    src = ch.source()
    body = src[src.index("void body("):src.index("template <int EPT, class IO>")]
    calls = [l.strip() for l in body.splitlines() if l.strip().startswith("F::")]
    assert calls == ["F::modadd(v0, v1, v2);", "F::modsub(v0, v1, v3);", "F::modmul(v2, v3, v4);", "F::modsqr(v4, v5);",
                     "F::modinv(v5, nullptr, v6); inv_normalise<F>(v6);"]
    assert "using namespace ma32;" in src and '#include "kernels32.h"' in src and '#include "w32_X25519.h"' in src
    assert "using P = ma32::P_X25519_W32;" in src and "body<Field<P>>(" in src and "__all" not in src       # one policy, no vote
    assert "HEAVY = true" in src and src.count("io.load(1, v1);") == src.count("io.load(1,") == 1 and src.count("io.store(0, v6);") == src.count("io.store(0,") == 1
    assert ch.symbol == "chain_accept_X25519_w32_batch" and ("int %s(" % ch.symbol) in src and "_aos" not in src
    assert ch.traffic_bytes() == 108 and ch.unfused_traffic_bytes() == 468            # 4-byte limbs: two arrays in, one out; five round trips
    assert ch.lib_path().endswith("libmodarith_amd_chain_accept_X25519_w32.so")


def test_w32_refusals_and_the_untouched_64_bit_text():
    with pytest.raises(ValueError, match="32-bit word form is built for"):
        Chain("NIST521", "c", wl=32)
    with pytest.raises(ValueError, match="word length must be 64 or 32"):
        Chain("X25519", "c", wl=16)
    ch = Chain("X25519", "c", wl=32)
    x, y = ch.inputs(2)
    for op, args in (("modadd_lazy", (x, y)), ("modsub_lazy", (x, y)), ("modneg_lazy", (x,))):
        with pytest.raises(ValueError, match="not offered at word length 32"):
            getattr(ch, op)(*args)
    with pytest.raises(ValueError, match="modarith_amd_w32_aos_to_soa"):
        ch.aos_symbol
    for P in ("X25519", "NIST256", "X448", "NIST521"):
        assert _accept(P).source() == _accept(P, wl=64).source()
        assert _accept(P).symbol == "chain_accept_%s_batch" % P and _accept(P).traffic_bytes() == 3 * 8 * derive(P).nlimbs


def test_w32_text_front_end(capsys):
    from modarith_amd.fuse import main
    text = "in x, y; t = modadd(x, y); w = modsub(x, y); s = modsqr(modmul(t, w)); out modinv(s)"
    assert parse("X25519", "accept", text, wl=32).source() == _accept("X25519", wl=32).source()
    assert parse("X25519", "accept", text).source() == _accept("X25519").source()
    assert main(["32", "X25519", "accept", text, "--source"]) == 0
    assert capsys.readouterr().out.strip() == _accept("X25519", wl=32).source().strip()
    assert main(["X25519", "accept", text, "--source"]) == 0                          # the three-argument form is unchanged
    assert capsys.readouterr().out.strip() == _accept("X25519").source().strip()
    assert main(["32", "NIST521", "accept", text, "--source"]) == 2
    assert main(["32", "X25519", "lazy", "in x, y; out modadd_lazy(x, y)", "--source"]) == 2
    assert "not offered at word length 32" in capsys.readouterr().out


def test_w32_chain_cross_compiles_inside_the_register_file(tmp_path):
    assert os.path.exists(_lib.LIB_PATH), "libmodarith_amd.so is not built: run __graft_entry__.build()"
    ch = Chain("NIST256", "twoout", wl=32)
    x, y = ch.inputs(2)
    t, w = ch.modadd(x, y), ch.modsub(x, y)
    ch.output(ch.modmul(t, w))
    ch.output(ch.modmli(ch.modsqr(t), 121665))
    f = ch.build(plugin_dir=str(tmp_path))
    assert f.built and os.path.exists(f.path) and hasattr(f.lib, "chain_twoout_NIST256_w32_batch")
    assert os.path.basename(f.path) == "libmodarith_amd_chain_twoout_NIST256_w32.so"
    assert "HEAVY = false" in ch.source()
    assert not ch.build(plugin_dir=str(tmp_path)).built          # cached by content
    obj = str(tmp_path / "chain_twoout_NIST256_w32.o")
    widths = lambda ks: sorted(k["name"][k["name"].index("k_chain<"):][:10] for k in ks)
    ks = [k for k in kernel_resources.kernels_of(obj) if "k_chain" in k["name"]]
    assert widths(ks) == ["k_chain<%d>" % e for e in range(1, W32_EPT_DEFAULT + 1) if e != 3]     # the default width and what its tails need
    assert ch.build(plugin_dir=str(tmp_path), ept=4).built       # another launch shape is another unit: every width
    ks += [k for k in kernel_resources.kernels_of(obj) if "k_chain" in k["name"]]
    assert widths(ks[-3:]) == ["k_chain<1>", "k_chain<2>", "k_chain<4>"]
    for k in ks:
        assert k["private_segment_fixed_size"] == 0 and k["vgpr_spill_count"] == 0 and k["agpr_count"] == 0, k
    # the 64-bit chain of the same name lives beside it
    ch64 = Chain("NIST256", "twoout")
    x, y = ch64.inputs(2)
    ch64.output(ch64.modmul(x, y))
    assert os.path.basename(ch64.lib_path(str(tmp_path))) == "libmodarith_amd_chain_twoout_NIST256.so"


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_built_library_holds_the_shared_inversion_without_spills(P):
    obj = os.path.join(ROOT, "modarith_amd", "build", "capi_%s_w32.o" % P)
    assert os.path.exists(obj), "no built objects: run __graft_entry__.build()"
    ks = [k for k in kernel_resources.kernels_of(obj) if "ma32::k_inv_simul<" in k["name"]]
    assert len(ks) == 1, [k["name"] for k in ks]
    assert ks[0]["vgpr_spill_count"] == 0 and ks[0]["agpr_count"] == 0, ks[0]
    print(P, ks[0])


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_predicate_admits_what_the_field_functions_return(P):
    """the cap on the fallback: a batch of field elements takes the shared path, element for element"""
    fp = derive(P, wl=32)
    N, R, _, _, p = wi.SHAPES[P]
    for cls in ("uniform", "plus_p"):                   # every element of the 2^18-element bulk classes
        for soa in wi.bulk_inputs(P, cls):
            ok = w32_inv_in_contract(fp, soa)
            assert ok.shape == (wi.BULK_N,) and ok.all(), (cls, int((~ok).sum()))
            assert all(w32_inv_in_contract(fp, [int(v) for v in soa[:, j]]) for j in range(0, wi.BULK_N, 4099))     # (the scalar form agrees)
    pool = wi.pool(P)
    below_2p = [t for t in pool if wi.value(P, t) < 2 * p and not max(t[:-1]) >> R]
    assert len(below_2p) >= 25 + 2 * 24 and all(w32_inv_in_contract(fp, t) for t in below_2p)
    assert w32_inv_in_contract(fp, wi.split(P, 2 * p)) and w32_inv_in_contract(fp, wi.split(P, p)) and w32_inv_in_contract(fp, [0] * N)
    assert not w32_inv_in_contract(fp, [wi.M32] * N)
    assert not w32_inv_in_contract(fp, [(1 << (R + 2)) - 1] * N) and not w32_inv_in_contract(fp, [1 << R] + [0] * (N - 1))
    topb = fp.n + 1 - R * (N - 1)
    assert w32_inv_in_contract(fp, [(1 << R) - 1] * (N - 1) + [(1 << topb) - 1]) and not w32_inv_in_contract(fp, [0] * (N - 1) + [1 << topb])
    with pytest.raises(ValueError):
        w32_inv_in_contract(derive(P), [0] * derive(P).nlimbs)


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_products_are_congruent_at_the_edge_of_the_predicate(host, P):  # noqa: F811
    """what the comment at inv_in_contract derives, checked on the arithmetic itself (csrc/field.h on the host): for the largest
    admitted operands, for random admitted ones and for running products of them, modmul is congruent to a b / R, returns an
    admitted element below 2p, and modis0 of it says exactly whether the value is zero"""
    fp = derive(P, wl=32)
    N, R, _, _, p = wi.SHAPES[P]
    topb = fp.n + 1 - R * (N - 1)
    Rinv = pow(fp.R, -1, p) if fp.montgomery else 1
    rng = random.Random(4100 + N)
    edge = [(1 << R) - 1] * (N - 1) + [(1 << topb) - 1]
    ops = [edge, wi.split(P, 2 * p - 1), wi.split(P, 2 * p), wi.split(P, p), [0] * N, wi.split(P, p - 1), wi.split(P, 1)]
    ops += [[rng.randrange(1 << R) for _ in range(N - 1)] + [rng.randrange(1 << topb)] for _ in range(12)]
    ops += [[rng.choice((0, (1 << R) - 1)) for _ in range(N - 1)] + [rng.choice((0, (1 << topb) - 1))] for _ in range(12)]
    assert all(w32_inv_in_contract(fp, a) for a in ops)
    # the set W of the comment is wider than the predicate for product outputs of the pseudo-Mersenne form: limb 1 up to 2^Radix + 2^15 - 1
    slack = []
    if not fp.montgomery:
        slack = [[(1 << R) - 1, (1 << R) + (1 << 15) - 1] + [(1 << R) - 1] * (N - 3) + [(1 << (topb - 1)) - 1],
                 [0, (1 << R) + (1 << 15) - 1] + [rng.randrange(1 << R) for _ in range(N - 3)] + [(1 << (topb - 1)) - 1]]
        assert not any(w32_inv_in_contract(fp, a) for a in slack)       # (never an input element: a prefix or the running inverse)
    checked = 0
    for a in ops + slack:                                # (a slack operand on the left, where the kernel has its prefixes ...)
        c = a
        for b in ops + [edge] * 3 + slack:               # (... and on the right: inv * c_{r-1} multiplies two product outputs)                       # a running product, as the forward pass keeps it
            want = wi.value(P, c) * wi.value(P, b) * Rinv % p
            c = host.call(P, "modmul", c, b)[1]
            assert wi.value(P, c) % p == want and wi.value(P, c) < 2 * p, (P, a, b)
            assert c[N - 1] >> topb == 0 and all(v < (1 << R) + (1 << 15) for v in c[:N - 1])
            assert host.call(P, "modis0", c)[0] == (1 if want == 0 else 0)
            if want == 0:
                c = a if wi.value(P, a) % p else edge    # (the kernel keeps zeros out of the running product)
            checked += 1
    assert checked == (len(ops) + len(slack)) * (len(ops) + 3 + len(slack))
