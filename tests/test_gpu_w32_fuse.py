"""Fused chains of the 32-bit word form on the GPU (modarith_amd/fuse.py Chain(prime, name, wl=32)): one kernel per chain, words equal
to the call-by-call sequence of Field(P, wl=32) over batches made of tests/w32_inputs.pool(P) -- every class: canonical, [p, 2p),
budget edge, all-maximal, arbitrary 32-bit words -- in every layout and at every width; and one-operation chains against the
reference's own words (tests/golden/field_w32_<P>.json.xz)."""
import random

import pytest

from tests import w32_inputs as wi
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
A24 = {"X25519": 121665, "NIST256": 121665, "X448": 39081}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _signed(v):
    return v if v < (1 << 31) else v - (1 << 32)


def _pool_batch(torch, P, n, seed):
    """flat int32 [N, n]: elements of the pool, every one of them present, in a seeded order"""
    pool = wi.pool(P)
    rng = random.Random(seed)
    pick = list(range(len(pool))) + [rng.randrange(len(pool)) for _ in range(n - len(pool))]
    rng.shuffle(pick)
    rows = [[_signed(v) for v in pool[i]] for i in pick[:n]]
    return torch.tensor(rows, dtype=torch.int32, device="cuda").T.contiguous()


# ---- the chains, each with its call-by-call twin over Field(P, wl=32).  (inputs, selectors) -> outputs
def _accept(P):
    from modarith_amd.fuse import Chain
    ch = Chain(P, "accept", wl=32)
    x, y = ch.inputs(2)
    ch.output(ch.modinv(ch.modsqr(ch.modmul(ch.modadd(x, y), ch.modsub(x, y)))))
    return ch


def _accept_calls(F, t, s):
    x, y = t
    return [F.modinv(F.modsqr(F.modmul(F.modadd(x, y), F.modsub(x, y))))]


def _double(P):
    """the doubling half of a ladder step (rfc7748.c: A, B, AA, BB, E, x2 = AA BB, z2 = E (AA + a24 E)): nine calls"""
    from modarith_amd.fuse import Chain
    ch = Chain(P, "double", wl=32)
    x2, z2 = ch.inputs(2)
    A, B = ch.modadd(x2, z2), ch.modsub(x2, z2)
    AA, BB = ch.modsqr(A), ch.modsqr(B)
    E = ch.modsub(AA, BB)
    ch.output(ch.modmul(AA, BB))
    ch.output(ch.modmul(E, ch.modadd(AA, ch.modmli(E, A24[P]))))
    assert len(ch.ops) == 9
    return ch


def _double_calls(F, t, s):
    x2, z2 = t
    A, B = F.modadd(x2, z2), F.modsub(x2, z2)
    AA, BB = F.modsqr(A), F.modsqr(B)
    E = F.modsub(AA, BB)
    return [F.modmul(AA, BB), F.modmul(E, F.modadd(AA, F.modmli(E, A24[F.prime])))]


def _step(P):
    """a full ladder step with two modcsw selectors, written with modadd / modsub (this word length has no generic=False forms)"""
    from modarith_amd.fuse import Chain
    ch = Chain(P, "ladderstep", wl=32)
    x1, x2, z2, x3, z3 = ch.inputs(5)
    s0, s1 = ch.selector(), ch.selector()
    x2, x3 = ch.modcsw(s0, x2, x3)
    z2, z3 = ch.modcsw(s1, z2, z3)
    A, B, C, D = ch.modadd(x2, z2), ch.modsub(x2, z2), ch.modadd(x3, z3), ch.modsub(x3, z3)
    AA, BB, DA, CB = ch.modsqr(A), ch.modsqr(B), ch.modmul(D, A), ch.modmul(C, B)
    E = ch.modsub(AA, BB)
    for v in (ch.modmul(AA, BB), ch.modmul(E, ch.modadd(AA, ch.modmli(E, A24[P]))), ch.modsqr(ch.modadd(DA, CB)), ch.modmul(x1, ch.modsqr(ch.modsub(DA, CB)))):
        ch.output(v)
    return ch


def _step_calls(F, t, s):
    X1, X2, Z2, X3, Z3 = [x.clone() for x in t]
    F.modcsw(s[0], X2, X3)
    F.modcsw(s[1], Z2, Z3)
    A, B, C, D = F.modadd(X2, Z2), F.modsub(X2, Z2), F.modadd(X3, Z3), F.modsub(X3, Z3)
    AA, BB, DA, CB = F.modsqr(A), F.modsqr(B), F.modmul(D, A), F.modmul(C, B)
    E = F.modsub(AA, BB)
    return [F.modmul(AA, BB), F.modmul(E, F.modadd(AA, F.modmli(E, A24[F.prime]))), F.modsqr(F.modadd(DA, CB)), F.modmul(X1, F.modsqr(F.modsub(DA, CB)))]


def _misc(P):
    """modmli modnsqr modhaf modsqrt modpro nres redc modneg modcpy modcmv in one chain"""
    from modarith_amd.fuse import Chain
    ch = Chain(P, "misc", wl=32)
    a, b = ch.inputs(2)
    d = ch.selector()
    u = ch.modhaf(ch.modnsqr(ch.modmli(a, -3), 3))
    v = ch.modneg(ch.redc(ch.nres(b)))
    w = ch.modcmv(d, u, ch.modcpy(v))
    ch.output(ch.modsqrt(w))
    ch.output(ch.modpro(u))
    ch.output(w)
    return ch


def _misc_calls(F, t, s):
    a, b = t
    u = F.modhaf(F.modnsqr(F.modmli(a, -3), 3))
    v = F.modneg(F.redc(F.nres(b)))
    w = F.modcmv(s[0], u, F.modcpy(v))
    return [F.modsqrt(w), F.modpro(u), w]


CHAINS = {"accept": (_accept, _accept_calls), "double": (_double, _double_calls), "ladderstep": (_step, _step_calls), "misc": (_misc, _misc_calls)}


def build(ch, ept=None):
    """the plug-in of a chain at one width; the explicit widths are kept apart from the default one (a plug-in's name does not carry it)"""
    import os
    from modarith_amd import generate as gen
    return ch.build(ept=ept, plugin_dir=os.path.join(gen.PLUGIN_DIR, "w32_ept%d" % ept) if ept else None)


def _check(torch, F, f, calls, t, s, what):
    want = calls(F, t, s)
    got = f(*t, *s)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        bad = (F.to_flat(g) != F.to_flat(w)).any(dim=0).nonzero().flatten().tolist()
        assert not bad, "%s, output %d: %d elements differ, first at %r" % (what, k, len(bad), bad[:8])


@pytest.mark.parametrize("name", list(CHAINS))
@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_w32_chain_equals_the_call_sequence(torch_cuda, P, name):
    torch = torch_cuda
    from modarith_amd.field import Field
    F = Field(P, wl=32, tile=None)
    make, calls = CHAINS[name]
    ch = make(P)
    heavy = name in ("accept", "misc")
    n = 2 * 4096 + 3 if heavy else 3 * 4096 + 3                                      # odd, and not a multiple of four: every width has a tail
    ld = n + 5                                                                    # rows of a wider buffer: a stride that is a multiple of four
    assert ld % 4 == 0

    def rows(seed):
        big = torch.zeros((F.N, ld), dtype=torch.int32, device="cuda")
        big[:, :n] = _pool_batch(torch, P, n, seed)
        assert big.data_ptr() % 16 == 0
        return big
    bufs = [rows(100 * k + len(name)) for k in range(ch.nin)]
    t = [b[:, :n] for b in bufs]
    s = [torch.randint(0, 2, (n,), dtype=torch.int32, device="cuda") for _ in range(ch.nsel)]
    for ept in ((None,) if heavy else (None, 1, 2, 4)):
        f = build(ch, ept)
        what = "%s %s ept=%r" % (P, name, ept)
        _check(torch, F, f, calls, t, s, what + " flat")                          # aligned rows, n = 4 k + 3
        # unaligned by one element (4-byte accesses whatever the width), an even count 8 bytes into the rows, a contiguous odd batch
        _check(torch, F, f, calls, [b[:, 1:n] for b in bufs], [d[1:].contiguous() for d in s], what + " off by one")
        _check(torch, F, f, calls, [b[:, 2:n - 1] for b in bufs], [d[2:n - 1].contiguous() for d in s], what + " off by two")
        _check(torch, F, f, calls, [x.contiguous() for x in t], s, what + " odd stride")
        # tiles of 4096 and of 128 (whole tiles)
        for tile in (4096, 128):
            m = 2 * 4096
            _check(torch, F, f, calls, [F.to_tiled(x[:, :m].contiguous(), tile) for x in t], [d[:m].contiguous() for d in s], what + " tiled %d" % tile)
        # outputs aliasing inputs: the first outputs written over the first inputs
        want = calls(F, t, s)
        tc = [b.clone()[:, :n] for b in bufs]                      # (the aligned rows again: every width)
        k = min(len(want), len(tc))
        outs = tc[:k] + [torch.zeros_like(bufs[0])[:, :n] for _ in range(len(want) - k)]
        got = f(*tc, *s, out=outs)
        for g, w in zip(got, want):
            assert torch.equal(g, w), what + " in place"


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_one_operation_chains_return_the_reference_words(torch_cuda, P):
    """modmul modsqr modadd modsub as chains of one call over the fixture's records: the reference's own outputs"""
    torch = torch_cuda
    from modarith_amd.fuse import Chain
    fx = load_golden("field_w32_%s.json" % P)
    pool = [wi.unpack(s) for s in fx["pool"]]
    dev = lambda rows: torch.tensor([[_signed(v) for v in r] for r in rows], dtype=torch.int32, device="cuda").T.contiguous()
    compared = 0
    for fn in ("modmul", "modsqr", "modadd", "modsub"):
        recs = fx["records"][fn]
        ch = Chain(P, "one_" + fn, wl=32)
        if fn == "modsqr":
            ch.output(ch.modsqr(ch.input()))
            ins = [dev([pool[r[0]] for r in recs])]
        else:
            a, b = ch.inputs(2)
            ch.output(getattr(ch, fn)(a, b))
            ins = [dev([pool[r[0]] for r in recs]), dev([pool[r[1]] for r in recs])]
        want = dev([wi.unpack(r[-1]) for r in recs])
        for ept in (1, 2, 4):
            z, = build(ch, ept)(*ins)
            bad = (z != want).any(dim=0).nonzero().flatten().tolist()
            assert not bad, (P, fn, ept, bad[:8])
        compared += len(recs)
    assert compared == sum(len(fx["records"][fn]) for fn in ("modmul", "modsqr", "modadd", "modsub"))
