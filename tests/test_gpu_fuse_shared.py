"""Fused chains with batch-wide operands (Chain.shared()) and field constants on the GPU, at both word lengths.  The truth is the
call-by-call sequence of Field(P, wl) with the shared element materialised as a broadcast batch -- every one of those calls is pinned
to the reference's words elsewhere in the suite --, compared with torch.equal; the one-operation chain is also compared with the
reference's own output words (tests/golden/field_<P>.json, field_w32_<P>.json) and, at 64 bits, with Field.modmuls.  Shapes are the
smallest that reach every branch of csrc/chain.inc's chain_batch / chain_aos: n = 1; n = 131 flat (the widest aligned width and a
remainder launch, which must see the same shared values); tiles of 128; an unaligned view; in place; n = 4 * 64 + 3 at four elements
per lane (32 bits); one chunk of 512 and one element through the element-major entry (64 bits)."""
import random

import numpy as np
import pytest

from tests import w32_inputs as wi
from tests.conftest import limbs, load_golden
from tests.util import derive_any

pytestmark = pytest.mark.gpu
GENERATED = "2519"
CASES = [(P, wl) for P in ("X25519", "NIST256", "X448") for wl in (64, 32)] + [(GENERATED, 64)]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-w%d" % c)
def ctx(request, torch_cuda):
    from modarith_amd import generate as gen
    from modarith_amd.field import Field
    P, wl = request.param
    if P == GENERATED and gen.find_field(P, wl=64, built=True) is None:
        pytest.skip("no plug-in of the generated field %s in this tree" % P)
    return P, wl, Field(P, wl=wl, tile=None)


# ---------------------------------------------------------------------------------------------------------------- operands
def _elements(P, wl, n, seed):
    """n elements as rows of unsigned limbs: 64 bits -- every limb uniform below 2^Radix, the top limb spanning the bits of a value
    below 2^Nbits (inside the limb contract, not canonical); 32 bits -- canonical values and values in [p, 2p) of the operand pool's
    recipe (what the field functions return)"""
    if wl == 64:
        fp = derive_any(P)
        rng = np.random.default_rng(seed)
        out = rng.integers(0, 1 << fp.radix, size=(n, fp.nlimbs), dtype=np.uint64)
        out[:, fp.nlimbs - 1] = rng.integers(0, 1 << (fp.n - fp.radix * (fp.nlimbs - 1)), size=n, dtype=np.uint64)
        return [[int(v) for v in r] for r in out]
    p = wi.SHAPES[P][4]
    rng = random.Random(seed)
    return [wi.split(P, rng.randrange(0, 2 * p)) for _ in range(n)]


def _dev(torch, wl, rows, width=None):
    """rows of unsigned limbs -> flat device batch [N, n] of the word length's signed dtype, in rows of `width` words (a view when wider)"""
    arr = np.array(rows, dtype=np.uint64 if wl == 64 else np.uint32).view(np.int64 if wl == 64 else np.int32)
    t = torch.empty((arr.shape[1], arr.shape[0]), dtype=torch.int64 if wl == 64 else torch.int32, device="cuda")     # (fresh rows: unit element stride at n = 1 too)
    t.copy_(torch.from_numpy(arr).T)
    if width is None or width == t.shape[1]:
        return t
    big = torch.zeros((t.shape[0], width), dtype=t.dtype, device="cuda")
    big[:, :t.shape[1]] = t
    return big[:, :t.shape[1]]


def _batch(torch, P, wl, n, seed, width=None):
    return _dev(torch, wl, _elements(P, wl, n, seed), width)


def _bcast(torch, wl, b, like):
    """the shared element b (unsigned limbs) as the batch a call-by-call caller streams: the shape and layout of `like`"""
    col = _dev(torch, wl, [b])
    if like.dim() == 3:
        return col.reshape(1, -1, 1).expand(like.shape).contiguous()
    return col.expand(like.shape[0], like.shape[1]).contiguous()


# ---------------------------------------------------------------------------------------------------------------- chains
def _chain(P, wl, name):
    from modarith_amd.fuse import Chain
    return Chain(P, name + "_sh", wl=wl)


_BUILT = {}


def _built(P, wl, make, **kw):
    key = (P, wl, make.__name__, tuple(sorted(kw.items())))
    if key not in _BUILT:
        ch = make(P, wl)
        if kw:                                                  # a plug-in's name does not carry its launch shape: explicit ones apart
            import os
            from modarith_amd import generate as gen
            kw["plugin_dir"] = os.path.join(gen.PLUGIN_DIR, "w32_ept%d" % kw["ept"])
        _BUILT[key] = ch.build(**kw)
    return _BUILT[key]


def _mul(P, wl):
    ch = _chain(P, wl, "mul")
    x = ch.input()
    ch.output(ch.modmul(x, ch.shared()))
    return ch


def _mul_calls(F, t, b, s):
    return [F.modmul(t[0], b[0])]


def _edadd(P, wl):
    """x y d + t and x d - t: the shape of an Edwards addition (edwards.c: the products of coordinates times the curve's d), two results"""
    ch = _chain(P, wl, "edadd")
    x, y, t = ch.inputs(3)
    d = ch.shared()
    ch.output(ch.modadd(ch.modmul(ch.modmul(x, y), d), t))
    ch.output(ch.modsub(ch.modmul(d, x), t))
    return ch


def _edadd_calls(F, t, b, s):
    x, y, tt = t
    return [F.modadd(F.modmul(F.modmul(x, y), b[0]), tt), F.modsub(F.modmul(b[0], x), tt)]


def _uses(P, wl):
    """a shared operand on either side of modadd / modsub, as g of modcmv and as f of modcsw"""
    ch = _chain(P, wl, "uses")
    x, y = ch.inputs(2)
    b, c = ch.shared(), ch.shared()
    s0, s1 = ch.selector(), ch.selector()
    u = ch.modadd(x, b)
    v = ch.modsub(c, y)
    w = ch.modcmv(s0, b, u)                                      # s0 ? b : u
    g2, f2 = ch.modcsw(s1, v, c)                                 # (c as f; b as g above)
    ch.output(ch.modadd(w, g2))
    ch.output(f2)
    return ch


def _uses_calls(F, t, sh, s):
    x, y = t
    b, c = sh
    u = F.modadd(x, b)
    v = F.modsub(c, y)
    w = F.modcmv(s[0], b, u.clone())
    g2, f2 = F.modcsw(s[1], v.clone(), c.clone())
    return [F.modadd(w, g2), f2]


def _two(P, wl):
    """products by two different shared operands, on either side: b and c are told apart"""
    ch = _chain(P, wl, "two")
    x, y = ch.inputs(2)
    b, c = ch.shared(), ch.shared()
    ch.output(ch.modmul(x, b))
    ch.output(ch.modmul(c, y))
    return ch


def _two_calls(F, t, sh, s):
    return [F.modmul(t[0], sh[0]), F.modmul(sh[1], t[1])]


def _consts(P, wl):
    """modint(5), modone() and modzer() as operands, a negative modint, and a shared operand under unary operations"""
    ch = _chain(P, wl, "consts")
    x = ch.input()
    b = ch.shared()
    k = ch.modadd(ch.modint(5), ch.modsub(ch.modone(), ch.modzer()))
    ch.output(ch.modmul(x, k))
    ch.output(ch.modadd(ch.modsqr(b), ch.modmli(ch.modneg(b), 3)))
    ch.output(ch.modmul(x, ch.modint(-7)))
    return ch


def _consts_calls(F, t, sh, s):
    x, b = t[0], sh[0]
    n = F._chk(x)
    const = lambda a: a if x.dim() == 2 else F.to_tiled(a, x.shape[2])
    k = F.modadd(const(F.modint(5, n)), F.modsub(const(F.modone(n)), const(F.modzer(n))))
    return [F.modmul(x, k), F.modadd(F.modsqr(b), F.modmli(F.modneg(b), 3)), F.modmul(x, const(F.modint(-7, n)))]


def _inv(P, wl):
    """HEAVY: one element per lane; b reaches every element's inversion"""
    ch = _chain(P, wl, "inv")
    x = ch.input()
    ch.output(ch.modinv(ch.modmul(x, ch.shared())))
    return ch


def _inv_calls(F, t, b, s):
    return [F.modinv(F.modmul(t[0], b[0]))]


def _check(torch, F, f, calls, t, shared, s, what, out=None):
    """f(batches, shared limbs, selectors) against calls(batches, broadcast batches, selectors).  The truth is taken first: `out` may
    alias the inputs"""
    wl = F.wl
    want = calls(F, [x.contiguous() if x.dim() == 2 else x for x in t], [_bcast(torch, wl, b, t[0] if t[0].dim() == 3 else t[0].contiguous()) for b in shared], s)
    got = f(*t, *shared, *s, out=out)
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(F.to_flat(g), F.to_flat(w)), "%s, output %d" % (what, k)


def _sels(torch, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 2, (n,), dtype=torch.int32, generator=g).cuda() for _ in range(k)]


def _shapes(torch, ctx, make, calls, seed):
    """every branch of chain_batch for one chain: n = 1, n = 131 in aligned rows, tiles of 128, an unaligned view, in place"""
    P, wl, F = ctx
    ch = make(P, wl)
    f = _built(P, wl, make)
    shared = _elements(P, wl, ch.nshared, seed + 50)
    what = "%s w%d %s" % (P, wl, ch.name)
    one = [_batch(torch, P, wl, 1, seed + i) for i in range(ch.nin)]
    _check(torch, F, f, calls, one, shared, _sels(torch, 1, ch.nsel, seed), what + " n = 1")
    rows = [_batch(torch, P, wl, 131, seed + 10 + i, width=132) for i in range(ch.nin)]     # aligned rows of an even stride (and a multiple of 4)
    assert all(x.data_ptr() % 16 == 0 for x in rows)
    s = _sels(torch, 131, ch.nsel, seed + 1)
    _check(torch, F, f, calls, rows, shared, s, what + " n = 131")
    _check(torch, F, f, calls, [x[:, 1:100] for x in rows], shared, [d[1:100].contiguous() for d in s], what + " unaligned")
    flat = [_batch(torch, P, wl, 384, seed + 20 + i) for i in range(ch.nin)]
    s = _sels(torch, 384, ch.nsel, seed + 2)
    _check(torch, F, f, calls, [F.to_tiled(x, 128) for x in flat], shared, s, what + " tiled")
    mine = [x.clone() for x in flat]
    outs = [mine[0]] + [torch.empty_like(mine[0]) for _ in ch.outs[1:]]
    _check(torch, F, f, calls, mine, shared, s, what + " in place", out=outs)
    return ch, f, shared


# ---------------------------------------------------------------------------------------------------------------- tests
def test_shared_multiplicand(torch_cuda, ctx):
    torch = torch_cuda
    P, wl, F = ctx
    ch, f, (b,) = _shapes(torch, ctx, _mul, _mul_calls, 100)
    assert ch.traffic_bytes() == 2 * (wl // 8) * F.N
    if wl == 64:
        x = _batch(torch, P, wl, 131, 7, width=132)
        assert torch.equal(f(x, b)[0], F.modmuls(x, b))
        assert torch.equal(f(x, torch.tensor(np.array(b, dtype=np.uint64).view(np.int64)))[0], F.modmuls(x, b))     # a CPU integer tensor
    else:
        f4 = _built(P, wl, _mul, ept=4)
        x = _batch(torch, P, wl, 4 * 64 + 3, 8, width=4 * 64 + 4)
        _check(torch, F, f4, _mul_calls, [x], [b], [], "%s w32 mul ept=4" % P)
    with pytest.raises(ValueError, match="1 element batches followed by 1 shared operands"):
        f(_batch(torch, P, wl, 1, 1))
    with pytest.raises(ValueError, match="limbs on the host"):
        f(_batch(torch, P, wl, 1, 1), b[:-1])


def test_shared_multiplicand_returns_the_reference_words(torch_cuda, ctx):
    """up to 16 modmul records of the prime's fixture, one call of n = 1 per record, the record's second operand shared"""
    torch = torch_cuda
    P, wl, F = ctx
    f = _built(P, wl, _mul)
    if wl == 64:
        g = load_golden("field_%s.json" % P)
        recs = [(limbs(a), limbs(b), limbs(c)) for a, b, c in zip(g["A"], g["B"], g["ops"]["modmul"])]
    else:
        g = load_golden("field_w32_%s.json" % P)
        pool = [wi.unpack(s) for s in g["pool"]]
        recs = [(pool[r[0]], pool[r[1]], wi.unpack(r[-1])) for r in g["records"]["modmul"]]
    step = max(1, len(recs) // 16)
    picked = recs[::step][:16]
    assert len(picked) == min(16, len(recs))
    for a, b, c in picked:
        z, = f(_dev(torch, wl, [a]), b)
        assert torch.equal(z, _dev(torch, wl, [c])), (P, wl, a, b)


def test_edwards_add_shape_with_two_results(torch_cuda, ctx):
    torch = torch_cuda
    P, wl, F = ctx
    ch, f, (d,) = _shapes(torch, ctx, _edadd, _edadd_calls, 200)
    assert ch.traffic_bytes() == 5 * (wl // 8) * F.N
    if wl == 32:
        f4 = _built(P, wl, _edadd, ept=4)
        t = [_batch(torch, P, wl, 4 * 64 + 3, 30 + i, width=4 * 64 + 4) for i in range(3)]
        _check(torch, F, f4, _edadd_calls, t, [d], [], "%s w32 edadd ept=4" % P)
    else:
        n = 513                                                  # one chunk of 512 and one element
        t = [_batch(torch, P, wl, n, 40 + i) for i in range(3)]
        want = f(*t, d)
        got = f.aos(*[F.to_aos(x) for x in t], d)
        for k in range(2):
            assert torch.equal(got[k], F.to_aos(want[k])), (P, k)


def test_every_use_of_a_shared_operand(torch_cuda, ctx):
    torch = torch_cuda
    P, wl, F = ctx
    ch, f, shared = _shapes(torch, ctx, _uses, _uses_calls, 300)
    assert shared[0] != shared[1]
    if wl == 64:
        n = 513
        t = [_batch(torch, P, wl, n, 60 + i) for i in range(2)]
        s = _sels(torch, n, 2, 61)
        want = f(*t, *shared, *s)
        got = f.aos(*[F.to_aos(x) for x in t], *shared, *s)
        for k in range(len(want)):
            assert torch.equal(got[k], F.to_aos(want[k])), (P, k)


def test_two_shared_operands_are_not_crossed(torch_cuda, ctx):
    ch, f, shared = _shapes(torch_cuda, ctx, _two, _two_calls, 320)
    assert shared[0] != shared[1]


def test_constants_as_operands(torch_cuda, ctx):
    _shapes(torch_cuda, ctx, _consts, _consts_calls, 350)


def test_shared_operand_in_front_of_an_inversion(torch_cuda, ctx):
    _shapes(torch_cuda, ctx, _inv, _inv_calls, 400)


@pytest.mark.parametrize("P", ["X25519", "NIST256", "X448"])
def test_out_of_contract_limbs_take_the_exact_products(torch_cuda, P):
    """64 bits.  Shared limbs 2^63 + ... up to 2^64 - 1 beside element operands inside the contract: the whole launch runs the exact
    products and returns the words of Field.modmul on the broadcast batch, which takes them in every wave.  And the converse: a shared
    operand inside the contract, a few lanes outside (the lanes of tests/test_gpu_fuse.py's test of the same name)"""
    torch = torch_cuda
    from modarith_amd.field import Field
    F, wl = Field(P, tile=None), 64
    rng = random.Random(900 + F.N)
    for make, calls in ((_mul, _mul_calls), (_edadd, _edadd_calls)):
        ch = make(P, wl)
        f = _built(P, wl, make)
        wild = [(1 << 63) + rng.randrange(0, 1 << 63) for _ in range(F.N)]
        wild[0] = (1 << 64) - 1
        for n, width in ((1, None), (131, 132)):
            t = [_batch(torch, P, wl, n, 500 + i, width) for i in range(ch.nin)]
            _check(torch, F, f, calls, t, [wild], [], "%s %s wild shared n = %d" % (P, ch.name, n))
        if make is _edadd:
            t = [_batch(torch, P, wl, 513, 510 + i) for i in range(3)]
            want = f(*t, wild)
            got = f.aos(*[F.to_aos(x) for x in t], wild)
            assert torch.equal(got[0], F.to_aos(want[0])) and torch.equal(got[1], F.to_aos(want[1]))
        n = 1 << 14
        rows = [_elements(P, wl, n, 520 + i) for i in range(ch.nin)]
        for j in list(range(0, n, 997)) + list(range(4096, 4096 + 256)):
            rows[0][j] = [rng.randrange(0, 1 << 64) for _ in range(F.N)]
        tame, = _elements(P, wl, 1, 530)
        _check(torch, F, f, calls, [_dev(torch, wl, r) for r in rows], [tame], [], "%s %s wild lanes" % (P, ch.name))


def test_a_captured_call_keeps_the_value_it_was_captured_with(torch_cuda):
    """the shared operand travels in the kernel arguments: one capture of a shared-multiplicand call on a single stream, the host limbs
    overwritten afterwards, two replays on fresh batches -- both multiply by the captured value"""
    torch = torch_cuda
    from modarith_amd.field import Field
    P, wl = "X25519", 64
    F = Field(P, tile=None)
    f = _built(P, wl, _mul)
    b, other = _elements(P, wl, 2, 700)
    host = torch.tensor(np.array(b, dtype=np.uint64).view(np.int64))
    n = 131
    x = _batch(torch, P, wl, n, 701, width=132)
    z = torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)      # (rows of the same even stride: two elements per lane and a remainder launch)
    f(x, host, out=[z])                                          # warm-up outside the capture (code object, Field binding)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            f(x, host, out=[z])
    torch.cuda.current_stream().wait_stream(side)
    host.copy_(torch.tensor(np.array(other, dtype=np.uint64).view(np.int64)))
    for seed in (702, 703):
        x.copy_(_batch(torch, P, wl, n, seed))
        z.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(z, F.modmuls(x, b)) and not torch.equal(z, F.modmuls(x, other))
