"""Fused chains with ints computed inside them, on the GPU and at both word lengths: the predicates modis0 / modis1 / modsign / modcmp /
modqr, the 0/1 expressions, computed selectors of modcmv / modcsw, the progenitor passed to modqr / modsqrt / modinv, int32 results.
The truth is the call-by-call sequence through Field(P, wl) -- every one of those calls is pinned to the reference's words elsewhere in
the suite --, compared with torch.equal; the one-operation chains are also compared with the reference's recorded values (the fixtures
tests/test_gpu_parity.py and tests/test_gpu_w32_parity.py read) and with the Euler criterion; the decompression chain with Curve.set.
Operands: the pools of tests/w32_inputs.py and of the 64-bit fixtures, extended here by 0, 1, p (the zero that is not canonical), p + 1,
p - 1, their Montgomery forms, pairs equal in value and different in limbs, residues and non-residues, so that every predicate takes
both values (asserted).  Shapes are the smallest that reach every branch of csrc/chain.inc for the int arrays."""
import concurrent.futures as cf
import os
import random

import pytest

from tests import w32_inputs as wi
from tests.conftest import limbs, load_golden
from tests.test_gpu_fuse_shared import _bcast, _dev, _elements
from tests.util import derive_any

pytestmark = pytest.mark.gpu
GENERATED = "2519"
CASES = [(P, wl) for P in ("X25519", "NIST256", "X448") for wl in (64, 32)] + [(GENERATED, 64)]
SELECT = "in u, v; sel s; d = (modsign(u) ^ s) & (not modis0(v)); w = modcmv(d, modneg(u), u); g2, f2 = modcsw(modcmp(u, v), u, v); out w, g2, f2, d"
# the same decisions behind a product with a shared operand: what the vote of the 64-bit form has to get right
WILD = "in u; shared c; sel s; t = modmul(u, c); d = (modsign(t) ^ s) & (not modis0(u)); out modcmv(d, modneg(t), t), modcmv(modcmp(t, c), c, u), d"
ONE_OP = {"modis0": "in a; out modis0(a)", "modis1": "in a; out modis1(a)", "modsign": "in a; out modsign(a)", "modcmp": "in a, b; out modcmp(a, b)",
          "modqr": "in a; out modqr(a)"}
PROG_H = "in a; h = modpro(a); out modsqrt(a, h), modinv(a, h), modqr(a, h)"
PROG_0 = "in a; out modsqrt(a), modinv(a), modqr(a)"


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _parse(P, wl, name, text):
    from modarith_amd.fuse import parse
    return parse(P, name + "_pr", text, wl=wl)


_BUILT = {}


def _built(P, wl, name, text, **kw):
    key = (P, wl, name, tuple(sorted(kw.items())))
    if key not in _BUILT:
        _BUILT[key] = _parse(P, wl, name, text).build(plugin_dir=_plugin_dir(**kw), **kw)
    return _BUILT[key]


def _plugin_dir(ept=None):
    """the library's directory; a plug-in's name does not carry its launch shape: explicit ones apart"""
    from modarith_amd import generate as gen
    return gen.PLUGIN_DIR if ept is None else os.path.join(gen.PLUGIN_DIR, "w32_ept%d" % ept)


def _units(P, wl):
    """every plug-in of one case: (name, text, build arguments)"""
    u = [(k, t, {}) for k, t in ONE_OP.items()] + [("select", SELECT, {}), ("prog_h", PROG_H, {}), ("prog_0", PROG_0, {})]
    if wl == 32:
        u += [("select", SELECT, {"ept": 2}), ("select", SELECT, {"ept": 4})]
    elif P != GENERATED:
        u.append(("wild", WILD, {}))
    return u


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-w%d" % c)
def ctx(request, torch_cuda):
    from modarith_amd import generate as gen
    from modarith_amd.field import Field
    P, wl = request.param
    if P == GENERATED and gen.find_field(P, wl=64, built=True) is None:
        pytest.skip("no plug-in of the generated field %s in this tree" % P)
    with cf.ThreadPoolExecutor(max_workers=8) as ex:             # independent hipcc units, seconds each: side by side
        for j in [ex.submit(_built, P, wl, name, text, **kw) for name, text, kw in _units(P, wl)]:
            j.result()
    return P, wl, Field(P, wl=wl, tile=None)


# ---------------------------------------------------------------------------------------------------------------- operands
def _fp(P, wl):
    from modarith_amd.params import derive
    return derive_any(P) if wl == 64 else derive(P, wl=32)


def _pool_values(P, wl):
    """internal-form integers below 2p: the directed ones first -- 0, 1, p, p + 1, p - 1, 2p - 1, the Montgomery forms of 0, 1, -1 (the
    same numbers again where the field is not a Montgomery one) and those plus p --, then 40 seeded ones (residues and non-residues)"""
    fp = _fp(P, wl)
    p, R = fp.p, (fp.R % fp.p if fp.montgomery else 1)
    vals = [0, 1, p, p + 1, p - 1, 2 * p - 1, R, R + p, (p - 1) * R % p, (p - 1) * R % p + p, 2, 2 * R % p]
    rng = random.Random(4100 + fp.nlimbs + wl)
    return vals + [rng.randrange(0, 2 * p) for _ in range(40)]


def _rows(P, wl, vals):
    fp = _fp(P, wl)
    return [fp.to_limbs(v) for v in vals]                        # (the top limb takes everything left: values of p and more fit it)


def _plain(P, wl, vals):
    """the field elements the internal-form integers stand for"""
    fp = _fp(P, wl)
    Rinv = pow(fp.R, -1, fp.p) if fp.montgomery else 1
    return [v * Rinv % fp.p for v in vals]


def _pairs(P, wl):
    """(a, b) values for modcmp: equal limbs; equal in value and different in limbs (v and v + p, either way round); different values"""
    fp = _fp(P, wl)
    vals = _pool_values(P, wl)
    other = []
    for k, v in enumerate(vals):
        other.append(v if k % 3 == 0 else (v + fp.p if v < fp.p else v - fp.p) if k % 3 == 1 else vals[(k + 5) % len(vals)])
    return vals, other


def _sels(torch, n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 2, (n,), dtype=torch.int32, generator=g).cuda()


def _batch(torch, P, wl, n, seed, width=None):
    """n in-contract elements; the first of them the directed ones of the pool, so that zeros, ones and equal pairs are among them"""
    rows = (_rows(P, wl, _pool_values(P, wl)[:12]) + _elements(P, wl, max(n - 12, 0), seed))[:n]
    random.Random(seed).shuffle(rows)
    return _dev(torch, wl, rows, width)


def _same(torch, F, got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype, (what, k)
        if g.dtype == torch.int32 and g.dim() == 1:
            assert torch.equal(g, w), "%s, int output %d" % (what, k)
        else:
            assert torch.equal(F.to_flat(g), F.to_flat(w)), "%s, output %d" % (what, k)


def _both(t):
    v = set(t.tolist())
    return v == {0, 1}


# ---------------------------------------------------------------------------------------------------------------- the calls through Field
def _select_calls(F, u, v, s):
    d = (F.modsign(u) ^ s) & (1 - F.modis0(v))
    w = F.modcmv(d, F.modneg(u), u.clone())
    g2, f2 = F.modcsw(F.modcmp(u, v), u.clone(), v.clone())
    return [w, g2, f2, d]                                        # (the element results, then the int results: the order of out[])


def _wild_calls(F, u, c, s):
    t = F.modmul(u, c)
    d = (F.modsign(t) ^ s) & (1 - F.modis0(u))
    return [F.modcmv(d, F.modneg(t), t.clone()), F.modcmv(F.modcmp(t, c), c, u.clone()), d]


def _plainly(x):
    """what the call-by-call caller holds: rows of their own (a view of a wider batch is copied)"""
    return x.contiguous() if x.dim() == 2 else x


def _check_select(torch, F, f, u, v, s, what, out=None):
    want = _select_calls(F, _plainly(u).clone(), _plainly(v).clone(), s.clone())          # the truth first: `out` may alias the inputs
    _same(torch, F, f(u, v, s, out=out), want, what)
    return want


# ---------------------------------------------------------------------------------------------------------------- tests
def test_one_operation_chains_return_the_words_of_field_and_of_the_reference(torch_cuda, ctx):
    torch = torch_cuda
    P, wl, F = ctx
    f = {k: _built(P, wl, k, t) for k, t in ONE_OP.items()}
    vals, other = _pairs(P, wl)
    A, B = _dev(torch, wl, _rows(P, wl, vals)), _dev(torch, wl, _rows(P, wl, other))
    for k in ("modis0", "modis1", "modsign"):
        got, = f[k](A)
        assert got.dtype == torch.int32 and got.shape == (len(vals),)
        assert torch.equal(got, getattr(F, k)(A)) and _both(got), (P, wl, k)
    x = _plain(P, wl, vals)
    assert f["modis0"](A)[0].tolist() == [int(v == 0) for v in x] and f["modis1"](A)[0].tolist() == [int(v == 1) for v in x]
    assert f["modsign"](A)[0].tolist() == [v & 1 for v in x]
    got, = f["modcmp"](A, B)
    assert torch.equal(got, F.modcmp(A, B)) and _both(got)
    y = _plain(P, wl, other)
    assert got.tolist() == [int(a == b) for a, b in zip(x, y)] and sum(got.tolist()) > len(vals) // 2
    p = _fp(P, wl).p
    got, = f["modqr"](A)
    assert torch.equal(got, F.modqr(None, A)) and _both(got)
    assert got.tolist() == [1 if v == 0 or pow(v, (p - 1) // 2, p) == 1 else 0 for v in x]          # the Euler criterion
    # the reference's recorded values
    if wl == 64:
        g = load_golden("field_%s.json" % P)
        GA, GB, o = _dev(torch, wl, [limbs(r) for r in g["A"]]), _dev(torch, wl, [limbs(r) for r in g["B"]]), g["ops"]
        for k in ("modis0", "modis1", "modsign"):
            assert f[k](GA)[0].tolist() == o[k] == getattr(F, k)(GA).tolist(), (P, k)
        assert f["modcmp"](GA, GB)[0].tolist() == o["modcmp"]
        recs = load_golden("sqrt_%s.json" % P)["recs"]
        assert f["modqr"](_dev(torch, wl, [limbs(r["x"]) for r in recs]))[0].tolist() == [r["qr"] for r in recs]
    else:
        fx = load_golden("field_w32_%s.json" % P)
        pool = [wi.unpack(s) for s in fx["pool"]]
        for k in ("modis0", "modis1", "modsign"):
            recs = fx["records"][k]
            assert f[k](_dev(torch, wl, [pool[r[0]] for r in recs]))[0].tolist() == [r[1] for r in recs], (P, k)
        recs = fx["records"]["modcmp"]
        assert f["modcmp"](_dev(torch, wl, [pool[r[0]] for r in recs]), _dev(torch, wl, [pool[r[1]] for r in recs]))[0].tolist() == [r[2] for r in recs]


def test_computed_selectors_over_every_shape(torch_cuda, ctx):
    """d = (modsign(u) ^ s) & not modis0(v); modcmv(d, -u, u); modcsw(modcmp(u, v), u, v): ints computed in the chain select, and one of
    them is a result.  Every launch shape of chain_batch and chain_aos, the int arrays at odd offsets and aliased"""
    torch = torch_cuda
    P, wl, F = ctx
    f = _built(P, wl, "select", SELECT)
    ch = f.chain
    assert (ch.nin, ch.nsel, len(ch.outs), len(ch.pouts)) == (2, 1, 3, 1) and ch.traffic_bytes() == 5 * (wl // 8) * F.N + 8
    for n in (1, 3, 63, 64, 65, 4101):
        width = n + (n & 1) if n > 1 else None                  # aligned rows of an even stride: two elements per lane where the build has them, and a remainder
        u, v = _batch(torch, P, wl, n, 10 + n, width), _batch(torch, P, wl, n, 20 + n, width)
        if n >= 64:
            v[:, 5:40] = u[:, 5:40]                              # equal pairs: modcmp takes both values
        want = _check_select(torch, F, f, u, v, _sels(torch, n, n), "%s w%d n = %d" % (P, wl, n))
        if n >= 64:                                              # (the directed elements and the equal pairs are among them)
            assert _both(want[3]) and _both(F.modcmp(_plainly(u), _plainly(v))) and _both(F.modis0(_plainly(v)))
    n = 4101
    u, v, s = _batch(torch, P, wl, n, 31, n + 3), _batch(torch, P, wl, n, 32, n + 3), _sels(torch, n, 33)
    # element batches one element further on: the 16-byte rule fails, one element per lane; the int arrays follow by element
    _check_select(torch, F, f, u[:, 1:], v[:, 1:], s[1:].clone(), "%s w%d offset by one element" % (P, wl))
    # an int result at an odd int32 offset; an int result in the array of its selector; an element result in the array of an input
    m = 385
    u, v, s = _batch(torch, P, wl, m, 41, m + 1), _batch(torch, P, wl, m, 42, m + 1), _sels(torch, m, 43)
    room = torch.full((m + 2,), -7, dtype=torch.int32, device="cuda")
    fresh = lambda: [torch.empty_strided(u.shape, u.stride(), dtype=u.dtype, device="cuda") for _ in range(3)]
    _check_select(torch, F, f, u, v, s, "odd int offset", out=fresh() + [room[1:m + 1]])
    assert room[0].item() == -7 and room[m + 1].item() == -7 and room.data_ptr() % 8 == 0
    mine = s.clone()
    _check_select(torch, F, f, u, v, mine, "int output in its selector's array", out=fresh() + [mine])
    uu = fresh()[0].copy_(u)                                     # (rows of the stride the other operands have)
    _check_select(torch, F, f, uu, v, s, "element output in an input's array", out=[uu] + fresh()[:2] + [torch.empty_like(s)])
    for tile, n in ((128, 384), (4096, 8192)):
        u, v = _batch(torch, P, wl, n, 50 + tile), _batch(torch, P, wl, n, 51 + tile)
        _check_select(torch, F, f, F.to_tiled(u, tile), F.to_tiled(v, tile), _sels(torch, n, tile), "%s w%d tiles of %d" % (P, wl, tile))
    if wl == 32:
        for ept in (2, 4):
            fe = _built(P, wl, "select", SELECT, ept=ept)
            n = 4 * 64 + 3
            u, v = _batch(torch, P, wl, n, 60 + ept, n + 1), _batch(torch, P, wl, n, 61 + ept, n + 1)
            assert u.data_ptr() % 16 == 0 and u.stride(0) % 4 == 0
            _check_select(torch, F, fe, u, v, _sels(torch, n, ept), "%s w32 ept = %d" % (P, ept))
            _check_select(torch, F, fe, u[:, 1:], v[:, 1:], _sels(torch, n - 1, ept), "%s w32 ept = %d, offset" % (P, ept))
    elif F.N <= 14:
        for n in (1, 511, 512, 513, 1029):                       # the element-major entry: chunks of 512, the last one short
            u, v, s = _batch(torch, P, wl, n, 70 + n), _batch(torch, P, wl, n, 71 + n), _sels(torch, n, n)
            want = _select_calls(F, u.clone(), v.clone(), s.clone())
            room = torch.full((n + 2,), -7, dtype=torch.int32, device="cuda")
            got = f.aos(F.to_aos(u), F.to_aos(v), s, out=[torch.empty((n, F.N), dtype=u.dtype, device="cuda") for _ in range(3)] + [room[1:n + 1]])
            assert torch.equal(got[3], want[3]) and room[0].item() == -7 and room[n + 1].item() == -7, (P, n)
            for k in (0, 1, 2):
                assert torch.equal(got[k], F.to_aos(want[k])), (P, n, k)
            assert torch.equal(f.aos(F.to_aos(u), F.to_aos(v), s)[3], want[3])
    u, v, s = _batch(torch, P, wl, 8, 81), _batch(torch, P, wl, 8, 82), _sels(torch, 8, 83)
    with pytest.raises(ValueError, match="3 outputs followed by 1 int32 outputs"):
        f(u, v, s, out=[torch.empty_like(u)] * 3)
    for bad in (torch.empty(8, dtype=torch.int64, device="cuda"), torch.empty(9, dtype=torch.int32, device="cuda"), torch.empty(8, dtype=torch.int32),
                torch.empty(16, dtype=torch.int32, device="cuda")[::2]):
        with pytest.raises(ValueError, match="int outputs are contiguous int32"):
            f(u, v, s, out=[torch.empty_like(u) for _ in range(3)] + [bad])


def test_progenitor_passed_to_modqr_modsqrt_modinv(torch_cuda, ctx):
    torch = torch_cuda
    P, wl, F = ctx
    fh, f0 = _built(P, wl, "prog_h", PROG_H), _built(P, wl, "prog_0", PROG_0)
    assert fh.chain.source().count("F::modpro(") == 1 and "nullptr" not in fh.chain.source() and f0.chain.source().count("nullptr") == 3
    a = _dev(torch, wl, _rows(P, wl, _pool_values(P, wl)) + _elements(P, wl, 79, 900), width=132)
    h = F.modpro(a)
    want = [F.modsqrt(a, h), F.modinv(a, h), F.modqr(h, a)]
    got = fh(a)
    _same(torch, F, got, want, "%s w%d progenitor" % (P, wl))
    _same(torch, F, f0(a), got, "%s w%d h = None" % (P, wl))
    _same(torch, F, f0(a), [F.modsqrt(a), F.modinv(a), F.modqr(None, a)], "%s w%d Field without h" % (P, wl))
    assert _both(got[2])


@pytest.mark.parametrize("P", ["X25519", "NIST256", "X448"])
def test_out_of_contract_lanes_decide_as_the_call_sequence_does(torch_cuda, P):
    """64 bits.  Limbs up to 2^64 - 1 in some lanes, and in the shared operand: the waves that hold them run the exact products, and
    the predicates and the words they select are those of the call-by-call sequence, which takes the same vote"""
    torch = torch_cuda
    from modarith_amd.field import Field
    F, wl = Field(P, tile=None), 64
    f = _built(P, wl, "wild", WILD)
    rng = random.Random(1900 + F.N)
    n = 1 << 13
    rows = _rows(P, wl, _pool_values(P, wl)[:12]) + _elements(P, wl, n - 12, 1901)
    for j in list(range(0, n, 997)) + list(range(4096, 4096 + 256)):
        rows[j] = [rng.randrange(0, 1 << 64) for _ in range(F.N)]
    rows[1000] = [(1 << 64) - 1] * F.N
    u, s = _dev(torch, wl, rows), _sels(torch, n, 1902)
    tame, = _elements(P, wl, 1, 1903)
    wild = [(1 << 63) + rng.randrange(0, 1 << 63) for _ in range(F.N)]
    wild[0] = (1 << 64) - 1
    for c, what in ((tame, "wild lanes"), (wild, "wild shared operand"), (rows[3], "shared operand equal to an element")):
        cb = _bcast(torch, wl, c, u)
        want = _wild_calls(F, u.clone(), cb, s.clone())
        _same(torch, F, f(u, c, s), want, "%s %s" % (P, what))
    m = 513
    got = f.aos(F.to_aos(u[:, :m].contiguous()), wild, s[:m].contiguous())
    want = _wild_calls(F, u[:, :m].contiguous(), _bcast(torch, wl, wild, u[:, :m].contiguous()), s[:m].contiguous())
    assert torch.equal(got[2], want[2]) and all(torch.equal(got[k], F.to_aos(want[k])) for k in (0, 1))


def _curve_points(torch, name, sign=False):
    """the points of the curve's reference records that are not the neutral element, as big-endian coordinates (x, y uint8 [n, Nbytes])
    and, where asked for, the sign of x as the curve's get() returns it beside y alone"""
    from modarith_amd.edwards import Curve
    from tests.test_gpu_curveref import batch
    g = load_golden("curveref_%s.json" % name)
    W = Curve(name)
    pts = batch(torch, [r[k] for r in g["records"] for k in ("P", "M", "D", "A", "S", "N", "C", "R", "A+A")] + [g["gen"]])
    keep = W.isinf(pts) == 0
    pts = pts[:, :, keep].contiguous()
    sx = W.get(pts.clone(), want_x=False)[2] if sign else None
    x, y, _ = W.get(pts)
    assert x.shape[0] >= 60
    return x, y, sx


@pytest.mark.parametrize("wl", [64, 32])
def test_predicate_only_chain_is_this_point_on_the_curve(torch_cuda, wl):
    """P-256: modcmp(y^2, x^3 - 3x + b), b shared, four bytes per element out and no limb array.  The points of the reference's records
    are on the curve; with a coordinate perturbed they are not"""
    torch = torch_cuda
    from modarith_amd.field import Field
    from modarith_amd.fuse import oncurve_chain
    ch, (b,) = oncurve_chain("NIST256", wl, name="oncurve_pr")
    f = ch.build(plugin_dir=_plugin_dir())
    assert (len(ch.outs), len(ch.pouts)) == (0, 1) and "NOUT = 0" in ch.source() and ch.traffic_bytes() == 2 * (wl // 8) * ch.params.nlimbs + 4
    F = Field("NIST256", wl=wl, tile=None)
    xb, yb, _ = _curve_points(torch, "NIST256")
    k = xb.shape[0]
    bad_y, bad_x = yb.clone(), xb.clone()
    bad_y[:, -1] ^= 1
    bad_x[:, 7] ^= 0x40
    x = F.modimp(torch.cat([xb, xb, bad_x]).contiguous())[0]
    y = F.modimp(torch.cat([yb, bad_y, yb]).contiguous())[0]
    bb = _bcast(torch, wl, b, x)
    want = F.modcmp(F.modsqr(y), F.modadd(F.modsub(F.modmul(F.modsqr(x), x), F.modmli(x, 3)), bb))
    ok, = f(x, y, b)
    assert ok.dtype == torch.int32 and torch.equal(ok, want)
    assert ok.tolist() == [1] * k + [0] * (2 * k)
    n = 384                                                      # tiles, and the result in the caller's array
    xs, ys = (F.to_tiled(t[:, :n].contiguous(), 128) for t in (x.repeat(1, 3), y.repeat(1, 3)))
    mine = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    assert f(xs, ys, b, out=[mine])[0] is mine and torch.equal(mine, want.repeat(3)[:n])
    if wl == 64:
        assert torch.equal(f.aos(F.to_aos(x), F.to_aos(y), b)[0], want)


def _decompress_calls(F, y, db, s):
    """edwards.c:290-334 call by call, the early return of its modqr failure as the overwrite the chain makes of it"""
    n = F._chk(y)
    one = F.modone(n)
    Y = F.modsqr(y)
    U = F.modsub(one, Y)
    V = F.modsub(F.modneg(one), F.modmul(Y, db))
    O = F.modsqr(U)
    W = F.modmul(F.modmul(U, O), V)
    H = F.modpro(W)
    ok = F.modqr(H, W)
    R = F.modsqrt(W, H)
    X = F.modmul(F.modmul(F.modinv(W, H), R), O)
    X = F.modcmv(F.modsign(X) ^ s, F.modneg(X), X.clone())
    bad = 1 - ok
    return [F.modcmv(bad, F.modzer(n), X), F.modcmv(bad, one, y.clone()), one.clone(), ok]


@pytest.mark.parametrize("wl", [64, 32])
def test_decompression_of_ed25519_points_as_one_chain(torch_cuda, wl):
    """ecnXXXset from y and the sign of x (edwards.c:290-334) over X25519 as ONE chain: compressed points of the reference's records,
    the same with the sign flipped, and y values that have no x.  Word for word the same calls through Field; by value Curve.set
    (whose modinv is not the normalised one: compared as exported bytes)"""
    torch = torch_cuda
    from modarith_amd.edwards import Curve
    from modarith_amd.field import Field
    from modarith_amd.fuse import decompress_chain
    ch, (d,) = decompress_chain("ED25519", wl, name="decompress_pr")
    f = ch.build(plugin_dir=_plugin_dir())
    F = Field("X25519", wl=wl, tile=None)
    _, yb, sx = _curve_points(torch, "ED25519", sign=True)
    k = yb.shape[0]
    p, dd = (1 << 255) - 19, 0x52036CEE2B6FFE738CC740797779E89800700A4D4141D8AB75EB4DCA135978A3
    has_x = lambda v: pow((1 - v * v) * (-1 - dd * v * v), (p - 1) // 2, p) in (0, 1)          # U V is a square exactly where U^3 V is
    lone = [v for v in range(2, 200) if not has_x(v)][:24] + [p - 3, p - 5]
    lone = [v for v in lone if not has_x(v)]
    assert len(lone) >= 24
    extra = torch.tensor([list(v.to_bytes(32, "big")) for v in lone + [0, p - 1]], dtype=torch.uint8, device="cuda")
    ybytes = torch.cat([yb, yb, extra]).contiguous()
    s = torch.cat([sx, 1 - sx, _sels(torch, extra.shape[0], 7)]).to(torch.int32).contiguous()
    y = F.modimp(ybytes)[0]
    n = y.shape[1]
    want = _decompress_calls(F, y, _bcast(torch, wl, d, y), s)
    got = f(y, d, s)
    _same(torch, F, got, want, "decompression w%d" % wl)
    E = Curve("ED25519", wl=wl)
    Pt = E.set(s, None, ybytes)
    ok = got[3]
    assert torch.equal(ok, 1 - E.isinf(Pt)) and ok.tolist() == [1] * (2 * k) + [0] * len(lone) + [1, 1]              # (y = 0 and y = -1 have an x; y = 1 is the neutral element itself: left out)
    for c in range(3):
        assert torch.equal(F.modexp(got[c]), F.modexp(Pt[c].contiguous())), "coordinate %d against Curve.set" % c
    # both signs of one y are the two points (x, y), (-x, y); the recovered x of a record has the record's sign
    assert torch.equal(F.modsign(got[0])[:k], sx) and torch.equal(F.modsign(got[0])[k:2 * k], 1 - sx)
    m = n // 128 * 128
    if m:
        tiled = f(F.to_tiled(y[:, :m].contiguous(), 128), d, s[:m].contiguous())
        _same(torch, F, tiled, [w[..., :m].contiguous() for w in want], "decompression w%d, tiles" % wl)
