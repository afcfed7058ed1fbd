"""Fused chains with little-endian records, sign bits, the shifts and modfsb on the GPU, at both word lengths and through both ways to the
bytes of csrc/chain.inc (MA_CHAIN_BYTES=staged|direct).  Equality is exact everywhere.  The truth is the call-by-call sequence of
Field(P, wl) on the same device with the byte handling done in torch -- torch.flip(rec, [1]) for the byte order, masking and shifting
the top byte for the sign --; Field's own modimp / modexp / modshl / modshr / mod2r / modfsb are pinned to the reference by the golden
tests (tests/test_gpu_parity.py, tests/test_gpu_w32_parity.py), and the import-only and export-only little-endian chains are compared
with the reference's recorded words directly, the fixture's records flipped.  One pool of 8192 records per field and kind serves every
test of a case: the directed records 0, 1, p - 1, p, p + 1, 2^Nbits - 1, all 0xff first (for chains that take a sign out: each with the
top bit clear and set), then random ones of which every third is in [p, 2p) as far as Nbytes -- less the sign bit -- allow.  The sizes
straddle one workgroup's chunk (256 lanes of 1, 2 or 4 elements): dead lanes, the remainder launch, one partial chunk."""
import concurrent.futures as cf
import os
import random

import numpy as np
import pytest

from tests import w32_inputs as wi
from tests.conftest import limbs, load_golden
from tests.test_gpu_fuse_shared import _dev

pytestmark = pytest.mark.gpu


def _gm240_w32():
    """GM240 at word length 32 is a case where its generated plug-in is there (build() makes it; tests/test_gpu_w32_gen.py too): 30-byte
    records assembled byte by byte through the opaque form of the loaders"""
    from modarith_amd import generate as gen
    return gen.find_field("GM240", wl=32, built=True) is not None


CASES = [(P, wl) for P in ("X25519", "NIST256", "X448") for wl in (64, 32)] + [("NIST521", 64), ("GM240", 64)] + ([("GM240", 32)] if _gm240_w32() else [])
NS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1025)
POOL = 8192
PATHS = ("staged", "direct")
CHAINS = {"limp": "lebytes a; out a, flag(a)",
          "lexp": "in a; outlebytes modcpy(a)",
          "lmul": "lebytes a, b; outlebytes modmul(a, b)",
          "lmuls": "lesbytes a, b; outlesbytes (modmul(a, b), sign(a) ^ sign(b)); out flag(a)",
          "mix": "bytes a; in e; outlebytes modsqr(modadd(a, e))",        # big-endian in, little-endian out, one element batch in
          "bl": "bytes a; lebytes b; outlebytes modmul(a, b)",
          "bsgn": "sbytes a; in e; outsbytes (modsqr(modadd(a, e)), sign(a)); out sign(a), flag(a)",
          "shl": "in a; out modshl(a, 1), modshl(a, {K})",
          "shr": "in a, b; v, r = modshr(a, 1); w, q = modshr(a, {K}); out v, w, modcmv(r, b, a), r, q",
          "m2r": "in a; out mod2r(0), mod2r({R}), mod2r({NB1}), mod2r({B8})",
          "fsb": "in a; v, f = modfsb(a); w, g = flatten(a); out v, w, f, g",
          "b249": "in D, x; one = modone(); d = modadd(D, one); d, f = modfsb(d); d, r = modshr(d, 1); out modmul(x, d)"}      # rfc7748.c:249
WIDE = ("lmul", "lmuls", "mix")                                           # built at every width
B249 = ("X25519", "NIST256")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _widths(wl):
    return (1, 2) if wl == 64 else (1, 2, 4)


def _fp(P, wl):
    from modarith_amd import generate as gen
    return gen.find_field(P, wl=wl, built=True)[0]


def _consts(P, wl):
    fp = _fp(P, wl)
    return {"K": min(fp.radix - 1, 31), "R": fp.radix, "NB1": fp.n - 1, "B8": 8 * fp.nbytes}


_BUILT = {}


def _built(P, wl, name, width=None):
    """one plug-in per (field, word length, chain, width); a plug-in's name does not carry its width: the explicit ones apart"""
    from modarith_amd import generate as gen
    from modarith_amd.fuse import parse
    default = 2 if wl == 64 else 1
    width = width or default
    key = (P, wl, name, width)
    if key not in _BUILT:
        ch = parse(P, name + "_le", CHAINS[name].format(**_consts(P, wl)), wl=wl)
        if width == default:
            _BUILT[key] = ch.build()
        else:
            _BUILT[key] = ch.build(plugin_dir=os.path.join(gen.PLUGIN_DIR, "le_ept%d" % width), ept=width)
    return _BUILT[key]


def _le(torch, values, nb):
    return torch.tensor([list(int(v).to_bytes(nb, "little")) for v in values], dtype=torch.uint8, device="cuda")


def _be(torch, values, nb):
    return torch.tensor([list(int(v).to_bytes(nb, "big")) for v in values], dtype=torch.uint8, device="cuda")


def _pool(fp, seed, signed=False, count=POOL):
    """the integers the records spell (the sign bit included where signed)"""
    p, nb = fp.p, fp.nbytes
    top = 1 << (8 * nb - 1)
    rng = random.Random(seed)
    directed = [0, 1, p - 1, p, p + 1, (1 << fp.n) - 1, (1 << (8 * nb)) - 1]
    if seed % 2:
        directed.reverse()                                      # (the second operand: other pairs)
    cap = top if signed else 2 * top                             # what the value itself may reach
    if signed:
        directed = [d & ~top for d in directed] + [d | top for d in directed]
    rest = [rng.randrange(p, min(2 * p, cap)) if j % 3 == 0 and p < cap else rng.randrange(0, min(p, cap)) for j in range(count - len(directed))]
    if signed:
        rest = [v | (rng.randrange(2) * top) for v in rest]
    return directed + rest


def _split_sign(torch, rec, little=True):
    """(the record with its top bit cleared, that bit as int32): the masking and shifting a caller does today"""
    col = -1 if little else 0
    m = rec.clone()
    m[:, col] &= 0x7f
    return m, (rec[:, col] >> 7).to(torch.int32)


def _with_sign(torch, rec, s, little=True):
    out = rec.clone()
    out[:, -1 if little else 0] |= (s << 7).to(torch.uint8)
    return out


def _elements(P, wl, n, seed):
    """rows of unsigned limbs inside the limb contract: 64 bits -- every limb uniform below 2^Radix, the top limb spanning what is left of
    Nbits; 32 bits -- values below 2p, as the field functions return them"""
    fp = _fp(P, wl)
    if wl == 64:
        rng = np.random.default_rng(seed)
        out = rng.integers(0, 1 << fp.radix, size=(n, fp.nlimbs), dtype=np.uint64)
        out[:, fp.nlimbs - 1] = rng.integers(0, 1 << (fp.n - fp.radix * (fp.nlimbs - 1)), size=n, dtype=np.uint64)
        return [[int(v) for v in r] for r in out]
    rng = random.Random(seed)
    return [fp.to_limbs(rng.randrange(0, 2 * fp.p)) for _ in range(n)]


class Case:
    pass


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-w%d" % c)
def ctx(request, torch_cuda):
    from modarith_amd.field import Field
    torch = torch_cuda
    P, wl = request.param
    names = [name for name in CHAINS if name != "b249" or P in B249]
    units = [(name, None) for name in names] + [(name, w) for name in WIDE for w in _widths(wl)]
    with cf.ThreadPoolExecutor(max_workers=8) as ex:             # independent hipcc units, seconds each: side by side
        for j in [ex.submit(_built, P, wl, name, w) for name, w in units]:
            j.result()
    os.environ.pop("MA_CHAIN_BYTES", None)
    c = Case()
    c.P, c.wl, c.F, c.fp = P, wl, Field(P, wl=wl, tile=None), _fp(P, wl)
    F, fp, nb = c.F, c.fp, c.fp.nbytes
    flip = lambda t: torch.flip(t, [1]).contiguous()
    # without a sign: the truth, once, call by call through Field
    c.va, c.vb = _pool(fp, 10), _pool(fp, 11)
    c.A, c.B = _le(torch, c.va, nb), _le(torch, c.vb, nb)
    c.Abe = flip(c.A)
    c.e = _dev(torch, wl, _elements(P, wl, POOL, 12))
    a, c.fa = F.modimp(c.Abe)
    b, c.fb = F.modimp(flip(c.B))
    for f in (c.fa, c.fb):
        assert 0 < int(f.sum()) < POOL                           # flags of both values
    c.lmul = flip(F.modexp(F.modmul(a, b)))
    c.mix = flip(F.modexp(F.modsqr(F.modadd(a, c.e))))
    # with a sign
    c.vsa, c.vsb = _pool(fp, 20, signed=True), _pool(fp, 21, signed=True)
    c.SA, c.SB = _le(torch, c.vsa, nb), _le(torch, c.vsb, nb)
    (ma, sa), (mb, sb) = _split_sign(torch, c.SA), _split_sign(torch, c.SB)
    top = 1 << (8 * nb - 1)
    assert sa.cpu().tolist() == [int(v >= top) for v in c.vsa]
    rnd = sa[14:]
    assert 0.45 * rnd.numel() < int(rnd.sum()) < 0.55 * rnd.numel() and int(sa[:7].sum()) == 0 and int(sa[7:14].sum()) == 7
    x, c.fsa = F.modimp(flip(ma))
    y, _ = F.modimp(flip(mb))
    if fp.p < top:                                               # values of p and above fit below the sign: the directed records exercise flag 0
        assert int((c.fsa == 0).sum()) >= 3
    else:
        assert int((c.fsa == 0).sum()) == 0
    c.sa = sa
    c.lmuls = _with_sign(torch, flip(F.modexp(F.modmul(x, y))), sa ^ sb)
    # a sign in a big-endian record: the top bit of byte 0
    c.SAbe = flip(c.SA)
    c.bsgn = _with_sign(torch, F.modexp(F.modsqr(F.modadd(x, c.e))), sa, little=False)
    return c


# ---------------------------------------------------------------------------------------------------------------- the reference's words
@pytest.mark.parametrize("path", PATHS)
def test_goldens(ctx, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c, F = ctx, ctx.F
    if c.P == "GM240" and c.wl == 32:
        return                                                   # (a generated field: its fixture records no byte records of this shape)
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    fimp, fexp = _built(c.P, c.wl, "limp"), _built(c.P, c.wl, "lexp")
    if c.wl == 64:
        recs = load_golden("field_%s.json" % c.P)["ops"]["bytes"]
        rb, want_l, want_f, want_b = [r["bytes"] for r in recs], [limbs(r["imp"]) for r in recs], [r["imp_ret"] for r in recs], [r["exp"] for r in recs]
        src_l = want_l
    else:
        fx = load_golden("field_w32_%s.json" % c.P)
        pool = [wi.unpack(s) for s in fx["pool"]]
        imp, exp = fx["records"]["modimp"], fx["records"]["modexp"]
        rb, want_l, want_f = [r[0] for r in imp], [wi.unpack(r[1]) for r in imp], [r[2] for r in imp]
        src_l, want_b = [pool[r[0]] for r in exp], [r[1] for r in exp]
    b = torch.tensor([list(bytes.fromhex(r))[::-1] for r in rb], dtype=torch.uint8, device="cuda")
    v, ok = fimp(b)
    assert F.to_limbs(v) == [list(r) for r in want_l] and ok.cpu().tolist() == want_f and 0 in want_f and 1 in want_f
    out, = fexp(_dev(torch, c.wl, src_l))
    assert [bytes(row)[::-1].hex() for row in out.cpu().numpy()] == want_b


# ---------------------------------------------------------------------------------------------------------------- values and shapes
def _flat(c, n):
    return c.e[:, :n].contiguous()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("width", (1, 2, 4))
def test_values_and_shapes(ctx, torch_cuda, monkeypatch, path, width):
    torch = torch_cuda
    c, F = ctx, ctx.F
    if width not in _widths(c.wl):
        return                                                   # (four elements per lane: 32-bit limbs only)
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    fmul, fsgn, fmix = (_built(c.P, c.wl, name, width) for name in WIDE)
    for n in NS:
        got, = fmul(c.A[:n], c.B[:n])
        assert torch.equal(got, c.lmul[:n]), ("lmul", n)
        got, flag = fsgn(c.SA[:n], c.SB[:n])
        assert torch.equal(got, c.lmuls[:n]) and torch.equal(flag, c.fsa[:n]), ("lmuls", n)
        got, = fmix(_flat(c, n), c.Abe[:n])
        assert torch.equal(got, c.mix[:n]), ("mix", n)
    for n, tile in ((8192, 4096), (640, 128)):                   # tiled element batches beside records that have no layout
        got, = fmix(F.to_tiled(_flat(c, n), tile), c.Abe[:n])
        assert torch.equal(got, c.mix[:n]), ("mix tiled", n, tile)
    got, = fmul(c.A, c.B)
    assert torch.equal(got, c.lmul)
    got, flag = fsgn(c.SA, c.SB)
    assert torch.equal(got, c.lmuls) and torch.equal(flag, c.fsa)


@pytest.mark.parametrize("path", PATHS)
def test_sign_of_a_big_endian_record(ctx, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c = ctx
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    f = _built(c.P, c.wl, "bsgn")
    for n in (3, 257, POOL):
        got, s, flag = f(_flat(c, n), c.SAbe[:n])
        assert torch.equal(got, c.bsgn[:n]) and torch.equal(s, c.sa[:n]) and torch.equal(flag, c.fsa[:n]), n


# ---------------------------------------------------------------------------------------------------------------- addresses
def _at(torch, t, off):
    """a copy of the record tensor t that starts `off` bytes behind a 16-byte aligned address"""
    buf = torch.empty(t.numel() + 32, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


@pytest.mark.parametrize("path", PATHS)
def test_alignment(ctx, torch_cuda, monkeypatch, path):
    from modarith_amd._lib import DeviceError
    torch = torch_cuda
    c = ctx
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    f = _built(c.P, c.wl, "lmul")
    n = 513
    out1 = _at(torch, torch.full_like(c.A[:n], 0x5a), 1)
    if c.fp.nbytes % 8 == 0:
        out8 = _at(torch, torch.zeros_like(c.A[:n]), 8)
        f(_at(torch, c.A[:n], 8), _at(torch, c.B[:n], 8), out=[out8])           # 8 but not 16: the direct path whatever was asked for
        assert torch.equal(out8, c.lmul[:n])
        got, = f(_at(torch, c.A[:n], 8), c.B[:n])
        assert torch.equal(got, c.lmul[:n])
        for args, out in (((_at(torch, c.A[:n], 1), c.B[:n]), None), ((c.A[:n], c.B[:n]), [out1])):
            with pytest.raises(DeviceError, match="byte records must be 8-byte aligned"):
                f(*args, out=out)
        torch.cuda.synchronize()
        assert bool((out1 == 0x5a).all())                        # nothing was written
    else:
        f(_at(torch, c.A[:n], 1), _at(torch, c.B[:n], 3), out=[out1])        # records of 66 and 30 bytes may be anywhere
        assert torch.equal(out1, c.lmul[:n])


@pytest.mark.parametrize("path", PATHS)
def test_output_on_its_input(ctx, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c = ctx
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    for width in _widths(c.wl):
        f = _built(c.P, c.wl, "lmul", width)
        for n in (513, POOL):
            a = c.A[:n].clone()
            got, = f(a, c.B[:n], out=[a])
            assert got is a and torch.equal(a, c.lmul[:n]), (width, n)
    f = _built(c.P, c.wl, "bl")                                  # a little-endian output on the array of a big-endian input
    for n in (513, POOL):
        want, = f(c.Abe[:n], c.B[:n])
        assert torch.equal(want, c.lmul[:n])
        a = c.Abe[:n].clone()
        got, = f(a, c.B[:n], out=[a])
        assert got is a and torch.equal(a, want), n


# ---------------------------------------------------------------------------------------------------------------- the rest of field.c
def _inputs(c, torch, n, seed, wild=True):
    """a flat batch: elements inside the limb contract, a stretch of the field's own plus_p elements (values in [p, 2p), the top limb
    unmasked) and, at word length 64, lanes of fabricated limbs up to 2^64 - 1 (tests/test_gpu_fuse.py::test_out_of_contract_limbs_take_the_exact_products)"""
    x = _dev(torch, c.wl, _elements(c.P, c.wl, n, seed))
    if not wild:
        return x
    k = n // 3
    x[:, k:2 * k] = c.F.uniform(k, seed=seed, plus_p=True)
    if c.wl == 64:
        rng = np.random.default_rng(seed)
        for j in list(range(0, n, 97)) + list(range(256, min(n, 320))):
            x[:, j] = torch.from_numpy(rng.integers(0, 1 << 64, size=c.fp.nlimbs, dtype=np.uint64).view(np.int64)).cuda()
    return x


def _eq(torch, F, got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and torch.equal(F.to_flat(g) if g.dim() > 1 else g, F.to_flat(w) if w.dim() > 1 else w), (what, k)


def test_shifts(ctx, torch_cuda):
    torch = torch_cuda
    c, F = ctx, ctx.F
    K = _consts(c.P, c.wl)["K"]
    n = 1025
    a, b = _inputs(c, torch, n, 31), _inputs(c, torch, n, 32)
    for m in (1, 257, n):
        x, y = a[:, :m].contiguous(), b[:, :m].contiguous()
        _eq(torch, F, _built(c.P, c.wl, "shl")(x), [F.modshl(1, x.clone()), F.modshl(K, x.clone())], ("modshl", m))
        v, w, f = x.clone(), x.clone(), x.clone()
        r, q = F.modshr(1, v), F.modshr(K, w)
        assert set(r.cpu().tolist()) <= {0, 1}
        F.modcmv(r, y, f)
        _eq(torch, F, _built(c.P, c.wl, "shr")(x, y), [v, w, f, r, q], ("modshr", m))
    assert 0 < int(r.sum()) < n and int(q.max()) > 1


def test_constants_and_modfsb(ctx, torch_cuda):
    torch = torch_cuda
    c, F = ctx, ctx.F
    k = _consts(c.P, c.wl)
    n = 513
    got = _built(c.P, c.wl, "m2r")(_inputs(c, torch, n, 33, wild=False))
    _eq(torch, F, got, [F.mod2r(r, n) for r in (0, k["R"], k["NB1"], k["B8"])], "mod2r")
    assert not bool(got[3].any())                                # 2^(8 Nbytes) is zero, as field.c has it
    a = _inputs(c, torch, 1025, 34)
    for m in (1, 257, 1025):
        x = a[:, :m].contiguous()
        v, w = x.clone(), x.clone()
        f, g = F.modfsb(v), F.flatten(w)
        _eq(torch, F, _built(c.P, c.wl, "fsb")(x), [v, w, f, g], ("modfsb", m))
    assert 0 < int(f.sum()) < 1025


def test_the_body_of_rfc7748_249(ctx, torch_cuda):
    torch = torch_cuda
    c, F = ctx, ctx.F
    if c.P not in B249:
        return
    n = 1025
    D, x = _inputs(c, torch, n, 35, wild=False), _inputs(c, torch, n, 36, wild=False)
    d = F.modadd(D, F.modone(n))
    F.modfsb(d)
    F.modshr(1, d)
    for m in (1, 257, n):
        got, = _built(c.P, c.wl, "b249")(D[:, :m].contiguous(), x[:, :m].contiguous())
        assert torch.equal(got, F.modmul(x, d)[:, :m]), m


# ---------------------------------------------------------------------------------------------------------------- the chains the library carries
VALID = 512
LIB_POOL = 1536                                                  # 14 directed records, random ones, the valid points: a multiple of the smallest tile


@pytest.fixture(scope="module", params=(64, 32), ids=lambda wl: "w%d" % wl)
def ed(request, torch_cuda):
    from modarith_amd import generate as gen
    from modarith_amd.edwards import Curve
    from modarith_amd.field import Field
    from modarith_amd.fuse import decompress_chain, edwards_to_montgomery_chain, rfc8032_decode_chain, rfc8032_encode_chain
    torch = torch_cuda
    wl = request.param
    c = Case()
    c.wl, c.F, c.fp = wl, Field("X25519", wl=wl, tile=None), _fp("X25519", wl)
    dec, (c.d,) = rfc8032_decode_chain("ED25519", wl, name="rfc8032_decode_le")
    dc, (d2,) = decompress_chain("ED25519", wl, name="decompress_le")
    assert d2 == c.d
    chains = [dec, dc, rfc8032_encode_chain("ED25519", wl, name="rfc8032_encode_le"), edwards_to_montgomery_chain("ED25519", wl, name="ed_to_mont_le")]
    with cf.ThreadPoolExecutor(max_workers=4) as ex:
        c.dec, c.dc, c.enc, c.e2m = [j.result() for j in [ex.submit(ch.build) for ch in chains]]
    os.environ.pop("MA_CHAIN_BYTES", None)
    # k G for k = 1 .. VALID: affine coordinates as the curve layer exports them
    E = Curve("ED25519")
    c.xb, c.yb, _ = E.mulgen_get(_be(torch, range(1, VALID + 1), 32))
    c.sx = (c.xb[:, -1] & 1).to(torch.int32)                     # RFC 8032's x_0: the least significant bit of x
    flip = lambda t: torch.flip(t, [1]).contiguous()
    c.valid = _with_sign(torch, flip(c.yb), c.sx)
    c.recs = torch.cat([_le(torch, _pool(c.fp, 40, signed=True, count=LIB_POOL - VALID), 32), c.valid]).contiguous()
    assert c.recs.shape == (LIB_POOL, 32)
    c.masked, c.s = _split_sign(torch, c.recs)
    c.y, c.fy = c.F.modimp(flip(c.masked))
    return c


def _tiled_like(torch, F, n, tile):
    return torch.empty((n // tile, F.N, tile), dtype=F.dtype, device="cuda")


@pytest.mark.parametrize("path", PATHS)
def test_rfc8032_decode(ed, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c, F, n = ed, ed.F, LIB_POOL
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    X, Y, Z, ok = c.dc(c.y, c.d, c.s)
    bad = 1 - c.fy                                               # y not below p: no point, whatever y - p would give
    F.modcmv(bad, F.modzer(n), X)
    F.modcmv(bad, F.modone(n), Y)
    want = [X, Y, Z, ok & c.fy]
    good = int(want[3].sum())
    assert 4 * good >= n and 4 * (n - good) >= n and int(bad.sum()) >= 3 and bool(want[3][-VALID:].all())
    _eq(torch, F, c.dec(c.recs, c.d), want, "decode")
    for m in (1, 257):
        _eq(torch, F, c.dec(c.recs[:m], c.d), [w[..., :m].contiguous() for w in want], ("decode", m))
    out = [_tiled_like(torch, F, n, 128) for _ in range(3)] + [torch.empty(n, dtype=torch.int32, device="cuda")]
    _eq(torch, F, c.dec(c.recs, c.d, out=out), want, "decode, tiles")
    # a record with no point behind it is the neutral element
    one, lost = F.redc(F.modone(n)), want[3] == 0
    assert not bool(F.redc(want[0])[:, lost].any()) and torch.equal(F.redc(want[1])[:, lost], one[:, lost]) and torch.equal(F.redc(want[2]), one)


@pytest.mark.parametrize("path", PATHS)
def test_rfc8032_encode(ed, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c, F = ed, ed.F
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    x, y = F.modimp(c.xb)[0], F.modimp(c.yb)[0]
    want = _with_sign(torch, torch.flip(F.modexp(y), [1]).contiguous(), F.modsign(x))
    assert torch.equal(want, c.valid) and 0 < int(F.modsign(x).sum()) < VALID
    got, = c.enc(x, y)
    assert torch.equal(got, want)
    assert bytes(got[0].cpu().numpy()).hex() == "5866666666666666666666666666666666666666666666666666666666666666"
    for m in (1, 257):
        got, = c.enc(x[:, :m].contiguous(), y[:, :m].contiguous())
        assert torch.equal(got, want[:m]), m
    got, = c.enc(F.to_tiled(x, 128), F.to_tiled(y, 128))
    assert torch.equal(got, want)
    # decode after encode: the affine point again
    X, Y, Z, ok = c.dec(got, c.d)
    assert bool(ok.all()) and torch.equal(F.redc(X), F.redc(x)) and torch.equal(F.redc(Y), F.redc(y)) and torch.equal(F.redc(Z), F.redc(F.modone(VALID)))


@pytest.mark.parametrize("path", PATHS)
def test_edwards_to_montgomery(ed, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c, F, n = ed, ed.F, LIB_POOL
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    one = F.modone(n)
    u = F.modmul(F.modadd(one, c.y), F.modinv(F.modsub(one, c.y)))
    want = torch.flip(F.modexp(u), [1]).contiguous()
    got, ok = c.e2m(c.recs)
    assert torch.equal(got, want) and torch.equal(ok, c.fy)
    for m in (1, 257):
        got, ok = c.e2m(c.recs[:m])
        assert torch.equal(got, want[:m]) and torch.equal(ok, c.fy[:m]), m
    assert bytes(want[LIB_POOL - VALID].cpu().numpy()).hex() == "09" + "00" * 31               # the base point: u = 9
    ones = [j for j in range(14) if bytes(c.masked[j].cpu().numpy()) == bytes([1] + [0] * 31)]
    assert len(ones) == 2 and all(not bool(want[j].any()) for j in ones)                        # y = 1: modinv of 0 is 0
