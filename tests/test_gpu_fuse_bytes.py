"""Fused chains that speak bytes (Chain.input_bytes / Chain.output_bytes: modimp and modexp inside the kernel) on the GPU, at both word
lengths and through both ways to the bytes of csrc/chain.inc (MA_CHAIN_BYTES=staged|direct).  Equality is exact everywhere.  The truth
is the call-by-call sequence of Field(P, wl) -- modimp, the field calls, modexp -- on the same device; Field's own modimp / modexp are
pinned to the reference by tests/test_gpu_parity.py::test_golden_bytes and tests/test_gpu_w32_parity.py, and the import-only and
export-only chains are compared with the reference's recorded words directly.  One pool of 8192 records per field serves every test of
a case: 0, 1, p - 1, p, p + 1, 2^Nbits - 1, all 0xff first, then random values of which every third is in [p, 2p) (as far as Nbytes go), so that
lanes whose flag is 0 sit in the waves of lanes whose flag is 1.  The sizes straddle one workgroup's chunk (256 lanes of 1, 2 or 4
elements): dead lanes, the remainder launch, one partial chunk."""
import concurrent.futures as cf
import os
import random

import pytest

from tests import w32_inputs as wi
from tests.conftest import limbs, load_golden
from tests.test_gpu_fuse_shared import _batch, _dev
from tests.util import derive_any

pytestmark = pytest.mark.gpu
CASES = [(P, wl) for P in ("X25519", "NIST256", "X448") for wl in (64, 32)] + [("NIST521", 64), ("GM240", 64)]
NS = (1, 2, 3, 255, 256, 257, 511, 512, 513, 1025)
POOL = 8192
PATHS = ("staged", "direct")
CHAINS = {"imp": "bytes a; out a, flag(a)",
          "exp": "in a; outbytes modcpy(a)",
          "mul": "bytes a, b; outbytes modmul(a, b)",                     # no element array on either side
          "sqe": "bytes a; in e; outbytes modsqr(modadd(a, e))",
          "steer": "bytes a; outbytes modcmv(not flag(a), modzer(), a); out flag(a)"}
WIDE = ("mul", "sqe")                                                     # built at every width


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _widths(wl):
    return (1, 2) if wl == 64 else (1, 2, 4)


_BUILT = {}


def _built(P, wl, name, width=None):
    """one plug-in per (field, word length, chain, width); a plug-in's name does not carry its width: the explicit ones apart"""
    from modarith_amd import generate as gen
    from modarith_amd.fuse import parse
    default = 2 if wl == 64 else 1
    width = width or default
    key = (P, wl, name, width)
    if key not in _BUILT:
        ch = parse(P, name + "_by", CHAINS[name], wl=wl)
        if width == default:
            _BUILT[key] = ch.build()
        else:
            _BUILT[key] = ch.build(plugin_dir=os.path.join(gen.PLUGIN_DIR, "bytes_ept%d" % width), ept=width)
    return _BUILT[key]


def _fp(P, wl):
    from modarith_amd.params import derive
    return derive_any(P) if wl == 64 else derive(P, wl=32)


def _records(torch, values, nb):
    return torch.tensor([list(int(v).to_bytes(nb, "big")) for v in values], dtype=torch.uint8, device="cuda")


def _pool(P, wl, seed):
    fp = _fp(P, wl)
    p, nb = fp.p, fp.nbytes
    rng = random.Random(seed)
    directed = [0, 1, p - 1, p, p + 1, (1 << fp.n) - 1, (1 << (8 * nb)) - 1]
    if seed % 2:
        directed.reverse()                                      # (the second operand: other pairs)
    rest = [rng.randrange(p, min(2 * p, 1 << (8 * nb))) if j % 3 == 0 else rng.randrange(0, p) for j in range(POOL - len(directed))]
    return directed + rest


class Case:
    pass


@pytest.fixture(scope="module", params=CASES, ids=lambda c: "%s-w%d" % c)
def ctx(request, torch_cuda):
    from modarith_amd.field import Field
    torch = torch_cuda
    P, wl = request.param
    units = [(name, None) for name in CHAINS] + [(name, w) for name in WIDE for w in _widths(wl)]
    with cf.ThreadPoolExecutor(max_workers=8) as ex:             # independent hipcc units, seconds each: side by side
        for j in [ex.submit(_built, P, wl, name, w) for name, w in units]:
            j.result()
    os.environ.pop("MA_CHAIN_BYTES", None)
    c = Case()
    c.P, c.wl, c.F = P, wl, Field(P, wl=wl, tile=None)
    F, nb = c.F, c.F.nbytes
    c.va, c.vb = _pool(P, wl, 10), _pool(P, wl, 11)
    c.A, c.B = _records(torch, c.va, nb), _records(torch, c.vb, nb)
    c.e = _batch(torch, P, wl, POOL, 12)
    # the truth, once: call by call through Field
    a, c.fa = F.modimp(c.A)
    b, _ = F.modimp(c.B)
    p = _fp(P, wl).p
    # (modfsb decides by one subtraction of p: its answer is `below p` for every integer below 2p, and the reference's own beyond)
    assert all(f == int(v < p) for f, v in zip(c.fa.cpu().tolist(), c.va) if v < 2 * p) and 4 * int((c.fa == 0).sum()) >= POOL
    c.mul = F.modexp(F.modmul(a, b))
    c.sqe = F.modexp(F.modsqr(F.modadd(a, c.e)))
    steered = a.clone()
    F.modcmv(1 - c.fa, F.modzer(POOL), steered)
    c.steer = F.modexp(steered)
    return c


# ---------------------------------------------------------------------------------------------------------------- the reference's words
@pytest.mark.parametrize("path", PATHS)
def test_goldens(ctx, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c, F = ctx, ctx.F
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    fimp, fexp = _built(c.P, c.wl, "imp"), _built(c.P, c.wl, "exp")
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
    b = torch.tensor([list(bytes.fromhex(r)) for r in rb], dtype=torch.uint8, device="cuda")
    v, ok = fimp(b)
    assert F.to_limbs(v) == [list(r) for r in want_l] and ok.cpu().tolist() == want_f and 0 in want_f and 1 in want_f
    out, = fexp(_dev(torch, c.wl, src_l))
    assert [bytes(row).hex() for row in out.cpu().numpy()] == want_b


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
    fmul, fsqe = _built(c.P, c.wl, "mul", width), _built(c.P, c.wl, "sqe", width)
    for n in NS:
        got, = fmul(c.A[:n], c.B[:n])
        assert torch.equal(got, c.mul[:n]), ("mul", n)
        got, = fsqe(_flat(c, n), c.A[:n])
        assert torch.equal(got, c.sqe[:n]), ("sqe", n)
    for n, tile in ((8192, 4096), (640, 128)):                   # tiled element batches beside records that have no layout
        got, = fsqe(F.to_tiled(_flat(c, n), tile), c.A[:n])
        assert torch.equal(got, c.sqe[:n]), ("sqe tiled", n, tile)
    got, = fmul(c.A, c.B)
    assert torch.equal(got, c.mul)


@pytest.mark.parametrize("wl", (64, 32))
def test_second_chunk_in_one_workgroup(torch_cuda, monkeypatch, wl):
    """more elements than the grid of a flat batch covers in one sweep (4096 workgroups): every workgroup of the staged kernel goes
    round its loop again, through the barriers inside it; the last round is partial"""
    from modarith_amd.field import Field
    torch = torch_cuda
    n = 2 * 4096 * 256 + 513
    F = Field("X25519", wl=wl, tile=None)
    f = _built("X25519", wl, "mul")
    g = torch.Generator(device="cuda").manual_seed(5)
    A, B = (torch.randint(0, 256, (n, 32), dtype=torch.uint8, device="cuda", generator=g) for _ in range(2))
    (a, fa), (b, _) = F.modimp(A), F.modimp(B)
    assert 0.25 * n < int(fa.sum()) < 0.75 * n                   # the top bit of a record decides, about evenly
    want = F.modexp(F.modmul(a, b))
    for path in PATHS:
        monkeypatch.setenv("MA_CHAIN_BYTES", path)
        got, = f(A, B)
        assert torch.equal(got, want), path


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
    f = _built(c.P, c.wl, "mul")
    n = 513
    out8 = _at(torch, torch.zeros_like(c.A[:n]), 8)
    f(_at(torch, c.A[:n], 8), _at(torch, c.B[:n], 8), out=[out8])           # 8 but not 16: the direct path whatever was asked for
    assert torch.equal(out8, c.mul[:n])
    got, = f(_at(torch, c.A[:n], 8), c.B[:n])
    assert torch.equal(got, c.mul[:n])
    out1 = _at(torch, torch.full_like(c.A[:n], 0x5a), 1)
    if c.F.nbytes % 8 == 0:
        for args, out in (((_at(torch, c.A[:n], 1), c.B[:n]), None), ((c.A[:n], c.B[:n]), [out1])):
            with pytest.raises(DeviceError, match="byte records must be 8-byte aligned"):
                f(*args, out=out)
        torch.cuda.synchronize()
        assert bool((out1 == 0x5a).all())                        # nothing was written
    else:
        f(_at(torch, c.A[:n], 1), _at(torch, c.B[:n], 3), out=[out1])        # records of 66 and 30 bytes may be anywhere
        assert torch.equal(out1, c.mul[:n])


def test_override_is_read_at_every_call(ctx, torch_cuda, monkeypatch):
    from modarith_amd._lib import DeviceError
    c = ctx
    f = _built(c.P, c.wl, "mul")
    monkeypatch.setenv("MA_CHAIN_BYTES", "lds")
    with pytest.raises(DeviceError, match="MA_CHAIN_BYTES is staged or direct"):
        f(c.A[:4], c.B[:4])
    monkeypatch.delenv("MA_CHAIN_BYTES")
    got, = f(c.A[:4], c.B[:4])                                   # the shipped path
    assert torch_cuda.equal(got, c.mul[:4])


@pytest.mark.parametrize("path", PATHS)
def test_output_on_its_input(ctx, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c = ctx
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    for width in _widths(c.wl):
        f = _built(c.P, c.wl, "mul", width)
        for n in (513, POOL):
            a = c.A[:n].clone()
            got, = f(a, c.B[:n], out=[a])
            assert got is a and torch.equal(a, c.mul[:n]), (width, n)


# ---------------------------------------------------------------------------------------------------------------- flags and neighbours
@pytest.mark.parametrize("path", PATHS)
def test_flags_steer(ctx, torch_cuda, monkeypatch, path):
    torch = torch_cuda
    c = ctx
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    f = _built(c.P, c.wl, "steer")
    for n in (257, POOL):
        got, ok = f(c.A[:n])
        assert torch.equal(ok, c.fa[:n]) and torch.equal(got, c.steer[:n]), n
    zero = torch.zeros(c.F.nbytes, dtype=torch.uint8, device="cuda")
    p = _fp(c.P, c.wl).p
    assert all(torch.equal(c.steer[j], zero) for j in range(16) if p <= c.va[j] < 2 * p)


@pytest.mark.parametrize("path", PATHS)
def test_neighbours_outside_the_limb_contract(ctx, torch_cuda, monkeypatch, path):
    """a byte input beside an element batch some of whose lanes carry limbs up to 2^64 - 1: the wave's vote falls to the exact products,
    for the imported values too"""
    torch = torch_cuda
    c, F = ctx, ctx.F
    if c.wl != 64:
        return                                                   # (one product policy at word length 32: nothing to vote on)
    monkeypatch.setenv("MA_CHAIN_BYTES", path)
    n = 1025
    e = c.e[:, :n].contiguous()
    e[:, ::5] = -1
    e[0, 1::7] = -1
    a, _ = F.modimp(c.A[:n])
    want = F.modexp(F.modsqr(F.modadd(a, e)))
    for width in (1, 2):
        got, = _built(c.P, c.wl, "sqe", width)(e, c.A[:n])
        assert torch.equal(got, want), width


# ---------------------------------------------------------------------------------------------------------------- every kind of array in one call
EVERY = "in a; bytes r; shared k; sel d; t = modmul(a, k); u = modadd(t, r); out modcmv(d, t, u); outbytes u; out flag(r) & (not modis0(u))"
EVERY_N = 640                                                    # the pool: every batch below is a prefix of it
SENTINEL = 0x5a


def _misaligned(torch, t, wl):
    """the flat batch t, rows and all, one word behind a 16-byte aligned address (_at on its bytes)"""
    return _at(torch, t.view(torch.uint8), wl // 8).view(t.dtype)


@pytest.mark.parametrize("P,wl,width", [("X25519", 64, None), ("NIST256", 32, None), ("NIST256", 32, 2)], ids=("X25519-w64", "NIST256-w32", "NIST256-w32-ept2"))
def test_every_kind_of_array(torch_cuda, monkeypatch, P, wl, width):
    """an element batch, a byte record, a shared operand and a selector in; an element batch, a byte record and an int out: every slot of
    in[] and out[] at once, through the main launch and the remainder launch of the one entry body.  The element batches are views of
    rows of EVERY_N words (an even stride: two elements per lane where the width allows, so that n = 1, 3, 513 are the remainder alone,
    the remainder after one lane, and after more than one workgroup of lanes); every output is a view of a buffer one element longer,
    whose last element must stay what it was"""
    from modarith_amd import generate as gen
    from modarith_amd.field import Field
    from modarith_amd.fuse import parse
    from tests.test_gpu_fuse_shared import _bcast, _elements
    torch = torch_cuda
    ch = parse(P, "every_by", EVERY, wl=wl)
    f = ch.build() if width is None else ch.build(plugin_dir=os.path.join(gen.PLUGIN_DIR, "bytes_ept%d" % width), ept=width)
    F = Field(P, wl=wl, tile=None)
    N, nb, n0 = F.N, F.nbytes, EVERY_N
    # the inputs, and the truth call by call through Field, once
    a = _batch(torch, P, wl, n0, 21)
    R = _records(torch, _pool(P, wl, 22)[:n0], nb)
    for j in (1, 300, n0 - 1):                                   # u = 0 there: both values of modis0
        a[:, j] = 0
        R[j] = 0
    k = _elements(P, wl, 1, 23)[0]
    d = torch.randint(0, 2, (n0,), dtype=torch.int32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(24))
    r, ok = F.modimp(R)
    t = F.modmul(a, _bcast(torch, wl, k, a))
    u = F.modadd(t, r)
    want_e = u.clone()
    F.modcmv(d, t, want_e)
    want_b, want_i = F.modexp(u), ok & (1 - F.modis0(u))
    assert 0 < int(want_i.sum()) < n0 and 0 < int(ok.sum()) < n0 and 0 < int(d.sum()) < n0 and int(F.modis0(u).sum()) == 3

    def run(n, ain, ebuf, eout, what):
        bbuf = torch.full((n + 1, nb), SENTINEL, dtype=torch.uint8, device="cuda")
        ibuf = torch.full((n + 1,), SENTINEL, dtype=torch.int32, device="cuda")
        got = f(ain, R[:n], k, d[:n], out=[eout, bbuf[:n], ibuf[:n]])
        assert got[0] is eout
        assert torch.equal(F.to_flat(eout), want_e[:, :n]) and torch.equal(bbuf[:n], want_b[:n]) and torch.equal(ibuf[:n], want_i[:n]), what
        assert bool((bbuf[n] == SENTINEL).all()) and int(ibuf[n]) == SENTINEL, what
        return ebuf

    for path in PATHS:
        monkeypatch.setenv("MA_CHAIN_BYTES", path)
        for n in (1, 3, 513):
            ebuf = torch.full((N, n0), SENTINEL, dtype=a.dtype, device="cuda")
            run(n, a[:, :n], ebuf, ebuf[:, :n], (path, n))
            assert bool((ebuf[:, n:] == SENTINEL).all()), (path, n)
        # tiled, at the smallest tile: the output's tiles are the first of a buffer of one tile more
        tile = 128
        ebuf = torch.full((n0 // tile + 1, N, tile), SENTINEL, dtype=a.dtype, device="cuda")
        run(n0, F.to_tiled(a, tile), ebuf, ebuf[:n0 // tile], (path, "tiled"))
        assert bool((ebuf[n0 // tile] == SENTINEL).all()), (path, "tiled")
        # element arrays one word off 16-byte alignment: one element per lane whatever the build's width
        n = 513
        ain = _misaligned(torch, a, wl)
        ebuf = _misaligned(torch, torch.full((N, n0), SENTINEL, dtype=a.dtype, device="cuda"), wl)
        assert ain.data_ptr() % 16 == wl // 8 == ebuf.data_ptr() % 16
        run(n, ain[:, :n], ebuf, ebuf[:, :n], (path, "misaligned"))
        assert bool((ebuf[:, n:] == SENTINEL).all()), (path, "misaligned")


# ---------------------------------------------------------------------------------------------------------------- the chain the library carries
def _multiples(c, count):
    """G, 2G, ... in affine coordinates with Python integers (a = -3)"""
    p, G = c.fp.p, (c.gx, c.gy)
    pts, Q = [], G
    for _ in range(count):
        pts.append(Q)
        (x1, y1), (x2, y2) = Q, G
        lam = (3 * x1 * x1 - 3) * pow(2 * y1, -1, p) % p if Q == G else (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - x1 - x2) % p
        Q = (x3, (lam * (x1 - x3) - y1) % p)
    return pts


@pytest.mark.parametrize("wl", (64, 32))
def test_pubkey_chain(torch_cuda, monkeypatch, wl):
    from modarith_amd.curves import wcurve
    from modarith_amd.field import Field
    from modarith_amd.fuse import oncurve_chain, pubkey_chain
    torch = torch_cuda
    c = wcurve("NIST256")
    p = c.fp.p
    pts = _multiples(c, 150)
    keys = list(pts)
    keys += [(x ^ (1 << (j % 256)), y) for j, (x, y) in enumerate(pts)]                 # one coordinate bit flipped
    keys += [(x, y ^ (1 << (7 * j % 256))) for j, (x, y) in enumerate(pts)]
    # coordinates that are not below p: points of small x (p = 3 mod 4: a root of the right-hand side is its (p + 1) / 4-th power) written
    # as x + p -- on the curve modulo p, and still no key --, and their y and others out of range
    small = [(k, pow(k ** 3 - 3 * k + c.b, (p + 1) // 4, p)) for k in range(60)]
    small = [(k, y) for k, y in small if (y * y - (k ** 3 - 3 * k + c.b)) % p == 0]
    assert len(small) > 8
    keys += [(k + p, y) for k, y in small] + [(k, y) for k, y in small[:4]] + [(x, p + j) for j, (x, y) in enumerate(pts[:20])]
    keys += [(p, 0), (0, p), ((1 << 256) - 1, (1 << 256) - 1), (0, 0)]
    want = [int(x < p and y < p and (y * y - (x * x * x - 3 * x + c.b)) % p == 0) for x, y in keys]
    assert sum(want) == 150 + 4
    X, Y = _records(torch, [k[0] for k in keys], 32), _records(torch, [k[1] for k in keys], 32)
    F = Field("NIST256", wl=wl, tile=None)
    ch, (b,) = pubkey_chain("NIST256", wl)
    f = ch.build()
    on, (b2,) = oncurve_chain("NIST256", wl, name="oncurve_by")
    assert b2 == b
    (x, fx), (y, fy) = F.modimp(X), F.modimp(Y)
    calls = fx & fy & on.build()(x, y, b)[0]
    assert calls.cpu().tolist() == want
    for path in PATHS:
        monkeypatch.setenv("MA_CHAIN_BYTES", path)
        ok, = f(X, Y, b)
        assert ok.dtype == torch.int32 and ok.cpu().tolist() == want, path
