"""The fixed-base kernels a caller gets when key generation or signing sits inside a hipGraph: with the stream under capture the library's
scratch pool is not available, and ecn_<c>_mulgen_get_batch / rfc7748_X448_base_batch fall back to kernels that need none --
k_ed25519_mulgen<true>, k_ed448_mulgen<true>, k_x448_base<true> (one record per lane, the inversion and the sign rule inside the kernel)
and k_nist256_mulgen_get, k_secp256k1_mulgen_get (four scalars per lane, one shared inversion, a grid capped at 262 144 lanes).
k_x25519_base (four keys per lane) is the only kernel of its entry, eager and under capture.

Every call is made eagerly and then captured and replayed; the launch name (modarith_amd_last_launch) says which path ran.  The judge
of the curve results is the integer model of tests/curve_model.py (pinned to the fixtures by tests/test_curve_model_cpu.py), the judge
of the rfc7748 base entries is the oracle's ladder (pinned to RFC 7748 by tests/golden/ladder_*.json); every record must also equal
the eager call bit for bit."""
import time

import numpy as np
import pytest

from tests import curve_model

pytestmark = pytest.mark.gpu
CURVES = [("ed25519", "ED25519"), ("ed448", "ED448"), ("nist256", "NIST256"), ("secp256k1", "SECP256K1")]
WEIER = ("nist256", "secp256k1")
PRODUCT, SELF = b"ecn mulgen_get", b"ecn mulgen_get (self-contained)"
BASE_PRODUCT, BASE_SELF = b"rfc7748 base", b"rfc7748 base (self-contained)"
CAP = 262144                    # lanes of the largest grid of the four-per-lane kernels
CHUNK = 1 << 20                 # csrc/edlad_k.h EDLAD_CHUNK
STRIDE = 211                    # the modelled sample of the large batches: a prime, so it visits every lane of a wave
Q4_X448 = 0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffdf3288fa7113b6d26bb58da4085b309ca37163d548de30a4aad6113cc


def eager_then_captured(call, outs, eager_name, captured_name):
    """call(stream) is one C-ABI call that writes the tensors of `outs`.  Made eagerly first (this loads the code objects and gives the eager
    results, returned as copies), then captured on a side stream -- one stream, a linear chain of kernels -- with the launch name read
    directly after the call, inside the capture.  Before each run the outputs are filled with a pattern that is no result (0xA5 bytes,
    sign -1; a zero fill would hide an unwritten record behind the all-zero answers), then the graph is replayed into them."""
    import torch
    from modarith_amd import _lib
    L = _lib.load()
    blank = lambda: [o.fill_(0xA5 if o.dtype == torch.uint8 else -1) for o in outs]
    blank()
    torch.cuda.synchronize()
    rc, name = call(None), L.modarith_amd_last_launch()
    assert rc == 0 and name == eager_name, (rc, name, L.modarith_amd_last_error().decode())
    torch.cuda.synchronize()
    eager = [o.clone() for o in outs]
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            rc = call(side.cuda_stream)
            name = L.modarith_amd_last_launch()
    assert rc == 0 and name == captured_name, (rc, name, L.modarith_amd_last_error().decode())
    blank()
    torch.cuda.synchronize()
    graph.replay()
    torch.cuda.synchronize()
    return eager


def mulgen_get(c, e, want_x=True, want_y=True):
    """ecn_<c>_mulgen_get_batch eagerly and under capture: ((x, y, sign) of the replay, (x, y, sign) of the eager call); an omitted
    coordinate is passed as NULL and comes back as None"""
    import torch
    from modarith_amd import _lib
    f = getattr(_lib.load(), "ecn_%s_mulgen_get_batch" % c)
    n = e.shape[0]
    x = torch.empty_like(e) if want_x else None
    y = torch.empty_like(e) if want_y else None
    sign = torch.empty(n, dtype=torch.int32, device="cuda")
    outs = [t for t in (x, y, sign) if t is not None]
    ptr = lambda t: None if t is None else t.data_ptr()
    eager = eager_then_captured(lambda s: f(e.data_ptr(), ptr(x), ptr(y), sign.data_ptr(), n, s), outs, PRODUCT, SELF)
    eager = [eager.pop(0) if t is not None else None for t in (x, y, sign)]
    return (x, y, sign), tuple(eager)


def base(curve, k):
    """rfc7748_<curve>_base_batch eagerly and under capture: (replay, eager)"""
    import torch
    from modarith_amd import _lib
    f = getattr(_lib.load(), "rfc7748_%s_base_batch" % curve)
    out = torch.empty_like(k)
    eager, = eager_then_captured(lambda s: f(k.data_ptr(), out.data_ptr(), k.shape[0], s), [out], BASE_PRODUCT,
                                 BASE_SELF if curve == "X448" else BASE_PRODUCT)
    return out, eager


def comb_edges(name, nbytes):
    """single comb digits d * 2^(W i): W from the table emitter, d around the point where the signed digit turns negative and at
    both ends of its range, in the bottom two windows and in the top windows that still fit the record (the last window with
    a bit inside the record holds one bit of a 256-bit record at W = 5: the two below it are taken too)"""
    from modarith_amd import emit
    W = emit.COMB_CURVES[name][0]
    top = (8 * nbytes - 1) // W
    out = [d << (W * i) for i in (0, 1, top - 2, top - 1, top) for d in (1, (1 << (W - 1)) - 1, 1 << (W - 1), (1 << (W - 1)) + 1, (1 << W) - 1)]
    return [v for v in out if v < 1 << (8 * nbytes)]


def corner_scalars(m):
    """(finite corners, scalars whose result is the point at infinity)"""
    bits = 8 * m.nbytes
    q, top = m.q, 1 << bits
    hexes = [int(ch * (2 * m.nbytes), 16) for ch in "789"]
    finite = [1, 2, q - 1, q + 1, top - 1, top >> 1, (top >> 1) - 1] + hexes + comb_edges(m.name, m.nbytes)
    return finite, [0, q, top // q * q]


def records(torch, ints, nbytes, order="big"):
    return torch.tensor(np.frombuffer(b"".join(v.to_bytes(nbytes, order) for v in ints), dtype=np.uint8).reshape(len(ints), nbytes).copy(), device="cuda")


def check_against_model(m, scalars, want, got, idx, want_x=True, want_y=True):
    """records idx of one call against the model's (x, y) of the same records: the delivered coordinates, and sign = the parity of the
    omitted one, 0 when both are delivered"""
    x, y, sign = got
    hx, hy, hs = (None if x is None else x.cpu().numpy()), (None if y is None else y.cpu().numpy()), sign.cpu().numpy()
    for j, (wx, wy) in zip(idx, want):
        if want_x:
            assert hx[j].tobytes() == wx, (m.name, "x", j, hex(scalars[j]))
        if want_y:
            assert hy[j].tobytes() == wy, (m.name, "y", j, hex(scalars[j]))
        parity = 0 if (want_x and want_y) else ((wx if want_y else wy)[-1] & 1)
        assert int(hs[j]) == parity, (m.name, "sign", j, hex(scalars[j]), int(hs[j]), parity)


def same(a, b):
    import torch
    return all((s is None and t is None) or torch.equal(s, t) for s, t in zip(a, b))


@pytest.mark.parametrize("c,name", CURVES)
def test_scratchless_mulgen_get_at_the_scalar_edges(c, name):
    """Small batches through k_ed25519_mulgen<true> / k_ed448_mulgen<true> (n = 175: two full waves and a ragged third) and
    k_nist256_mulgen_get / k_secp256k1_mulgen_get (n = 507: 128 lanes, lane t holds records t, t + 128, t + 256, t + 384, and for
    t >= 123 the fourth slot is the duplicate of record t).  Scalars: 0, 1, 2, q - 1, q, q + 1, the largest multiple of q in a record,
    all ones, the top bit and the value below it, 0x77.., 0x88.., 0x99.., single comb digits at both ends of the record, random
    records.  On the Weierstrass curves the scalars with an infinite result are placed so that one lane has four infinite results, one
    lane of the ragged tail has an infinite first record (and so an infinite duplicate), other lanes have one, two and three, and
    every slot is the infinite one of some lane.  Every record against the integer model (the corners through its plain double-and-add,
    the rest through its table form) and against the eager call; then with x = NULL and with y = NULL: the delivered coordinate
    unchanged, sign the parity of the omitted one."""
    import torch
    t0 = time.perf_counter()
    m = curve_model.model(name)
    finite, infinite = corner_scalars(m)
    rng = np.random.default_rng(2024)
    rnd = lambda: int.from_bytes(rng.bytes(m.nbytes), "big")
    if c in WEIER:
        n, lanes = 507, 128
        e = [None] * n
        rec = lambda lane, slot: lane + lanes * slot
        inf_at = [rec(5, g) for g in range(4)]                                          # all four
        inf_at += [rec(125, 0)]                                                         # ragged tail: records 125, 253, 381 and the duplicate of 125
        inf_at += [rec(10, 0), rec(11, 1), rec(12, 2), rec(13, 3)]                      # exactly one, every slot
        inf_at += [rec(20, 0), rec(20, 3), rec(21, 1), rec(21, 2)]                      # exactly two
        inf_at += [rec(30, 0), rec(30, 1), rec(30, 2), rec(31, 1), rec(31, 2), rec(31, 3)]      # exactly three
        for i, j in enumerate(inf_at):
            e[j] = infinite[i % len(infinite)]
        free = [j for j in ([0, n - 1, 122, 123, 127, 128, 255, 256, 383, 384] + list(range(1, n, 7))) if e[j] is None]
        free = list(dict.fromkeys(free))
    else:
        n = 175
        e = [None] * n
        free = [0, n - 1, 63, 64, 127, 128] + [j for j in range(1, n - 1) if j not in (63, 64, 127, 128)]
        finite = infinite + finite
    assert len(free) >= len(finite)
    for j, v in zip(free, finite):
        e[j] = v
    corners = [j for j in range(n) if e[j] is not None]
    e = [rnd() if v is None else v for v in e]
    # the model: corners by the plain double-and-add, everything else by the table form
    want = m.base_bytes(e)
    for j in corners:
        assert want[j] == m.affine_bytes(e[j], m.G), (name, j)
    assert n - len(corners) >= 64
    if c in WEIER:                                                                      # the layout is what the docstring says it is
        isinf = [w == m.export(None) for w in want]
        per_lane = [[isinf[t + lanes * g if t + lanes * g < n else t] for g in range(4)] for t in range(lanes)]
        counts = {k: [t for t in range(lanes) if sum(per_lane[t]) == k] for k in range(5)}
        assert counts[4] == [5] and counts[3] == [30, 31] and counts[2] == [20, 21, 125] and counts[1] == [10, 11, 12, 13], counts
        assert 125 + 3 * lanes >= n and per_lane[125] == [True, False, False, True] and all(any(per_lane[t][g] and sum(per_lane[t]) < 4 for t in range(lanes)) for g in range(4))
    eb = records(torch, e, m.nbytes)
    t_model = time.perf_counter() - t0
    got, eager = mulgen_get(c, eb)
    check_against_model(m, e, want, got, range(n))
    assert same(got, eager)
    gx, ex = mulgen_get(c, eb, want_y=False)
    check_against_model(m, e, want, gx, range(n), want_y=False)
    assert gx[1] is None and same(gx, ex) and torch.equal(gx[0], got[0])
    gy, ey = mulgen_get(c, eb, want_x=False)
    check_against_model(m, e, want, gy, range(n), want_x=False)
    assert gy[0] is None and same(gy, ey) and torch.equal(gy[1], got[1])
    print("%s: n = %d, %d corner records, model %.2f s, total %.2f s" % (name, n, len(corners), t_model, time.perf_counter() - t0))


def base_keys(curve, n, nb, spots, seed):
    """random little-endian keys with the corner keys at `spots` (each spot: zero, all ones, 0x88.., 0x77.., and for X448 the record
    of 4q, whose answer is all zero) -- returns the host array"""
    rng = np.random.default_rng(seed)
    k = rng.integers(0, 256, size=(n, nb), dtype=np.uint8)
    corner = [bytes(nb), b"\xff" * nb, b"\x88" * nb, b"\x77" * nb] + ([Q4_X448.to_bytes(56, "little")] if curve == "X448" else [])
    for s in spots:
        for i, v in enumerate(corner):
            j = s + i if s + len(corner) <= n else s - i
            k[j] = np.frombuffer(v, dtype=np.uint8)
    return k


@pytest.mark.parametrize("curve", ["X448", "X25519"])
def test_scratchless_rfc7748_base_small_batch(oracle, curve):
    """k_x448_base<true> under capture (n = 175: two full waves and a ragged third) and, beside it, k_x25519_base at the same size
    (64 lanes: records t, t + 64, t + 128 and, for t >= 47, the duplicate of record t): corner keys at the start, at a wave boundary
    and at the end, every record against the oracle's ladder on u = 5 / 9 and against the eager call; 4q on X448 gives the all-zero record"""
    import torch
    nb, u0 = (56, 5) if curve == "X448" else (32, 9)
    n = 175
    k = base_keys(curve, n, nb, (0, 62, n - 1), 7)
    got, eager = base(curve, torch.from_numpy(k).cuda())
    assert torch.equal(got, eager)
    u = bytes([u0]) + bytes(nb - 1)
    hg = got.cpu().numpy()
    for j in range(n):
        assert hg[j].tobytes() == oracle.ladder(curve, k[j].tobytes(), u), (curve, j)
    if curve == "X448":
        assert not hg[4].any() and not hg[n - 1 - 4].any()


def sprinkle(n, boundary, values):
    """{record: scalar}: the four values at records 0..3, on the last four records before `boundary`, on the four from it on, and on
    the last four of the batch -- so record 0, boundary - 1, boundary, boundary + 1 and n - 1 hold one each, the infinite ones among them"""
    zero, q, ones, edge = values
    out = {}
    for start, vals in ((0, (zero, q, ones, edge)), (boundary - 4, (edge, ones, q, zero)), (boundary, (zero, q, ones, edge)), (n - 4, (edge, ones, zero, q))):
        for i, v in enumerate(vals):
            out[start + i] = v
    return out


@pytest.mark.parametrize("c,name", CURVES)
def test_scratchless_mulgen_get_second_pass_and_chunk_boundary(c, name):
    """The four-per-lane Weierstrass kernels at n = 4 * 262144 + 77: the grid is capped at 262 144 lanes, the second grid-stride pass is 77
    lanes whose three further slots are all duplicates of their first record.  The Edwards kernels at n = 2^20 + 130: one full chunk
    and a ragged second launch at offset `first`.  Scalars 0, q, all ones and a comb edge sit at record 0, on both sides of the pass /
    chunk boundary and at the end.  Every record equals the eager path (the one-scalar-per-lane kernels with the shared export);
    the sprinkled records and every 211th equal the integer model; with y = NULL, x is unchanged and sign is the parity of y."""
    import torch
    t0 = time.perf_counter()
    m = curve_model.model(name)
    n, boundary = (4 * CAP + 77, 4 * CAP) if c in WEIER else (CHUNK + 130, CHUNK)
    spots = sprinkle(n, boundary, (0, m.q, (1 << (8 * m.nbytes)) - 1, comb_edges(name, m.nbytes)[-2]))
    gen = torch.Generator(device="cuda").manual_seed(23)
    eb = torch.randint(0, 256, (n, m.nbytes), dtype=torch.uint8, device="cuda", generator=gen)
    js = sorted(spots)
    eb[torch.tensor(js, device="cuda")] = records(torch, [spots[j] for j in js], m.nbytes)
    idx = sorted(set(js) | set(range(0, n, STRIDE)))
    he = eb[torch.tensor(idx, device="cuda")].cpu().numpy()
    scalars = {j: int.from_bytes(he[i].tobytes(), "big") for i, j in enumerate(idx)}
    want = m.base_bytes([scalars[j] for j in idx])
    assert all(want[idx.index(j)] == m.export(None) for j in js if spots[j] in (0, m.q))
    t_model = time.perf_counter() - t0
    got, eager = mulgen_get(c, eb)
    check_against_model(m, scalars, want, got, idx)
    assert same(got, eager)
    gx, ex = mulgen_get(c, eb, want_y=False)
    check_against_model(m, scalars, want, gx, idx, want_y=False)
    assert same(gx, ex) and torch.equal(gx[0], got[0])
    print("%s: n = %d, %d modelled records, model %.2f s, total %.2f s" % (name, n, len(idx), t_model, time.perf_counter() - t0))


@pytest.mark.parametrize("curve", ["X25519", "X448"])
def test_rfc7748_base_second_pass_and_chunk_boundary(oracle, curve):
    """k_x25519_base at n = 4 * 262144 + 77, eagerly and under capture (one kernel, one name): the second grid-stride pass of 77 lanes,
    which no smaller batch reaches; the judge of every record is the ladder kernel on u = 9.  k_x448_base<true> under capture at
    n = 2^20 + 130: one full chunk and a ragged second launch; the judge of every record is the eager call (the product path).  Corner
    keys on both sides of the boundary and at both ends; those and every 211th record against the oracle's ladder."""
    import torch
    from modarith_amd.field import rfc7748
    nb, u0 = (56, 5) if curve == "X448" else (32, 9)
    n, boundary = (4 * CAP + 77, 4 * CAP) if curve == "X25519" else (CHUNK + 130, CHUNK)
    hk = base_keys(curve, n, nb, (0, boundary - 5, boundary, n - 1), 29)
    k = torch.from_numpy(hk).cuda()
    got, eager = base(curve, k)
    assert torch.equal(got, eager)
    if curve == "X25519":
        u = torch.zeros_like(k)
        u[:, 0] = u0
        assert torch.equal(got, rfc7748(curve, k, u))
    idx = sorted(set(range(0, n, STRIDE)) | set(range(0, 5)) | set(range(boundary - 5, boundary + 5)) | set(range(n - 5, n)))
    hg = got[torch.tensor(idx, device="cuda")].cpu().numpy()
    ub = bytes([u0]) + bytes(nb - 1)
    for i, j in enumerate(idx):
        assert hg[i].tobytes() == oracle.ladder(curve, hk[j].tobytes(), ub), (curve, j)
    if curve == "X448":
        assert not got[4].any() and not got[boundary + 4].any()
