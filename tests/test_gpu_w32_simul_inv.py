"""The shared inversion of the 32-bit word form on the GPU (csrc/kernels.h k_inv_simul at MA_WL = 32 behind modinv_<P>_w32_batch): the same words
as the per-element kernel for every 32-bit limb pattern, no element spoiling another.

A batch of n = 3 * 16384 + 1237 elements of nres(uniform) with every element of tests/w32_inputs.pool(P) -- arbitrary 32-bit words
included -- and the zero forms 0, p, 2p scattered over positions in different groups and rounds, inverted in one call (the shared
path: modarith_amd_last_launch says so) and in chunks of 8192 (below the threshold: one inversion per element); then in place, on
tiles, at the threshold and one below it, with progenitors, and captured in a graph.  Values by Python integers."""
import pytest

from tests import w32_inputs as wi

pytestmark = pytest.mark.gpu
N_BIG = 3 * 16384 + 1237
THRESHOLD = 32768
CHUNK = 8192


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _launch():
    from modarith_amd import _lib
    return _lib.load().modarith_amd_last_launch().decode()


def _specials(P):
    """(position, limbs): the pool and the zero forms over positions of different lanes, waves and rounds"""
    N, R, _, _, p = wi.SHAPES[P]
    elems = wi.pool(P) + [wi.split(P, 0), wi.split(P, p), wi.split(P, 2 * p)] * 3
    rounds = (N_BIG + 16383) // 16384                       # 4 rounds of (N_BIG + 3) // 4 lanes
    lanes = (N_BIG + rounds - 1) // rounds
    pos, out = set(), []
    for k, e in enumerate(elems):
        r = k % rounds
        j = (k * 131 + (k // 7) * 64 + 5) % lanes           # a stride that visits many waves; collisions in a lane across rounds wanted
        q = r * lanes + j
        while q in pos or q >= N_BIG:
            q = (q + 1) % N_BIG
        pos.add(q)
        out.append((q, e))
    # one lane whose elements are special in EVERY round, one wave that holds nothing but zeros in a round
    for r in range(rounds):
        q = r * lanes + 77
        if q not in pos and q < N_BIG:
            pos.add(q)
            out.append((q, [wi.split(P, 2 * p), [wi.M32] * N, wi.split(P, 0), wi.split(P, p)][r % 4]))
    for j in range(128, 192):
        q = lanes + j
        if q not in pos:
            pos.add(q)
            out.append((q, wi.split(P, p if j % 2 else 0)))
    return out


def _batch(torch, F, P):
    x = F.nres(F.uniform(N_BIG, seed=77, array=3))
    assert x.dim() == 2
    sp = _specials(P)
    idx = torch.tensor([q for q, _ in sp], dtype=torch.int64, device=x.device)
    vals = torch.tensor([[v if v < (1 << 31) else v - (1 << 32) for v in e] for _, e in sp], dtype=torch.int32, device=x.device).T.contiguous()
    x[:, idx] = vals
    return x, sp


def _per_element(torch, F, x):
    """one inversion per element: chunks below the threshold"""
    n = x.shape[1]
    out = torch.empty_like(x)
    for k in range(0, n, CHUNK):
        m = min(CHUNK, n - k)
        src = x[:, k:k + m].contiguous()
        out[:, k:k + m] = F.modinv(src)
        assert _launch() == "modinv(w32)", _launch()
    return out


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_shared_inversion_gives_the_words_of_the_per_element_kernel(torch_cuda, P):
    torch = torch_cuda
    from modarith_amd.field import Field
    from modarith_amd.params import w32_inv_in_contract
    F = Field(P, wl=32, tile=None)
    fp = F.params
    N, R, _, _, p = wi.SHAPES[P]
    x, sp = _batch(torch, F, P)
    want = _per_element(torch, F, x)
    keep = x.clone()
    got = F.modinv(x)
    assert _launch() == "modinv(w32, simultaneous)", _launch()
    assert torch.equal(x, keep)
    bad = (got != want).any(dim=0).nonzero().flatten().tolist()
    assert not bad, "%d elements differ, first at %r" % (len(bad), bad[:8])

    # values, by Python integers: x * inv = 1 on in-domain elements (a sample of the uniform ones, every special one), 0 for zero
    Rm = fp.R if fp.montgomery else 1
    Rinv = pow(Rm, -1, p)
    special = dict(sp)
    sample = sorted(set(range(0, N_BIG, 389)) | set(special))
    xl = [[int(v) & wi.M32 for v in col] for col in x[:, sample].T.tolist()]
    il = [[int(v) & wi.M32 for v in col] for col in got[:, sample].T.tolist()]
    zeros = indomain = 0
    for q, a, b in zip(sample, xl, il):
        if q in special:
            assert a == special[q]
        if not w32_inv_in_contract(fp, a):
            continue                                          # no value to speak of: pinned word for word above
        xv, iv = wi.value(P, a) * Rinv % p, wi.value(P, b) * Rinv % p
        if xv == 0:
            assert b == [0] * N, (q, b)
            zeros += 1
        else:
            assert xv * iv % p == 1, q
            assert wi.value(P, b) < p                         # normalised form
            indomain += 1
    assert zeros >= 9 and indomain >= 100                     # (the three zero forms, three times each; 127 sampled uniform elements)

    # in place (scratch for the prefixes), through the C ABI directly and through Field.modinv (a temporary)
    y = x.clone()
    F._call("modinv", y.data_ptr(), None, y.data_ptr(), N_BIG, F._ld(y), torch.cuda.current_stream().cuda_stream)
    assert _launch() == "modinv(w32, simultaneous, in place)", _launch()
    assert torch.equal(y, want)
    y = x.clone()
    assert F.modinv(y, out=y) is y and torch.equal(y, want)
    assert _launch() == "modinv(w32, simultaneous)", _launch()

    # tiles of 4096 and of 128 (whole tiles: the first 12 * 4096 elements)
    m = 12 * 4096
    for tile in (4096, 128):
        xt = F.to_tiled(x[:, :m].contiguous(), tile)
        wt = _per_element(torch, F, x[:, :m].contiguous())
        assert torch.equal(F.to_flat(F.modinv(xt)), wt), tile
        assert _launch() == "modinv(w32, simultaneous)"
        F._call("modinv", xt.data_ptr(), None, xt.data_ptr(), m, tile, torch.cuda.current_stream().cuda_stream)
        assert _launch() == "modinv(w32, simultaneous, in place)"
        assert torch.equal(F.to_flat(xt), wt), tile

    # at the threshold and one below it
    for n, label in ((THRESHOLD, "modinv(w32, simultaneous)"), (THRESHOLD - 1, "modinv(w32)")):
        xs = x[:, N_BIG - n:].contiguous()
        got_n = F.modinv(xs)
        assert _launch() == label, (n, _launch())
        assert torch.equal(got_n, want[:, N_BIG - n:]), n

    # caller-supplied progenitors on a slice: their own kernel, the same words
    xs = x[:, 4000:4000 + 9000].contiguous()
    h = F.modpro(xs)
    assert torch.equal(F.modinv(xs, h), want[:, 4000:4000 + 9000]) and _launch() == "modinv(w32, h)"
    big_h = F.modpro(x)
    assert torch.equal(F.modinv(x, big_h), want) and _launch() == "modinv(w32, h)"


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_shared_inversion_in_a_captured_graph(torch_cuda, P):
    torch = torch_cuda
    from modarith_amd.field import Field
    F = Field(P, wl=32, tile=None)
    x, _ = _batch(torch, F, P)
    want = F.modinv(x)
    assert _launch() == "modinv(w32, simultaneous)"
    out = torch.zeros_like(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        F.modinv(x, out=out)                                  # warm-up on the side stream
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    out.zero_()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                                 # one kernel, one branch
        F.modinv(x, out=out)
    assert _launch() == "modinv(w32, simultaneous)"
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)
    # in place under capture: no scratch may be taken, the per-element kernel runs -- the same words
    y = x.clone()
    g2 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g2):
        F._call("modinv", y.data_ptr(), None, y.data_ptr(), N_BIG, F._ld(y), torch.cuda.current_stream().cuda_stream)
    assert _launch() == "modinv(w32)", _launch()
    g2.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, want)


def test_the_knob_keeps_one_inversion_per_element(torch_cuda):
    """MA_INV_SIMUL=0 is read once per process: a child process"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import torch\nfrom modarith_amd.field import Field\nfrom modarith_amd import _lib\n"
            "F = Field('X25519', wl=32, tile=None)\nx = F.nres(F.uniform(40000, seed=5))\nz = F.modinv(x)\ntorch.cuda.synchronize()\n"
            "print('LAUNCH', _lib.load().modarith_amd_last_launch().decode())\n"
            "print('ONE', F.to_ints(F.redc(F.modmul(x[:, :4].contiguous(), z[:, :4].contiguous()))))\n")
    env = dict(os.environ, MA_INV_SIMUL="0", PYTHONPATH=root)
    p = subprocess.run([sys.executable, "-c", code], env=env, cwd=root, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-2000:]
    assert "LAUNCH modinv(w32)\n" in p.stdout and "ONE [1, 1, 1, 1]" in p.stdout, p.stdout
