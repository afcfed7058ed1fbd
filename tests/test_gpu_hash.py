"""The batched hashes (include/modarith_amd_hash.h, modarith_amd.hash) on the GPU against hashlib.

The shapes are the padding edges and ragged waves, not large batches: every message length around a block edge sits side by side in
ONE batch through `lens`, so lanes of one wave need different block counts; n in {1, 63, 64, 65, 200} covers a lone lane, a wave
less one, a whole wave, a wave and one, and more than one lane group.  Then the layouts: rows with stride > len, base pointers off
by 1 and 3 bytes, a shared part (stride 0), clamped lengths with a canary, a digest stride wider than the digest, the Ed448 record
shape, one launch under graph capture, and the plain-C caller examples/hash_batch.c.
"""
import hashlib
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHA2_LENGTHS = {"sha256": (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128),
                "sha384": (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 256),
                "sha512": (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 256)}
RATE = {"sha3-224": 144, "sha3-256": 136, "sha3-384": 104, "sha3-512": 72, "shake128": 168, "shake256": 136}
BLOCK = {"sha256": 64, "sha384": 128, "sha512": 128, **RATE}
ALGOS = sorted(BLOCK)
LAUNCH = {a: "hash " + a for a in ALGOS}
_HASHLIB = {"sha256": hashlib.sha256, "sha384": hashlib.sha384, "sha512": hashlib.sha512, "sha3-224": hashlib.sha3_224,
            "sha3-256": hashlib.sha3_256, "sha3-384": hashlib.sha3_384, "sha3-512": hashlib.sha3_512, "shake128": hashlib.shake_128,
            "shake256": hashlib.shake_256}


def lengths_of(algo):
    if algo in SHA2_LENGTHS:
        return SHA2_LENGTHS[algo]
    r = RATE[algo]
    return (0, 1, r - 2, r - 1, r, r + 1, 2 * r - 1, 2 * r)


def truth(algo, msg, olen=32):
    h = _HASHLIB[algo](msg)
    return h.digest(olen) if algo.startswith("shake") else h.digest()


def run(algo, parts, lens=None, olen=32, out=None):
    from modarith_amd import hash as mh
    if algo.startswith("sha3-"):
        return mh.sha3(int(algo[5:]) // 8, parts, lens=lens, out=out)
    if algo.startswith("shake"):
        return getattr(mh, algo)(parts, olen, lens=lens, out=out)
    return getattr(mh, algo)(parts, lens=lens, out=out)


def last_launch():
    from modarith_amd import _lib
    return _lib.load().modarith_amd_last_launch().decode()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def data(torch_cuda):
    """200 rows of 352 seeded bytes, on the host and on the device: every test cuts its records out of these"""
    torch = torch_cuda
    g = torch.Generator().manual_seed(1600)
    host = torch.randint(0, 256, (200, 352), dtype=torch.uint8, generator=g)
    return host, host.cuda()


def rows(t):
    return [bytes(r) for r in t.cpu().tolist()]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("algo", ALGOS)
def test_every_padding_edge_side_by_side_in_one_batch(torch_cuda, data, algo, n):
    torch = torch_cuda
    host, dev = data
    ls = lengths_of(algo)
    lens = [ls[(j + n) % len(ls)] for j in range(n)]
    width = max(ls)
    part = dev[:n, :width]                                                    # rows of `width` bytes, 352 apart: stride > len
    got = run(algo, [part], lens=[torch.tensor(lens, dtype=torch.int32, device="cuda")])
    assert last_launch() == LAUNCH[algo]
    assert got.dtype == torch.uint8 and got.shape == (n, len(truth(algo, b"")))
    want = [truth(algo, bytes(host[j, :lens[j]].tolist())) for j in range(n)]
    assert rows(got) == want


@pytest.mark.parametrize("algo", ["shake128", "shake256"])
def test_shake_output_lengths_around_the_rate(torch_cuda, data, algo):
    torch = torch_cuda
    host, dev = data
    r, n = RATE[algo], 65
    lens = [(0, 67, r - 1, r, 2 * r)[j % 5] for j in range(n)]
    dl = torch.tensor(lens, dtype=torch.int32, device="cuda")
    for olen in (1, 32, 114, r - 1, r, r + 1, 2 * r + 5):
        got = run(algo, [dev[:n, :2 * r]], lens=[dl], olen=olen)
        assert got.shape == (n, olen)
        assert rows(got) == [truth(algo, bytes(host[j, :lens[j]].tolist()), olen) for j in range(n)], olen


def cuts_of(block):
    """column cuts of a row into 1, 2, 4 and 8 parts: at byte offsets 0, 1, 3, 7 and across a block edge, empty parts included"""
    b = block
    return [[], [0], [1], [3], [7], [b - 1], [b + 1], [0, 1, 3], [3, 7, b + 3], [b - 3, b - 3, b + 5],
            [0, 1, 3, 7, 7, b - 1, b + 1], [1, b, b, b + 1, 2 * b - 1, 2 * b, 2 * b + 2]]


@pytest.mark.parametrize("algo", ALGOS)
def test_the_same_records_cut_into_parts(torch_cuda, data, algo):
    """ragged records (every length of the sweep, side by side) given as 1, 2, 4 and 8 column slices of one array: same digests"""
    torch = torch_cuda
    host, dev = data
    n, b = 65, BLOCK[algo]
    ls = lengths_of(algo) + (7, b + 9, 2 * b + 3)
    lens = [ls[j % len(ls)] for j in range(n)]
    width = 2 * b + 8
    assert max(lens) <= width <= 352
    want = [truth(algo, bytes(host[j, :lens[j]].tolist()), 57) for j in range(n)]
    full = torch.tensor(lens, dtype=torch.int64)
    for cuts in cuts_of(b):
        edges = [0] + cuts + [width]
        assert len(edges) - 1 in (1, 2, 4, 8)
        parts = [dev[:n, a:e] for a, e in zip(edges, edges[1:])]
        plens = [(full - a).clamp(0, e - a).to(torch.int32).cuda() for a, e in zip(edges, edges[1:])]
        assert rows(run(algo, parts, lens=plens, olen=57)) == want, cuts


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("algo", ["sha256", "sha512", "shake256"])
def test_rows_of_57_bytes_at_odd_base_addresses(torch_cuda, data, algo, offset):
    torch = torch_cuda
    host, _ = data
    n = 65
    flat = torch.zeros(offset + n * 57 + 8, dtype=torch.uint8)
    flat[offset:offset + n * 57] = host[:n, :57].reshape(-1)
    dflat = flat.cuda()
    part = dflat[offset:offset + n * 57].view(n, 57)
    assert part.data_ptr() % 4 == offset and part.stride(0) == 57
    obuf = torch.zeros(offset + n * 64 + 8, dtype=torch.uint8, device="cuda")
    dl = len(truth(algo, b""))
    out = obuf[offset:offset + n * dl].view(n, dl)                            # the digests at an odd address as well
    got = run(algo, [part], out=out)
    assert got.data_ptr() == out.data_ptr()
    assert rows(got) == [truth(algo, bytes(host[j, :57].tolist())) for j in range(n)]


def test_a_shared_part_has_stride_zero(torch_cuda, data):
    torch = torch_cuda
    host, dev = data
    n = 65
    prefix = b"SigEd448\0\0"
    want = [truth("shake256", prefix + bytes(host[j, :57].tolist()), 114) for j in range(n)]
    assert rows(run("shake256", [prefix, dev[:n, :57]], olen=114)) == want                   # bytes: uploaded once, stride 0
    row = torch.tensor(list(prefix), dtype=torch.uint8, device="cuda").unsqueeze(0).expand(n, len(prefix))
    assert row.stride(0) == 0
    assert rows(run("shake256", [row, dev[:n, :57]], olen=114)) == want                      # an expand()ed row: stride 0 as it is
    assert rows(run("sha256", [dev[:n, :57], prefix, b""])) == [truth("sha256", bytes(host[j, :57].tolist()) + prefix) for j in range(n)]


@pytest.mark.parametrize("algo", ["sha256", "sha512", "sha3-256", "shake256"])
def test_lengths_above_the_part_are_clamped_and_the_canary_is_not_hashed(torch_cuda, data, algo):
    torch = torch_cuda
    host, dev = data
    n, width = 65, 40
    lens = torch.tensor([(1000, 41, 40, 2**31 - 1, 39)[j % 5] for j in range(n)], dtype=torch.int32, device="cuda")
    want = [truth(algo, bytes(host[j, :min(width, (1000, 41, 40, 2**31 - 1, 39)[j % 5])].tolist())) for j in range(n)]
    got = rows(run(algo, [dev[:n, :width]], lens=[lens]))
    assert got == want
    # the bytes behind the part (columns 40 ... of the same rows) are the canary: other values there, the same digests
    other = dev[:n].clone()
    other[:, width:] ^= 0xFF
    assert rows(run(algo, [other[:, :width]], lens=[lens])) == want


@pytest.mark.parametrize("algo", ["sha256", "sha384", "sha3-224", "shake128"])
def test_a_digest_stride_wider_than_the_digest_leaves_the_gap_untouched(torch_cuda, data, algo):
    torch = torch_cuda
    host, dev = data
    n = 65
    dl = len(truth(algo, b""))
    big = torch.full((n + 1, dl + 13), 0xA5, dtype=torch.uint8, device="cuda")
    out = big[:n, :dl]
    run(algo, [dev[:n, :100]], out=out)
    assert rows(big[:n, :dl]) == [truth(algo, bytes(host[j, :100].tolist())) for j in range(n)]
    assert bool((big[:n, dl:] == 0xA5).all()) and bool((big[n] == 0xA5).all())


def test_the_ed448_record_shape(torch_cuda, data):
    """10 shared + 57 + 57 + ragged M of 0..120 bytes, 114 out: SHAKE256(dom4 || R || A || M) of ed448.c:289-298, R and S as the
    two halves of one signature row"""
    torch = torch_cuda
    host, dev = data
    n = 200
    dom4 = b"SigEd448\0\0"
    sig, pub, msg = dev[:n, :114], dev[:n, 114:171], dev[:n, 171:291]
    mlen = [j % 121 for j in range(n)]
    got = run("shake256", [dom4, sig[:, :57], pub, msg], lens=[None, None, None, torch.tensor(mlen, dtype=torch.int32, device="cuda")], olen=114)
    want = [truth("shake256", dom4 + bytes(host[j, :57].tolist()) + bytes(host[j, 114:171].tolist()) + bytes(host[j, 171:171 + mlen[j]].tolist()), 114)
            for j in range(n)]
    assert rows(got) == want and last_launch() == "hash shake256"


def test_one_launch_under_graph_capture_replayed_once(torch_cuda, data):
    """the calls take no memory and do not synchronise: a launch is captured as it is, and its replay gives the same digests"""
    torch = torch_cuda
    host, dev = data
    n = 65
    prefix = torch.tensor(list(b"SigEd448\0\0"), dtype=torch.uint8, device="cuda").unsqueeze(0).expand(n, 10)
    part = dev[:n, :120].clone()
    lens = torch.tensor([j % 121 for j in range(n)], dtype=torch.int32, device="cuda")
    out = torch.zeros((n, 114), dtype=torch.uint8, device="cuda")
    want = run("shake256", [prefix, part], lens=[None, lens], olen=114).clone()               # warm-up outside the capture
    assert rows(want) == [truth("shake256", b"SigEd448\0\0" + bytes(host[j, :j % 121].tolist()), 114) for j in range(n)]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):                                            # one kernel, one branch
            run("shake256", [prefix, part], lens=[None, lens], olen=114, out=out)
    torch.cuda.current_stream().wait_stream(side)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want)


def test_empty_batch_and_python_side_refusals(torch_cuda, data):
    torch = torch_cuda
    _, dev = data
    assert run("sha256", [dev[:0, :57]]).shape == (0, 32)
    with pytest.raises(ValueError):
        run("sha256", [dev[:4, :8]] * 9)
    with pytest.raises(ValueError):
        run("shake256", [dev[:4, :8]], olen=0)
    with pytest.raises(ValueError):
        run("sha256", [dev[:4, :8].cpu()])
    with pytest.raises(ValueError):
        run("sha256", [dev[:4, :8].t()])                                      # bytes of a row not contiguous


def test_c_example_hash_batch(torch_cuda, tmp_path):
    """examples/hash_batch.c: HASH256 of a shared record and the Ed448 verify hash through the plain C-ABI, built with gcc"""
    exe = str(tmp_path / "hash_batch")
    subprocess.check_call(["gcc", "-O2", "-Wall", os.path.join(ROOT, "examples", "hash_batch.c"), "-I", os.path.join(ROOT, "include"),
                           "-L", os.path.join(ROOT, "modarith_amd"), "-l:libmodarith_amd.so", "-Wl,-rpath," + os.path.join(ROOT, "modarith_amd"), "-o", exe])
    n = 200
    p = subprocess.run([exe, str(n)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-500:] + p.stderr[-2000:]
    out = p.stdout.splitlines()
    assert out[0] == 'HASH256("abc") in %d lanes: the FIPS 180-4 value (hash sha256)' % n
    assert out[-1] == "%d records hashed (hash shake256)" % n

    def fill(nbytes, seed):                                                   # the generator of the example
        x, b = seed, bytearray()
        for _ in range(nbytes):
            x = (x * 1103515245 + 12345) & 0xFFFFFFFF
            b.append((x >> 16) & 0xFF)
        return bytes(b)
    sig, pub, msg = fill(n * 114, 1), fill(n * 57, 2), fill(n * 120, 3)
    want = ["%d %s" % (j, hashlib.shake_256(b"SigEd448\0\0" + sig[114 * j:114 * j + 57] + pub[57 * j:57 * j + 57] + msg[120 * j:120 * j + j % 121]).hexdigest(114))
            for j in range(n)]
    assert out[1:-1] == want
