"""Inputs of the 32-bit word form (Wordlength 32), shared by tests/golden/make_golden_w32.py (which runs the reference on them) and
the tests (which run this library on them).  TEST INFRASTRUCTURE ONLY; pure functions of (prime, seed), Python integers throughout.

The element pool covers, for every function: canonical values, values in [p, 2p) with the top limb unmasked, limbs at the budget
edge 2^(Radix+2)-1 in every position, the all-maximal element, and arbitrary 32-bit words (all-ones included).  The operand classes
of tests/edge_inputs.py (the 64-bit form) are the model."""
import random

import numpy as np

W32_PRIMES = ("X25519", "NIST256", "X448")
# (Nlimbs, Radix, Nbits, Nbytes, p): the values the reference generators choose at word length 32 (fixture "params" holds them too)
SHAPES = {
    "X25519": (9, 29, 255, 32, (1 << 255) - 19),
    "NIST256": (9, 29, 256, 32, (1 << 256) - (1 << 224) + (1 << 192) + (1 << 96) - 1),
    "X448": (16, 28, 448, 56, (1 << 448) - (1 << 224) - 1),
}
M32 = (1 << 32) - 1
POOL_SEED = {"X25519": 3201, "NIST256": 3202, "X448": 3203}
MLI_INTS = (0, 1, 2, 3, 19, 39081, 65536, 121665, 121666, 0x7FFFFFFF, -1)


def split(prime, x):
    """integer -> limbs, the top limb takes everything left (unmasked)"""
    N, R, _, _, _ = SHAPES[prime]
    out = []
    for _ in range(N - 1):
        out.append(x & ((1 << R) - 1))
        x >>= R
    assert x <= M32
    out.append(x)
    return out


def value(prime, limbs):
    R = SHAPES[prime][1]
    return sum(int(v) << (R * i) for i, v in enumerate(limbs))


def pool(prime, extra=24):
    """list of elements (limb lists).  `extra`: how many random elements of each of the three value classes follow the directed ones."""
    N, R, n, _, p = SHAPES[prime]
    rng = random.Random(POOL_SEED[prime])
    top = (1 << (R + 2)) - 1
    rb = lambda: rng.randrange(0, 1 << R)
    r = rng.randrange(2, p)
    out = []
    # canonical values
    for v in (0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 32, (1 << 32) - 1, 1 << 64, 1 << (n - 1), (1 << (n - 1)) - 1,
              (1 << R) - 1, 1 << R, ((1 << R) - 1) << R, (1 << n) - p, r, pow(r, -1, p)):
        out.append(split(prime, v % p))
    # [p, 2p), top limb unmasked
    for v in (p, p + 1, 2 * p - 1, 2 * p - 2, p + r, p + (1 << (n - 1))):
        out.append(split(prime, v))
    # the budget edge in every position (other limbs uniform Radix-bit), and its complement (edge everywhere but one position)
    for pos in range(N):
        out.append([top if i == pos else rb() for i in range(N)])
    for pos in range(N):
        out.append([rb() if i == pos else top for i in range(N)])
    out.append([top] * N)                                       # all-maximal
    out.append([top - 1] * N)
    out.append([1 << R] * N)
    out.append([(1 << (R + 1)) - 1] * N)
    # arbitrary 32-bit words
    out.append([M32] * N)
    out.append([1 << 31] * N)
    out.append([(1 << 31) - 1] * N)
    out.append([M32 if i % 2 else 0 for i in range(N)])
    for _ in range(8):
        out.append([rng.randrange(0, 1 << 32) for _ in range(N)])
    for _ in range(extra):
        out.append(split(prime, rng.randrange(0, p)))
        out.append(split(prime, rng.randrange(p, 2 * p)))
        out.append([rng.randrange(0, top + 1) for _ in range(N)])
    return out


def pairs(prime, count):
    """index pairs (i, j) of the binary records: every element once on each side (a seeded permutation), every directed element with
    itself, the all-maximal and all-ones pairs among them"""
    rng = random.Random(POOL_SEED[prime] + 7)
    perm = list(range(count))
    rng.shuffle(perm)
    out = [(i, perm[i]) for i in range(count)]
    out += [(i, i) for i in range(count) if i % 3 == 0]
    return out


def pack(limbs):
    """element -> fixed-width hex string, 8 digits per limb, limb 0 first"""
    return "".join("%08x" % (int(v) & M32) for v in limbs)


def unpack(s):
    return [int(s[i:i + 8], 16) for i in range(0, len(s), 8)]


# ---- bulk comparison (tests/golden/bulk_digests_w32.json.xz): inputs are a pure function of (prime, class)
BULK_N = 1 << 18
BULK_BLOCK = 4096
BULK_CLASSES = ("uniform", "plus_p", "edge")
BULK_OPS = ("modmul", "modsqr", "modadd", "modsub", "nres", "redc")


def _values(prime, n, seed, array):
    """the moduniform integers (tests/util.py uniform_model) of elements 0..n-1 of stream (seed, array)"""
    from tests.util import _stream_key, splitmix64_vec
    _, _, nbits, _, p = SHAPES[prime]
    nwd = (nbits + 63) // 64 + 1
    pos = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(nwd) + np.arange(nwd, dtype=np.uint64)[None, :])
    raw = splitmix64_vec(_stream_key(seed, array), pos).astype("<u8").tobytes()
    return [int.from_bytes(raw[j * nwd * 8:(j + 1) * nwd * 8], "little") % p for j in range(n)]


def soa_of_values(prime, vals, plus_p=False):
    """uint32 [N, n]: limbs of the values (+ p), top limb unmasked"""
    N, R, _, _, p = SHAPES[prime]
    out = np.empty((N, len(vals)), dtype=np.uint32)
    mask = (1 << R) - 1
    for j, v in enumerate(vals):
        if plus_p:
            v += p
        for i in range(N - 1):
            out[i, j] = v & mask
            v >>= R
        out[N - 1, j] = v
    return out


def edge_soa(prime, n, seed, array):
    """uint32 [N, n]: every limb from {0, 1, 2^R-1, 2^R, 2^(R+1)-1, 2^(R+2)-1} (6 of 9 draws) or uniform R-bit (3 of 9), by the
    splitmix64 stream (seed, array) at position limb * n + j (the recipe of tests/util.py edge_soa with this form's Radix)"""
    from tests.util import _stream_key, splitmix64_vec
    N, R, _, _, _ = SHAPES[prime]
    edges = np.array([0, 1, (1 << R) - 1, 1 << R, (1 << (R + 1)) - 1, (1 << (R + 2)) - 1], dtype=np.uint64)
    pos = np.arange(N * n, dtype=np.uint64)
    w = splitmix64_vec(_stream_key(seed, array), pos)
    sel = (w % np.uint64(9)).astype(np.int64)
    rnd = (w >> np.uint64(8)) & np.uint64((1 << R) - 1)
    out = np.where(sel < 6, edges[np.minimum(sel, 5)], rnd)
    return np.ascontiguousarray(out.reshape(N, n).astype(np.uint32))


def bulk_inputs(prime, cls, n=BULK_N):
    """(a, b) uint32 [N, n] for one input class of the bulk comparison"""
    if cls in ("uniform", "plus_p"):
        return (soa_of_values(prime, _values(prime, n, 42, 100), cls == "plus_p"),
                soa_of_values(prime, _values(prime, n, 42, 101), cls == "plus_p"))
    if cls == "edge":
        return edge_soa(prime, n, 43, 104), edge_soa(prime, n, 43, 105)
    raise ValueError(cls)


def block_digests(soa, block=BULK_BLOCK):
    """sha256 (first 16 hex digits) of every `block`-element slice of a uint32 [N, n] batch, limb-major, little-endian words"""
    import hashlib
    n = soa.shape[1]
    return [hashlib.sha256(np.ascontiguousarray(soa[:, k:k + block]).astype("<u4").tobytes()).hexdigest()[:16] for k in range(0, n, block)]
