"""Inputs of the GENERATED fields of the 32-bit word form (modarith_amd.generate.generate_w32), shared by
tests/golden/make_golden_w32_gen.py (which runs the reference's emitted C on them) and the tests (which run this library on them).
TEST INFRASTRUCTURE ONLY; pure functions of the field's parameters (modarith_amd.params.FieldParams at wl=32), Python integers throughout.

The recipe is that of tests/w32_inputs.py, which is keyed to the three built-in primes: canonical values, values in [p, 2p) with the
top limb unmasked, limbs at the budget edge 2^(Radix+2)-1 in every position, the all-maximal element, and arbitrary 32-bit words."""
import random

from modarith_amd import generate as gen

M32 = (1 << 32) - 1
MLI_INTS = (0, 1, 2, 3, 19, 39081, 65536, 121665, 121666, 0x7FFFFFFF, -1)
# random elements per value class after the directed part of the pool, by limb count: sized so that each fixture stays below the
# largest field fixture of the 64-bit form
EXTRA = {5: 24, 9: 20, 14: 12, 18: 6}


def examples():
    """[(tag, command-line argument, family or None)] of modarith_amd.generate.EXAMPLES_W32"""
    return [(gen.resolve(arg, fam, wl=32).name, arg, fam) for arg, fam in gen.EXAMPLES_W32]


def params(tag):
    for arg, fam in gen.EXAMPLES_W32:
        fp = gen.resolve(arg, fam, wl=32)
        if fp.name == tag:
            return fp
    raise KeyError(tag)


def seed(fp):
    return 3300 + fp.p % 9973


def split(fp, x):
    """integer -> limbs, the top limb takes everything left (unmasked)"""
    out = fp.to_limbs(x)
    assert out[-1] <= M32
    return out


def value(fp, limbs):
    return fp.from_limbs(limbs)


def in_contract(fp, limbs):
    """below 2p in digit form (limbs 0..N-2 below 2^Radix, top limb unmasked): what the field functions return and accept"""
    return value(fp, limbs) < 2 * fp.p and not max(limbs[:-1]) >> fp.radix


def pool(fp, extra):
    """list of elements (limb lists).  `extra`: how many random elements of each of the three value classes follow the directed ones."""
    N, R, n, p = fp.nlimbs, fp.radix, fp.n, fp.p
    rng = random.Random(seed(fp))
    top = (1 << (R + 2)) - 1
    rb = lambda: rng.randrange(0, 1 << R)
    r = rng.randrange(2, p)
    out = []
    for v in (0, 1, 2, 3, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 1 << 32, (1 << 32) - 1, 1 << 64, 1 << (n - 1), (1 << (n - 1)) - 1,
              (1 << R) - 1, 1 << R, ((1 << R) - 1) << R, (1 << n) - p, r, pow(r, -1, p)):
        out.append(split(fp, v % p))
    for v in (p, p + 1, 2 * p - 1, 2 * p - 2, p + r, p + (1 << (n - 1))):        # [p, 2p), top limb unmasked
        out.append(split(fp, v))
    for pos in range(N):                                                        # the budget edge in every position ...
        out.append([top if i == pos else rb() for i in range(N)])
    for pos in range(N):                                                        # ... and everywhere but one
        out.append([rb() if i == pos else top for i in range(N)])
    out.append([top] * N)                                                       # all-maximal
    out.append([top - 1] * N)
    out.append([1 << R] * N)
    out.append([(1 << (R + 1)) - 1] * N)
    out.append([M32] * N)                                                       # arbitrary 32-bit words
    out.append([1 << 31] * N)
    out.append([(1 << 31) - 1] * N)
    out.append([M32 if i % 2 else 0 for i in range(N)])
    for _ in range(8):
        out.append([rng.randrange(0, 1 << 32) for _ in range(N)])
    for _ in range(extra):
        out.append(split(fp, rng.randrange(0, p)))
        out.append(split(fp, rng.randrange(p, 2 * p)))
        out.append([rng.randrange(0, top + 1) for _ in range(N)])
    return out


def pairs(fp, count):
    """index pairs (i, j) of the binary records: every element once on each side (a seeded permutation), every third with itself"""
    rng = random.Random(seed(fp) + 7)
    perm = list(range(count))
    rng.shuffle(perm)
    return [(i, perm[i]) for i in range(count)] + [(i, i) for i in range(count) if i % 3 == 0]


def pack(limbs):
    """element -> fixed-width hex string, 8 digits per limb, limb 0 first"""
    return "".join("%08x" % (int(v) & M32) for v in limbs)


def unpack(s):
    return [int(s[i:i + 8], 16) for i in range(0, len(s), 8)]
