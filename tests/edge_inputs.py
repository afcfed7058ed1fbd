"""Inputs at the edge of the limb budget, for every prime: shared by tests/test_fast_products_host.py (CPU) and
tests/test_gpu_edge_products.py (GPU).  TEST INFRASTRUCTURE ONLY.

The FAST products of csrc/field.h (operands cut at P::SPLIT, 64-bit accumulators, column chain, half-limb forms) are right only
because emit.split_point / chain_ok / sparse_terms prove that no accumulator passes 2^64 with every limb at 2^(Radix+2) - 1.  The
records built here contain that input -- the same class in every limb of both operands -- and its neighbours; drawing each limb's
class independently never produces it (for nine limbs: one element in 10^18).

Everything is built with Python integers and converted to uint64 at the end: for a radix of 62 the budget 2^(R+2) is not a 64-bit
value (T = 64, top = the all-ones word), and a numpy shift of a uint64 by 64 does not give 0."""
import numpy as np

M64 = (1 << 64) - 1


def limb_top(fp, limit=None):
    """(T, top): the width of the limb budget min(R + 2, 64) and the largest limb inside it; `limit` replaces top for the forms
    whose budget is narrower (field.h FOLD52: (2^64 - 1) / mm)"""
    T = min(fp.radix + 2, 64)
    top = (1 << T) - 1
    if limit is not None:
        top = min(top, int(limit))
    return T, top


def edge_classes(fp, H, limit=None):
    """the limb classes E, duplicates removed, order kept.  H: the cut position P::SPLIT ((R + 2) / 2 where there is none).  "2^H - 1" and
    "top with its low H bits cleared" put the maximum into one HALF of the cut and zero into the other: what tells an s1 overflow from an
    s0 / s2 one.  The low limb of p (and its complement) make the first Montgomery reduction digit extreme."""
    R = fp.radix
    T, top = limb_top(fp, limit)
    p0 = fp.p & ((1 << R) - 1)
    E = [0, 1, (1 << R) - 1, 1 << R, (1 << (R + 1)) - 1, top, top - 1, (1 << H) - 1, 1 << H, top & ~((1 << H) - 1), p0, (1 << R) - 1 - p0]
    if limit is not None:
        E = [min(v, top) for v in E] + [top - 2]
    return list(dict.fromkeys(v & M64 for v in E))


def _u64(rows):
    """list of per-element limb lists (Python ints) -> uint64 [N, n]"""
    return np.ascontiguousarray(np.array(rows, dtype=np.uint64).T)


def uniform_below(rng, top, shape):
    """uniform limbs in [0, top]"""
    return rng.integers(0, top, size=shape, dtype=np.uint64, endpoint=True)


def first_digit(fp, a0, b0):
    """the first reduction digit of the Montgomery product of two elements with low limbs a0, b0 (field.h monty_digit<0>: column 0 holds
    a0 * b0 alone): (a0 * b0 * ndash) mod 2^R"""
    return (a0 * b0 * fp.ndash) & ((1 << fp.radix) - 1)


def directed_low_limbs(fp):
    """Montgomery primes: low limbs a0 inside the budget for which the first reduction digit of redc(a) = modmul(a, 1) and of
    nres(a) = modmul(a, R^2 mod p) is 2^R - 1, and others for which it is 0.  The digit is (a0 * b0 * ndash) mod 2^R with
    ndash * p0 = -1 (mod 2^R), so for redc (b0 = 1) the maximal digit needs a0 = p0 (mod 2^R); for nres it needs
    a0 = -(r2_0 * ndash)^-1, which exists only when r2_0 is odd.  Returns {"redc_max": [...], "nres_max": [...], "zero": [...]}."""
    R = fp.radix
    Q = 1 << R
    T, top = limb_top(fp)
    lifts = [k << R for k in range(4) if (k << R) <= top]
    p0 = fp.p & (Q - 1)
    assert (fp.ndash * p0 + 1) % Q == 0, "ndash is -1 / p mod 2^Radix"
    out = {"redc_max": [(p0 + k) for k in lifts if p0 + k <= top], "zero": list(lifts), "nres_max": []}
    r20 = fp.r2[0]
    if r20 % 2 == 1:
        x = (-pow(r20 * fp.ndash, -1, Q)) % Q
        out["nres_max"] = [x + k for k in lifts if x + k <= top]
    return out


def build_inputs(fp, H, n, seed, limit=None):
    """(a, b, info): uint64 [N, n] operands and the index ranges of the directed parts.
      [0, |E|^2)            a = one class in every limb, b = one class in every limb (holds the worst column)
      then N * |E|          the maximum in every limb of a but one, the odd limb over every position and class; b all-maximal
                            (the reduction digits depend on the low limbs: the worst digit sequence is not the all-maximal input)
      then 0, p, 2p as limbs (a; modinv of a value = 0), b uniform
      then (Montgomery)     the directed low limbs of directed_low_limbs(), other limbs maximal / uniform
      then mixtures         each limb a class with probability 0.7, else uniform in [0, top]
      then uniform          every limb uniform in [0, top]      (the two share what is left of n, half each)"""
    N = fp.nlimbs
    T, top = limb_top(fp, limit)
    E = edge_classes(fp, H, limit)
    rng = np.random.default_rng(seed)
    A, B = [], []
    for ea in E:
        for eb in E:
            A.append([ea] * N)
            B.append([eb] * N)
    info = {"E": E, "top": top, "same_class": (0, len(A))}
    for pos in range(N):
        for c in E:
            A.append([c if i == pos else top for i in range(N)])
            B.append([top] * N)
    info["odd_one"] = (info["same_class"][1], len(A))
    zero_like = [[0] * N, fp.to_limbs(fp.p), fp.to_limbs(2 * fp.p)]
    k0 = len(A)
    for z in zero_like:
        assert all(v <= top for v in z)
        A.append(list(z))
        B.append([int(v) for v in uniform_below(rng, top, N)])
    info["zero_like"] = (k0, len(A))
    k0 = len(A)
    info["directed"] = {}
    if fp.montgomery and limit is None:
        for kind, lows in directed_low_limbs(fp).items():
            s = len(A)
            for a0 in lows:
                A.append([a0] + [top] * (N - 1))
                B.append([top] * N)
                A.append([a0] + [int(v) for v in uniform_below(rng, top, N - 1)])
                B.append([int(v) for v in uniform_below(rng, top, N)])
            info["directed"][kind] = (s, len(A))
    m = len(A)
    assert m < n, "n too small for the directed records of %s (%d)" % (fp.name, m)
    a, b = np.empty((N, n), dtype=np.uint64), np.empty((N, n), dtype=np.uint64)
    a[:, :m], b[:, :m] = _u64(A), _u64(B)
    rest = n - m
    nmix = rest // 2
    cls = np.array(E, dtype=np.uint64)
    for arr in (a, b):
        pick = cls[rng.integers(0, len(E), size=(N, nmix))]
        uni = uniform_below(rng, top, (N, nmix))
        arr[:, m:m + nmix] = np.where(rng.random((N, nmix)) < 0.7, pick, uni)
        arr[:, m + nmix:] = uniform_below(rng, top, (N, rest - nmix))
    info["mixture"] = (m, m + nmix)
    info["uniform"] = (m + nmix, n)
    assert int(a.max()) <= top and int(b.max()) <= top
    return np.ascontiguousarray(a), np.ascontiguousarray(b), info


def values(fp, x):
    """v(x) = sum x_i 2^(R i) of every element of a uint64 [N, n] batch, as Python integers"""
    R = fp.radix
    cols = [[int(v) for v in row] for row in x]
    return [sum(cols[i][j] << (R * i) for i in range(len(cols))) for j in range(x.shape[1])]


def hexrec(x, j):
    return "[" + " ".join("%x" % int(v) for v in x[:, j]) + "]"


def first_diff(got, want):
    """index of the first element in which two [N, n] batches differ, or None"""
    bad = np.nonzero((got != want).any(axis=0))[0]
    return int(bad[0]) if bad.size else None


class Ref:
    """the CPU oracle of one prime behind one face: the per-prime restatement where there is one (tests/oracle_binding.py),
    the generic oracle (tests/generic_oracle.py, pinned to the reference's outputs over the whole 64-bit limb range by
    test_generic_oracle.py::test_round2_modnsqr_and_out_of_contract) for the rest.  uint64 [N, n] in and out."""
    GEN_OPS = {"modmul": 0, "modsqr": 3, "nres": 5, "redc": 6, "modinv": 7, "modsqrt": 8}

    def __init__(self, oracle, P):
        self.oracle, self.P = oracle, P
        self.per_prime = P in oracle.primes
        if not self.per_prime:
            from tests.generic_oracle import Generic
            self.G = Generic(oracle.lib, P)

    def _gen(self, op, a, b=None):
        from tests.util import vp
        c = np.empty_like(a)
        n = a.shape[1]
        self.G.lib.gen_batch(self.G.R, self.GEN_OPS[op], vp(a), vp(b) if b is not None else None, vp(c), n, n)
        return c

    def modmul(self, a, b):
        from tests.util import oracle_bin
        a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return oracle_bin(self.oracle, "modmul", self.P, a, b) if self.per_prime else self._gen("modmul", a, b)

    def un(self, op, a):
        from tests.util import oracle_un
        a = np.ascontiguousarray(a)
        return oracle_un(self.oracle, op, self.P, a) if self.per_prime else self._gen(op, a)

    def modnsqr(self, a, k):
        for _ in range(k):                   # modnsqr is k squarings in place (pseudo.py:745-755)
            a = self.un("modsqr", a)
        return a

    def modqr(self, a):
        """int32 [n]"""
        out = np.empty(a.shape[1], dtype=np.int32)
        for j in range(a.shape[1]):
            x = [int(v) for v in a[:, j]]
            if self.per_prime:
                out[j] = self.oracle.fn("modqr", self.P)(None, self.oracle.arr(self.P, x))
            else:
                out[j] = self.G.lib.gen_modqr(self.G.R, None, self.G.arr(x))
        return out


# Findings (measured with the oracle, which reproduces the reference's words on these inputs): for these moduli the reference's own
# arithmetic is not integer arithmetic any more on limbs beyond the tight form -- its 128-bit column sums, the one-word second pass of
# the "tighter reduction" form or its one-word pre-multiplied operands (mm * a, 2 * a) wrap -- so what it returns for modmul / modsqr is
# not congruent to the product.  The exact form returns the same words there (asserted on every record); the congruence is asserted on
# the tight records only (limbs below 2^Radix under the top one, value below 2p: the form of the reference's own outputs).
CONGRUENCE_FINDINGS = {
    "PM266": "5 x 54, EPM + fred: the one-word second pass", "PM336": "6 x 56, EPM + fred: the one-word second pass",
    "2519": "5 x 51, EPM + fred: the one-word second pass", "NUMS256W": "5 x 52, EPM: mm * a wraps at 64 bits beyond (2^64 - 1) / mm",
    "PM512": "9 x 57, mm = 0x472: mm times the folded 128-bit sum", "C41417": "7 x 60: 128-bit column sums", "M607": "10 x 61: 128-bit column sums",
    "GM240": "4 x 61: 128-bit column sums", "GM384": "7 x 62: 128-bit column sums", "C41417M": "7 x 60: 128-bit column sums"}


def policy_name():
    import os
    return "MA_FORCE_FAST" if os.environ.get("MA_FORCE_FAST") == "1" else "MA_FORCE_EXACT" if os.environ.get("MA_FORCE_EXACT") == "1" else "default vote"


def assert_same(P, op, a, b, got, want, policy=None):
    """limb-for-limb equality of two [N, n] batches; the message names prime, operation, policy and element and prints both operands and
    both results in hex, so that one run is enough to reproduce a difference in the host tier"""
    j = first_diff(got, want)
    assert j is None, "%s %s policy=%s element %d of %d (%d differ)\n  a    = %s\n  b    = %s\n  got  = %s\n  want = %s" % (
        P, op, policy or policy_name(), j, got.shape[1], int((got != want).any(axis=0).sum()), hexrec(a, j), hexrec(b, j) if b is not None else "-",
        hexrec(got, j), hexrec(want, j))


def chain_records(fp, a, info, count, seed=99):
    """operands for modinv / modsqrt / modqr: x^PE by an addition chain.  The reference takes its chain from an external tool, the oracle and
    the engine each have their own; the words agree (after redc) wherever every link is integer arithmetic.  An operand with the maximum in
    every limb (16p and more) is outside the reference's domain: its first products leave the limb budget, and what the chain returns then
    depends on the chain -- the engine's exact form and the oracle differ there.  The chain is closed on values below 2p (a Montgomery product
    of two such values is below 4p^2 / M + p <= 2p since 4p <= M; the pseudo-Mersenne second pass leaves less than 2p).  So: the directed
    records of value <= 2p (tight ones below 2p for CONGRUENCE_FINDINGS) -- 0, 1 in every limb, and 0, p, 2p written as limbs among them --
    then the edges of that domain and `count` values drawn below 2p, in the reference's own limb form (top limb unmasked).
    Returns (uint64 [N, m], values)."""
    p, q = fp.p, np.uint64(1 << fp.radix)
    m = info["mixture"][0]
    d = np.ascontiguousarray(a[:, :m])
    v = values(fp, d)
    if fp.name in CONGRUENCE_FINDINGS:
        keep = (d[:-1] < q).all(axis=0) & np.array([x < 2 * p for x in v])
    else:
        keep = np.array([x <= 2 * p for x in v])
    z0 = info["zero_like"][0]
    assert keep[0] and keep[z0] and keep[z0 + 1]
    rng = np.random.default_rng(seed)
    vals = [0, 1, 2, p - 2, p - 1, p, p + 1, 2 * p - 1] + [int.from_bytes(rng.bytes(fp.nbytes + 8), "little") % (2 * p) for _ in range(count)]
    recs = np.ascontiguousarray(np.concatenate([d[:, keep], _u64([fp.to_limbs(x) for x in vals])], axis=1))
    return recs, [x for x, ok in zip(v, keep) if ok] + vals
