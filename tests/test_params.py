"""The parameter driver (modarith_amd/params.py, emit.py) against the constants captured from the
reference generators (tests/golden/field_*.json "params").  CPU only."""
import os
import random

import pytest

from modarith_amd import emit
from modarith_amd import generate as gen
from modarith_amd.params import derive as _derive_named
from tests.conftest import load_golden

# the built-in primes, and the unnamed moduli of the generator mode (modarith_amd.generate.EXAMPLES) under their tags
GENERATED = {gen.resolve(arg, fam).name: (arg, fam) for arg, fam in gen.EXAMPLES}
ALL = list(emit.BUILT_PRIMES) + list(GENERATED)


def derive(P):
    return gen.resolve(*GENERATED[P]) if P in GENERATED else _derive_named(P)


def _i(v):
    return int(v, 16) if isinstance(v, str) else int(v)


@pytest.mark.parametrize("P", ALL)
def test_driver_matches_reference_constants(P):
    g = load_golden("field_%s.json" % P)["params"]
    fp = derive(P)
    assert (fp.n, fp.radix, fp.nlimbs, fp.xcess, fp.nbytes, fp.pm1d2) == (g["n"], g["base"], g["N"], g["xcess"], g["Nbytes"], g["PM1D2"])
    assert fp.p == _i(g["p"]) and fp.pe == _i(g["PE"])
    assert fp.roi == [_i(v) for v in g["ROI"]]
    hdr = " ".join(g["header"])
    for key, val in (("Nlimbs", fp.nlimbs), ("Radix", fp.radix), ("Nbits", fp.n), ("Nbytes", fp.nbytes)):
        assert "#define %s %d" % (key, val) in hdr
    assert ("#define MONTGOMERY" in hdr) == fp.montgomery
    if fp.family == "pseudo":
        assert (fp.m, fp.mm, fp.tw) == (_i(g["m"]), _i(g["mm"]), _i(g["TW"]))
        assert (fp.overflow, fp.fred, fp.epm, fp.carry_on) == (g["overflow"], g["fred"], g["EPM"], g["carry_on"])
        assert fp.bad_overflow == g["bad_overflow_mul"] == g["bad_overflow_sqr"]
    else:
        assert fp.ppw == [(-_i(v[1:]) if v.startswith("-") else _i(v)) for v in g["ppw"]]
        assert (fp.E, fp.R, fp.ndash, fp.trin) == (g["E"], _i(g["R"]), _i(g["ndash"]), g["trin"])
        assert fp.r2 == [_i(v) for v in g["cw"]]
        assert g["fullmonty"] is (fp.ndash != 1) and g["PM"] is fp.pm
        if fp.pm:
            assert _i(g["M"]) == fp.m == -fp.ppw[0]


def test_reference_stdout_lines():
    """the generators' own log lines (SURVEY 8(a) "pinned by")"""
    log = "\n".join(load_golden("field_X25519.json")["params"]["log"])
    assert "Chosen radix is 51 bits, using 5 limbs with excess of 0 bits" in log
    assert "Tighter reduction" in log and "Fully Exploitable Pseudo-Mersenne detected" in log
    log = "\n".join(load_golden("field_X448.json")["params"]["log"])
    assert "Extra virtual limb added" in log and "lucky trinomial" in log


@pytest.mark.parametrize("P", ALL)
def test_addition_chain_computes_progenitor(P):
    fp = derive(P)
    prog = emit.addition_chain(fp.pe)
    rng = random.Random(1)
    for _ in range(4):
        x = rng.randrange(2, fp.p)
        assert emit.eval_chain(prog, x, fp.p) == pow(x, fp.pe, fp.p)
    sq, mu = emit.chain_cost(prog)
    assert sq <= fp.pe.bit_length()               # squarings == bit length - 1: the leading run ladder is the main chain
    if not P.endswith("Q") and P not in ("BP256", "TWEEDLE", "SIDH434", "SIDH503", "SIDH610", "SIDH751", "MFP4", "MFP7", "MFP1973", "CSIDH512", "M607"):
        assert mu <= 20                           # shaped primes: long runs of ones; general primes take the loop form


def test_generated_headers_are_current():
    """csrc/generated/params_*.h in the tree equal what the driver emits now"""
    for P in emit.BUILT_PRIMES:
        path = os.path.join(emit.GEN_DIR, "params_%s.h" % P)
        assert os.path.exists(path), "run python -m modarith_amd.emit"
        assert open(path).read() == emit.header_text(derive(P))


def test_limb_split_roundtrip():
    for P in ALL:
        fp = derive(P)
        for x in (0, 1, fp.p - 1, fp.p, 2 * fp.p - 1):
            assert fp.from_limbs(fp.to_limbs(x)) == x


def test_split_proofs_per_prime():
    """emit.split_point / chain_ok: the three-accumulator cut positions the kernels were tuned with stay what they were, and the two
    primes that had no provable cut under the dense count of 2N column terms (ED500, SIDH503: Montgomery primes with ndash = 1 whose
    limbs are mostly 0 / -1 / powers of two, which never enter the accumulators -- field.h monty_reduce) get one from the per-prime
    count (emit.sparse_terms); a bound check of that count against the worst column redone here"""
    from modarith_amd import emit
    from modarith_amd.params import derive
    # every built modulus (generated from a run of the driver, kept as literals: a change of any prime's cut shows up in review)
    want = {"X25519": (28, True), "NIST256": (27, True), "X448": (29, True), "NIST521": (0, False), "PM266": (0, False), "PM383": (28, False),
            "NUMS256W": (0, False), "NIST384": (29, True), "NIST224": (29, True), "SECP256K1M": (27, True), "NIST256Q": (27, True),
            "ED25519Q": (26, True), "ED448Q": (29, True), "C2065": (28, True), "PM336": (30, False), "PM512": (29, False), "GM270": (28, True),
            "GM240": (0, False), "GM360": (29, False), "GM480": (0, False), "GM384": (0, False), "GM512": (0, False), "TWEEDLE": (27, True),
            "SIDH434": (28, True), "SIDH503": (29, False), "SECP256K1": (27, False), "C41417": (0, False), "ED248": (26, True), "ED376": (28, True),
            "ED500": (29, False), "SIDH610": (29, False), "SIDH751": (0, False), "MFP4": (27, True), "MFP7": (27, True), "MFP1973": (27, True),
            "CSIDH512": (0, False), "GM378": (28, True), "PM383M": (0, False), "PM266M": (0, False), "PM336M": (0, False), "C41417M": (0, False),
            "PM512M": (0, False), "M607": (0, False), "2519": (29, False), "1305": (24, True), "BP256": (27, True), "M2519": (0, False)}
    assert sorted(want) == sorted(ALL)
    derive = globals()["derive"]                                # (the module's: built-in and generated moduli alike)
    for name, (h, chain) in want.items():
        fp = derive(name)
        assert (emit.split_point(fp), emit.chain_ok(fp)) == (h, chain), name
    for name in ("ED500", "SIDH503"):
        fp = derive(name)
        n, H, W = emit.sparse_terms(fp), emit.split_point(fp), fp.radix + 2
        big = [v for i, v in enumerate(fp.ppw) if i > 0 and v not in (0, 1, -1) and v & (v - 1)]
        assert n == fp.nlimbs + len(big) + 1 and 2 * fp.nlimbs > n            # sparse indeed: fewer terms than the dense count
        lo, hi = (1 << H) - 1, (1 << (W - H)) - 1                              # halves of a limb below 2^W
        assert n * lo * lo < 1 << 64 and n * 2 * lo * hi < 1 << 64 and n * hi * hi < 1 << 64
        assert all(0 < v < 1 << fp.radix for v in big)                         # the prime limbs themselves are narrower than a limb
    assert emit.sparse_terms(derive("NIST384")) is None                        # ndash != 1: the dense count stands


# ---------------------------------------------------------------- accumulator bounds, recomputed from the column structure of csrc/field.h
class _Col:
    """upper bounds of the three 64-bit accumulators of field.h Wide<true, H>::Col / ::Acc after a sequence of mac() calls whose operands are
    only known to be <= x and <= y: an operand cut at H has a low half up to min(x, 2^H - 1) and a high half up to x >> H (a uint32)"""

    def __init__(self, H):
        self.H, self.s0, self.s1, self.s2 = H, 0, 0, 0

    def halves(self, x):
        lo, hi = min(x, (1 << self.H) - 1), x >> self.H
        assert hi < 1 << 32, "the high half of an operand does not fit Opd::hi"
        return lo, hi

    def mac(self, x, y, exact_y=False):
        xl, xh = self.halves(x)
        yl, yh = (y & ((1 << self.H) - 1), y >> self.H) if exact_y else self.halves(y)      # a compile-time constant: its very halves
        assert yh < 1 << 32
        self.s0 += xl * yl
        self.s1 += xl * yh + xh * yl
        self.s2 += xh * yh

    def check(self, where):
        for k in ("s0", "s1", "s2"):
            assert getattr(self, k) < 1 << 64, "%s: %s reaches 2^%.2f" % (where, k, __import__("math").log2(getattr(self, k)))


def _half_limb_form(fp):
    """the primes whose FAST products are one of field.h's half-limb forms (HALF, HALF_OV, MHALF, MHALF_TRI: the predicates of field.h)"""
    R, N = fp.radix, fp.nlimbs
    if fp.family == "pseudo":
        half = fp.epm and not fp.overflow and fp.fred and R == 51 and N == 5 and fp.mm == 19
        half_ov = R == 52 and N == 5 and not fp.epm and fp.overflow and (fp.mm >> 36) == 1 and (fp.mm & 0xfffffffff) < (1 << 16)
        return half or half_ov
    neg = [i for i, v in enumerate(fp.ppw) if i > 0 and v == -1]
    mhalf = fp.ndash == 1 and not fp.E and not neg and R == 52 and N == 5 and fp.ppw[0] == -1
    tri = fp.ndash == 1 and fp.E and R == 56 and N == 8 and fp.ppw == [-1, 0, 0, 0, -1, 0, 0, 0, 1]
    return mhalf or tri


def _chain_digit(t, c, R, where):
    """Wide::Acc::digit(): lo = s0 + ((s1 mod 2^(R-H)) << H) + c in ONE word, c' = (lo >> R) + (s1 >> (R-H)) + (s2 << (2H-R))"""
    H = t.H
    assert R - H <= 32 and R <= 2 * H < 64, where
    lo = t.s0 + (((1 << (R - H)) - 1) << H) + c
    assert lo < 1 << 64 and c + t.s0 + (1 << R) < 1 << 64, "%s: c + s0 + 2^R reaches 2^%.2f" % (where, __import__("math").log2(c + t.s0 + (1 << R)))
    c2 = (lo >> R) + (t.s1 >> (R - H)) + (t.s2 << (2 * H - R))
    assert c2 < 1 << 64, where
    return c2


@pytest.mark.parametrize("P", ALL)
def test_accumulators_stay_below_2_64(P):
    """For every prime with SPLIT > 0: the largest value each 64-bit accumulator (s0, s1, s2; on the column chain also c + s0 + 2^R and the
    carry word) can reach, in every column of the product loops of csrc/field.h, when every operand limb is 2^(Radix+2) - 1 and every reduction
    digit 2^Radix - 1 -- recomputed here with Python integers from the prime's limbs (fp.ppw, fp.mm) and the loops of field.h (pm_modmul /
    pm_modsqr and their _chain forms; monty_mul<SQR> + monty_reduce + monty_digit and monty_mul_chain + monty_reduce_chain), not from emit.py's
    closed formulas.  Operands that field.h widens before the cut (mm * a, 2 * a: one word) are taken at their widened bound.
    The half-limb forms (HALF: X25519; HALF_OV: SECP256K1; MHALF: NIST256, MFP4, MFP7, MFP1973; MHALF_TRI: X448) have columns of their own
    (2N half columns, early-wrapped terms, folded digits) that this transcription does not cover with confidence: they are left to the
    arithmetic comparison at the budget's edge (tests/test_fast_products_host.py, tests/test_gpu_edge_products.py).  Their cut position is still
    what monty_mul / pm_modmul would need, and is checked as such where the dense form is provable."""
    fp = derive(P)
    H = emit.split_point(fp)
    if H == 0:
        assert not emit.chain_ok(fp)
        return
    R, N = fp.radix, fp.nlimbs
    L, D, W64 = (1 << (R + 2)) - 1, (1 << R) - 1, (1 << 64) - 1
    chain = emit.chain_ok(fp) and not _half_limb_form(fp)
    if fp.family == "pseudo":
        if _half_limb_form(fp):
            return                                               # (docstring)
        MA, TA = min(L * fp.mm, W64), min(2 * L, W64)
        for sqr in (False, True):
            c = 0
            for row in range(N):
                hk0 = row + 1
                hpairs, lpairs = (N - 1 - hk0 + 1) // 2, (row + 1) // 2
                where = "%s %s row %d" % (P, "pm_modsqr" if sqr else "pm_modmul", row)
                if fp.epm:
                    col = _Col(H)
                    if not sqr:
                        for _ in range(N - 1 - row):
                            col.mac(MA, L)
                        for _ in range(row + 1):
                            col.mac(L, L)
                    else:
                        for _ in range(hpairs):
                            col.mac(MA, TA)
                        if (N - hk0) % 2 == 1:
                            col.mac(MA, L)
                        for _ in range(lpairs):
                            col.mac(L, TA)
                        if row % 2 == 0:
                            col.mac(L, L)
                    col.check(where)
                    if chain:
                        c = _chain_digit(col, c, R, where)
                else:
                    assert not chain
                    parts = ([N - 1 - row, row + 1] if not sqr else [hpairs, 1 if (N - hk0) % 2 == 1 else 0, lpairs, 1 if row % 2 == 0 else 0])
                    for cnt in parts:                            # Col hi / col; cross / sq: an accumulator set each
                        col = _Col(H)
                        for _ in range(cnt):
                            col.mac(L, L)
                        col.check(where)
        return
    assert not fp.pm
    ppw = fp.ppw
    LMAX = JMAX = N if fp.E else N - 1
    NCOL = 2 * N if fp.E else 2 * N - 1
    neg = [i for i, v in enumerate(ppw) if i > 0 and v == -1]
    NEG = neg[0] if neg else 0
    Q = 1 << R
    for sqr in (False, True):
        c = 0
        for colno in range(NCOL):
            lo, hi = (0, colno) if colno < N else (colno - (N - 1), N - 1)
            cnt = max(hi - lo + 1, 0)
            where = "%s monty_mul<%s> column %d" % (P, "SQR" if sqr else "MUL", colno)
            acc = _Col(H)
            if not sqr:
                for _ in range(cnt):
                    acc.mac(L, L)
            else:
                cross = _Col(H)
                for _ in range(cnt // 2):
                    cross.mac(L, L)
                cross.check(where + " cross")
                if chain:                                        # Acc::add_twice
                    acc.s0, acc.s1, acc.s2 = 2 * cross.s0, 2 * cross.s1, 2 * cross.s2
                if cnt and colno % 2 == 0:
                    acc.mac(L, L)
            words = 0                                            # one-word terms of this column (the carry word c of the chain)
            scratch = NEG > 0 and colno > NEG
            s = D
            for l in range(1, LMAX + 1):
                j = colno - l
                if not (0 <= j <= JMAX and j < colno):
                    continue
                d = ppw[l]
                if d > 1:
                    if chain or d & (d - 1):                     # monty_reduce shifts a power of two into t; the chain multiplies by it
                        acc.mac(D, d, exact_y=True)
                elif d == 1:
                    s, words = (s + D, words) if scratch else (s, words + D)
                elif d == -1:
                    words += 0 if scratch else Q
                else:
                    assert d == 0
            if scratch:
                words += s
            if colno <= JMAX and fp.ndash != 1:
                assert ppw[0] > 0
                if ppw[0] == 1:
                    words += D
                elif chain:
                    acc.mac(D, ppw[0], exact_y=True)
                else:
                    c0 = _Col(H)                                 # monty_digit: a Col of its own
                    c0.mac(D, ppw[0], exact_y=True)
                    c0.check(where + " digit")
            acc.check(where)
            if chain:
                assert c + words < 1 << 64
                c = _chain_digit(acc, c + words, R, where)
