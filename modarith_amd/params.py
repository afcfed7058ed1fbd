"""Per-prime parameter driver: prime -> radix, limb count and every constant the HIP kernels need.

This is the build's counterpart of the parameter blocks of the reference generators
(pseudo.py:124-147 + 1561-1678 for 2^n-c primes, monty.py:151-298 + 2129-2253 for Montgomery-form
primes).  It derives the same quantities from first principles so that the limb layout and the
non-canonical (< 2p) results of the kernels are bit-identical to the reference's generated field.c:

  pseudo-Mersenne : n, Radix, Nlimbs, xcess, m, mm = m*2^xcess, TW, and the variant flags
                    overflow / fred ("tighter reduction") / EPM / carry_on
  Montgomery      : Radix (with the "excess >= 2 or virtual limb" rule), signed prime limbs ppw[]
                    (2^Radix-1 rewritten to -1 with a carry), virtual-limb flag E, R, ndash,
                    R^2 mod p limbs (the nres constant), trinomial index
  both            : Nbytes, PM1D2 (2-adicity of p-1), PE (progenitor exponent), root of unity.

tests/test_params.py checks every value against the macro block / constants captured from the
reference (tests/golden/field_*.json "params").  The word length is a parameter of the derivation, as it is the first argument
of the reference generators: 64 (the default: u64 limbs with u128 column accumulators, SURVEY 8 sizes, every built prime) or 32
(u32 limbs with u64 columns, the form of simd/pseudo_cuda.py's field.cu; built for the three BASELINE primes, emit.W32_PRIMES;
tests/test_params_w32.py checks those against tests/golden/field_w32_*.json "params").
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional

WL = 64                     # the default word length

# named primes of the hot-path configs (pseudo.py:1498-1548, monty.py:1966-2062) + a few neighbours
NAMED = {
    "X25519": (2**255 - 19, "pseudo"),
    "ED25519": (2**255 - 19, "pseudo"),
    "NIST256": (2**256 - 2**224 + 2**192 + 2**96 - 1, "monty"),
    "X448": (2**448 - 2**224 - 1, "monty"),
    "ED448": (2**448 - 2**224 - 1, "monty"),
    "NIST384": (2**384 - 2**128 - 2**96 + 2**32 - 1, "monty"),
    "NIST224": (2**224 - 2**96 + 1, "monty"),
    "PM266": (2**266 - 3, "pseudo"),
    "C2065": (2**206 - 5, "pseudo"),
    "PM336": (2**336 - 3, "pseudo"),
    "PM383": (2**383 - 187, "pseudo"),
    "NUMS256W": (2**256 - 189, "pseudo"),
    "NIST521": (2**521 - 1, "pseudo"),
    # secp256k1: curve.py:190-198 takes pseudo.py's field at 64 bits (the split-high-part "overflow" form,
    # pseudo.py:1640-1657); monty.py's flavour of the same prime is kept under the key SECP256K1M
    "SECP256K1": (2**256 - 2**32 - 977, "pseudo"),
    "SECP256K1M": (2**256 - 2**32 - 977, "monty"),
    "C41417": (2**414 - 17, "pseudo"),
    # the same pseudo-Mersennes as monty.py builds them when asked (monty.py:2010-2042 names them too): PM383 / PM266 / PM336 in
    # its "exploitable pseudo-Mersenne" form (PM = True, monty.py:700-870), C41417 / PM512 as ordinary full-Montgomery primes
    "PM383M": (2**383 - 187, "monty"),
    "PM266M": (2**266 - 3, "monty"),
    "PM336M": (2**336 - 3, "monty"),
    "C41417M": (2**414 - 17, "monty"),
    "PM512M": (2**512 - 569, "monty"),
    # a 607-bit Mersenne prime: the only kind of modulus that takes pseudo.py's bad_overflow forms at 64 bits (601-610 bits)
    "M607": (2**607 - 1, "pseudo"),
    # the fields of curve.py's ED248 / ED376 / ED500 (monty.py:2095-2102)
    "ED248": (5 * 2**248 - 1, "monty"),
    "ED376": (65 * 2**376 - 1, "monty"),
    "ED500": (27 * 2**500 - 1, "monty"),
    # further named moduli of monty.py's list (monty.py:1990-2075)
    "GM270": (2**270 - 2**162 - 1, "monty"),
    "GM240": (2**240 - 2**183 - 1, "monty"),
    "GM360": (2**360 - 2**171 - 1, "monty"),
    "GM480": (2**480 - 2**240 - 1, "monty"),
    "GM384": (2**384 - 2**186 - 1, "monty"),
    "GM512": (2**512 - 2**127 - 1, "monty"),
    "GM378": (2**378 - 2**324 - 1, "monty"),
    "PM512": (2**512 - 569, "pseudo"),
    "TWEEDLE": (0x40000000000000000000000000000000038aa127696286c9842cafd400000001, "monty"),
    "SIDH434": (2**216 * 3**137 - 1, "monty"),
    "SIDH503": (2**250 * 3**159 - 1, "monty"),
    # the larger isogeny / MFP moduli of the same list (monty.py:2067-2105), round 3
    "SIDH610": (2**305 * 3**192 - 1, "monty"),
    "SIDH751": (2**372 * 3**239 - 1, "monty"),
    "MFP4": (3 * 67 * 2**246 - 1, "monty"),
    "MFP7": (2**145 * 3**9 * 59**3 * 311**3 * 317**3 * 503**3 - 1, "monty"),
    "MFP1973": (0x34e29e286b95d98c33a6a86587407437252c9e49355147ffffffffffffffffff, "monty"),
    "CSIDH512": (5326738796327623094747867617954605554069371494832722337612446642054009560026576537626892113026381253624626941643949444792662881241621373288942880288065659, "monty"),
    # group orders (curve.py:324-329 runs monty.py on "00<decimal q>"): general primes, full Montgomery
    "NIST256Q": (0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551, "monty"),
    "ED25519Q": (0x1000000000000000000000000000000014DEF9DEA2F79CD65812631A5CF5D3ED, "monty"),
    "ED448Q": ((2**448 - 2**224 - 1 + 1 - 28312320572429821613362531907042076847709625476988141958474579766324) // 4, "monty"),
}

# per-name radix choices the generators hard-wire for 64-bit words (monty.py:2002-2037, `if WL==64: base=...`)
RADIX_64 = {"GM240": 61, "GM360": 57, "GM480": 60, "GM384": 62, "GM512": 58, "MFP4": 52, "MFP7": 52, "MFP1973": 52, "PM512M": 58}

# ... and for 32-bit words (monty.py:2000-2037 `if WL==32: base=29` for the GM primes -- GM480 and GM512 get 29 from the default rule
# too --, pseudo.py:1507-1510 for NIST521): without them the default rule gives GM240 27, GM360 and GM384 28 bits
RADIX_32 = {"GM240": 29, "GM360": 29, "GM480": 29, "GM384": 29, "GM512": 29, "NIST521": 29}

# keys of NAMED that are not the generators' own spelling
REFERENCE_NAME = {"SECP256K1M": "SECP256K1", "PM383M": "PM383", "PM266M": "PM266", "PM336M": "PM336", "C41417M": "C41417", "PM512M": "PM512",
                  "M607": "2**607-1"}

# how each built name is spelled on the reference generators' command line (group orders: "00" + decimal)
def reference_argv(name: str):
    p, fam = NAMED[name]
    script = "pseudo.py" if fam == "pseudo" else "monty.py"
    if name.endswith("Q"):
        return script, "00" + str(p)
    return script, REFERENCE_NAME.get(name, name)


@dataclass
class FieldParams:
    name: str
    family: str                 # "pseudo" | "monty"
    p: int
    n: int                      # bit length of p                      (Nbits)
    radix: int                  # limb width in bits                   (Radix)
    nlimbs: int                 # number of u64 limbs                  (Nlimbs)
    xcess: int                  # nlimbs*radix - n
    nbytes: int                 # ceil(n/8)                            (Nbytes)
    pm1d2: int                  # 2-adicity of p-1
    pe: int                     # progenitor exponent (p-1-e)/(2e), e = 2^pm1d2
    roi: List[int]              # non-trivial root of unity, limbs (plain integer form)
    # pseudo-Mersenne only
    m: int = 0                  # 2^n - p
    mm: int = 0                 # m * 2^xcess  (fold multiplier)
    tw: int = 0                 # top word of p in limb nlimbs-1 (as added by caddp)
    overflow: bool = False
    bad_overflow: bool = False  # pseudo.py:1646-1648: the carried high part of the overflow form needs a double word
    fred: bool = False
    epm: bool = False
    carry_on: bool = False
    # Montgomery only
    ppw: List[int] = field(default_factory=list)   # signed prime limbs (+ virtual limb if E)
    E: bool = False
    R: int = 1
    ndash: int = 1
    r2: List[int] = field(default_factory=list)    # R^2 mod p, limbs (nres multiplier)
    trin: int = 0
    pm: bool = False            # monty.py's PM form: an exploitable pseudo-Mersenne given to monty.py (ppw[0] = -m)
    # derived for both families: non-zero prime limbs as (index, sign, magnitude) with the virtual
    # limb folded into limb nlimbs-1 as +2^radix (caddp/addp/subp: pseudo.py:202-220, monty.py:301-349)
    pp: List[tuple] = field(default_factory=list)
    wl: int = 64                # word length the derivation was made for (spint = u64 | u32)

    @property
    def montgomery(self) -> bool:
        return self.family == "monty"

    def to_limbs(self, x: int, masked_top: bool = False) -> List[int]:
        """integer -> limbs; top limb takes everything left unless masked_top (pseudo.py:1769-1775)."""
        b = 1 << self.radix
        out = []
        for _ in range(self.nlimbs - 1):
            out.append(x % b)
            x >>= self.radix
        out.append(x % b if masked_top else x)
        return out

    def from_limbs(self, limbs) -> int:
        return sum(int(v) << (self.radix * i) for i, v in enumerate(limbs))


def _bits(x: int) -> int:
    return x.bit_length()


def _makebig(x: int, radix: int, n: int) -> List[int]:
    return [(x >> (radix * i)) & ((1 << radix) - 1) for i in range(n)]


def _two_adic(p: int):
    q, k = p - 1, 0
    while q % 2 == 0:
        q //= 2
        k += 1
    e = 1 << k
    return k, (p - 1 - e) // (2 * e)


def _root_of_unity(p: int, k: int) -> int:
    if k == 1:
        return p - 1
    if k == 2:
        return pow(2, (p - 1) // 4, p)
    qnr = 2
    while pow(qnr, (p - 1) // 2, p) == 1:
        qnr += 1
    return pow(qnr, (p - 1) >> k, p)


# ------------------------------------------------------------------ pseudo-Mersenne (2^n - m)
def _pm_radix(n: int, WL: int = WL) -> int:
    """smallest limb count whose worst-case column sum fits 2*WL bits, radix <= WL-3
    (rule of pseudo.py:124-140)."""
    limbs = n // WL
    while True:
        limbs = max(limbs + 1, 2)
        radix = WL // 2
        while limbs * radix < n:
            radix += 1
        if radix > WL - 3:
            continue
        if limbs * ((1 << radix) - 1) ** 2 < 1 << (2 * WL):
            return radix


def derive_pseudo(name: str, p: int, radix: Optional[int] = None, wl: int = WL) -> FieldParams:
    WL = wl
    n = p.bit_length()
    if n < 120 or pow(3, p - 1, p) != 1:
        raise ValueError("not a sensible modulus")
    radix = radix or _pm_radix(n, WL)
    m = (1 << n) - p
    b = 1 << radix
    if m >= b:
        raise ValueError("not an exploitable pseudo-Mersenne; use the Montgomery family")
    N = -(-n // radix)
    xcess = N * radix - n
    mm = m << xcess
    if mm >= 1 << (WL - 1):
        raise ValueError("excess too large for this radix")
    tw = b if n % radix == 0 else 1 << (n % radix)
    overflow = (b - 1) * (b - 1) * mm * N >= 1 << (2 * WL)
    bad_overflow = overflow and (N - 1) * (b - 1) ** 2 >= 1 << (2 * WL - 3)      # pseudo.py:1646-1648 (no Karatsuba at 64 bits)
    fred = _bits(N + 1) + radix + _bits(mm) < WL
    epm = (not overflow) and mm * (b - 1) < 1 << WL
    carry_on = m * ((1 << (2 * WL - radix + xcess)) + (1 << (radix - xcess))) >= 1 << (2 * radix)
    k, pe = _two_adic(p)
    fp = FieldParams(name=name, family="pseudo", p=p, n=n, radix=radix, nlimbs=N, xcess=xcess,
                     nbytes=-(-n // 8), pm1d2=k, pe=pe, roi=_makebig(_root_of_unity(p, k), radix, N),
                     m=m, mm=mm, tw=tw, overflow=overflow, bad_overflow=bad_overflow, fred=fred, epm=epm, carry_on=carry_on, wl=WL)
    fp.pp = [(0, -1, m), (N - 1, +1, tw)]
    return fp


# ------------------------------------------------------------------ Montgomery, shape-aware
def _signed_limbs(p: int, radix: int, N: int, pm_m: int = 0):
    """rewrite limbs equal to 2^radix-1 as -1 with a carry into the next limb; a carry out of the
    top limb becomes a virtual extra limb (process_prime, monty.py:258-298).  pm_m = m for the PM form: a low limb
    2^radix - m becomes -m, with the same carry (monty.py:284-288)."""
    b = 1 << radix
    pw = _makebig(p, radix, N)
    out, carry = [], 0
    for i in range(N):
        v = pw[i] + carry
        if pm_m and i == 0:
            if v == b - pm_m:
                v, carry = -pm_m, 1
            out.append(v)
            continue
        if carry:
            if v == b - 1:
                v = -1                      # carry stays 1
            elif v == b:
                v, carry = 0, 1
            else:
                carry = 0
        elif v == b - 1:
            v, carry = -1, 1
        out.append(v)
    if carry:
        out.append(1)
    return out, bool(carry)


def _monty_radix(p: int, n: int, WL: int = WL) -> int:
    """default radix rule of monty.py:151-173: at least two spare bits in the top limb, or none at
    all together with a virtual limb."""
    limbs = n // WL
    while True:
        limbs = max(limbs + 1, 2)
        radix = WL // 2

        def bump(r):
            while limbs * r < n or r - (n % r) < 2:
                r += 1
            return r
        radix = bump(radix)
        if n % radix == 0:
            _, E = _signed_limbs(p, radix, limbs)
            if not E:
                radix += 1
        radix = bump(radix)
        if radix > WL - 3:
            continue
        if limbs * ((1 << radix) - 1) ** 2 < 1 << (2 * WL):
            return radix


def _trinomial(p: int, radix: int) -> int:
    """p = 2^n - 2^k - 1 with k a multiple of the radix -> k/radix, else 0 (monty.py:231-243)."""
    n = p.bit_length()
    m = (1 << n) - p - 1
    k = 20
    while k < n:
        if 1 << k > m:
            return 0
        if 1 << k == m:
            break
        k += 1
    else:
        return 0
    return k // radix if k % radix == 0 else 0


def derive_monty(name: str, p: int, radix: Optional[int] = None, wl: int = WL) -> FieldParams:
    WL = wl
    n = p.bit_length()
    if n < 120 or pow(3, p - 1, p) != 1:
        raise ValueError("not a sensible modulus")
    radix = radix or _monty_radix(p, n, WL)
    b = 1 << radix
    N = -(-n // radix)
    xcess = N * radix - n
    m = (1 << n) - p
    pm = m > 1 and _bits(m) + radix < WL               # "Exploitable Pseudo Mersenne detected" (monty.py:2151-2156)
    ppw, E = _signed_limbs(p, radix, N, m if pm else 0)
    if sum(1 for i, v in enumerate(ppw) if i > 0 and v == -1) > 1:
        raise ValueError("too many -1 limbs (monty.py:2217-2219)")
    if xcess < 2 and not E:
        raise ValueError("excess is only one bit; change the radix")
    R = 1 << (radix * (N + (1 if E else 0)))
    ndash = pow((R - p) % b, -1, b)
    k, pe = _two_adic(p)
    fp = FieldParams(name=name, family="monty", p=p, n=n, radix=radix, nlimbs=N, xcess=xcess,
                     nbytes=-(-n // 8), pm1d2=k, pe=pe, roi=_makebig(_root_of_unity(p, k), radix, N),
                     m=m, ppw=ppw, E=E, R=R, ndash=ndash, r2=_makebig(R * R % p, radix, N),
                     trin=_trinomial(p, radix), pm=pm, wl=WL)
    pp = [(i, -1 if v < 0 else +1, abs(v)) for i, v in enumerate(ppw[:N]) if v]
    if E:
        # fold +1 * 2^(radix*N) into limb N-1 as +2^radix
        # (a negative top limb, GM378's -1 at limb N-1, joins it: -x + x*q = x*(q-1) in the 64-bit arithmetic of
        # caddp / addp / subp, monty.py:301-349)
        pp = [t for t in pp if t[0] != N - 1] + [(N - 1, +1, ppw[N - 1] + b)]
    fp.pp = pp
    return fp


def derive(name: str, family: Optional[str] = None, radix: Optional[int] = None, wl: int = WL) -> FieldParams:
    """FieldParams for a named prime (or a python expression such as '2**255-19') at word length wl (64 | 32)."""
    if wl not in (32, 64):
        raise ValueError("word length must be 64 or 32")
    if name in NAMED:
        p, fam = NAMED[name]
    else:
        p, fam = int(eval(name, {"__builtins__": {}})), None
    fam = family or fam
    if fam is None:
        n = p.bit_length()
        fam = "pseudo" if ((1 << n) - p) < (1 << 32) else "monty"
    if radix is None and fam == "monty" and wl == 64:
        radix = RADIX_64.get(name)
    if radix is None and wl == 32:
        radix = RADIX_32.get(name)
    if wl == 32 and fam == "pseudo" and family is None and name in NAMED and ((1 << p.bit_length()) - p) >> _pm_radix(p.bit_length(), 32):
        # a named prime whose 2^n - m does not fit a limb of this word length is not a pseudo-Mersenne there: pseudo.py names
        # SECP256K1 for 64-bit words only (pseudo.py:1547 `and WL==64`), `monty.py 32 SECP256K1` builds it (monty.py:2061)
        fam = "monty"
    return derive_pseudo(name, p, radix, wl) if fam == "pseudo" else derive_monty(name, p, radix, wl)


def w32_inv_in_contract(fp: FieldParams, limbs):
    """The in-contract predicate of the 32-bit simultaneous inversion (csrc/kernels.h inv_in_contract, where it is justified): digit
    form below 2^(Nbits+1) -- limbs 0..N-2 below 2^Radix, top limb below 2^(Nbits + 1 - Radix (N-1)).  Elements that pass share an
    inversion with their neighbours in modinv_<P>_w32_batch; the others get one of their own.  Every element below 2p in digit form
    passes.  `limbs`: one element (N unsigned limbs) -> bool, or a limb-major batch [N, n] -> one bool per element."""
    import numpy as np
    if fp.wl != 32:
        raise ValueError("the predicate belongs to the 32-bit word form")
    N, R = fp.nlimbs, fp.radix
    topb = fp.n + 1 - R * (N - 1)
    a = np.asarray(limbs, dtype=np.uint64)
    if a.shape[0] != N:
        raise ValueError("expected %d limbs" % N)
    ok = ((a[:N - 1] >> np.uint64(R)) == 0).all(axis=0) & ((a[N - 1] >> np.uint64(topb)) == 0)
    return bool(ok) if a.ndim == 1 else ok


def w32_inv_closure(fp: FieldParams) -> dict:
    """The proof that goes with w32_inv_in_contract, computed: is "digit form below 2^(Nbits+1)" closed under the products of the
    32-bit word form of this prime?  It is what the comment above inv_in_contract in csrc/kernels.h works out by hand for X25519,
    NIST256 and X448, as interval arithmetic over the statements of csrc/field.h at MA_WL = 32 (pm_modmul + pm_second_pass,
    monty_mul + monty_reduce + monty_digit), which are identities over the integers as long as no 64-bit column and no 32-bit word
    wraps; so only sizes are shown.  Operand set W: limbs 0..N-2 at most 2^Radix - 1 -- plus `slack` on the one limb a
    pseudo-Mersenne second pass leaves unmasked (limb 1, limb 2 with carry_on) --, top limb below 2^TOPB, TOPB = Nbits + 1 -
    Radix (N-1).  Shown, with both operands anywhere in W:
      * products per column, with the top-limb slack and the unmasked limb;
      * pseudo-Mersenne: the fold by mm -- the pre-multiplied limbs of the EPM form fit a word; the overflow form's carried high
        part fits a word and lo + hi does not wrap; or mm times the folded sum fits the double word -- then the carries and the second
        pass (its word or double-word form), whose carry into the unmasked limb must not exceed the slack assumed (the least fixed
        point is taken) and whose output must stay below 2p;
      * Montgomery: the digit-times-prime-limb terms (shifted digits for powers of two, one word for +-1 limbs, the scaled borrow of
        monty.py's PM form), with the digit-times-p0 product where ndash != 1, the carries, and (a b + q p) / R < 2p for a, b below
        2^(Nbits+1) -- which needs R >= 2^(Nbits+3) or so: three spare bits, or the virtual limb.
    The squarings (pm_modsqr, monty_mul<true>) add the same products column by column -- twice the cross terms, `tot *= 2`, then the
    square -- so every partial sum there is at most the column bound shown for the product of two operands of W.
    -> {"closed": bool, "column": largest column sum found, "column_bits": its log2, "slack": carry into the unmasked limb,
        "topb": TOPB, "hi": largest carried high part of the overflow form (0 elsewhere), "why": the first bound that failed or ""}.
    closed = False is a statement about this proof, not about the prime: such a field keeps one inversion per element."""
    import math
    if fp.wl != 32:
        raise ValueError("the closure belongs to the 32-bit word form")
    N, R, n, p = fp.nlimbs, fp.radix, fp.n, fp.p
    Q, W64, W32 = 1 << R, 1 << 64, 1 << 32
    mask = Q - 1
    topb = n + 1 - R * (N - 1)
    out = {"closed": False, "column": 0, "column_bits": 0.0, "slack": 0, "topb": topb, "hi": 0, "why": ""}

    def fail(why):
        out["why"] = why
        return out

    def done(col, slack=0, hi=0):
        out.update(closed=True, column=col, column_bits=round(math.log2(col), 2), slack=slack, hi=hi)
        return out

    if not (0 < topb <= 29 and R <= 29):
        return fail("TOPB = %d, Radix = %d: the predicate is stated for at most 29 bits each" % (topb, R))
    top = (1 << topb) - 1
    if fp.family == "pseudo":
        if fp.bad_overflow:
            return fail("bad_overflow form")
        k = 2 if fp.carry_on else 1
        if k >= N - 1:
            return fail("too few limbs")
        slack = 0
        for _ in range(8):
            lim = [mask] * (N - 1) + [top]
            lim[k] += slack
            t = colmax = himax = hi_ov = 0
            for row in range(N):
                tt = sum(lim[j] * lim[N + row - j] for j in range(row + 1, N))
                col = sum(lim[j] * lim[row - j] for j in range(row + 1))
                if fp.epm:
                    if max(lim[1:]) * fp.mm >= W32:
                        return fail("a limb times mm leaves the word (EPM form)")
                    t += tt * fp.mm
                elif row < N - 1:
                    if tt >= W64:
                        return fail("folded column of row %d" % row)
                    if fp.overflow:
                        if row and mask + hi_ov >= W32:
                            return fail("lo + hi wraps in row %d" % row)
                        t += (mask + (hi_ov if row else 0)) * fp.mm
                        hi_ov = tt >> R
                        himax = max(himax, hi_ov)
                        if hi_ov >= W32:
                            return fail("carried high part of row %d leaves the word" % row)
                    else:
                        if tt * fp.mm >= W64:
                            return fail("mm times the folded column of row %d" % row)
                        t += tt * fp.mm
                t += col
                if fp.overflow and row == N - 1:
                    t += hi_ov * fp.mm
                if t >= W64:
                    return fail("column %d" % row)
                colmax = max(colmax, t)
                t >>= R
            # second pass: ut = m (2^xcess t + (v_top >> (Radix - xcess))), in a word (fred) or a double word
            ut = (t << fp.xcess) + ((mask >> (R - fp.xcess)) if fp.xcess else 0)
            ut *= fp.m
            if ut >= (W32 if fp.fred else W64):
                return fail("second pass: m (2^xcess t + top bits) leaves the %s" % ("word" if fp.fred else "double word"))
            carry = ((mask + min(ut, mask)) >> R) + (ut >> R)
            if fp.carry_on:                                    # (one more masked limb: the carry of limb 0 goes through limb 1)
                carry = ((mask + min(carry, mask)) >> R) + (carry >> R)
            if mask + slack + carry >= W32:
                return fail("second pass: carry into limb %d" % k)
            if carry <= slack:
                value = ((1 << (n - R * (N - 1))) - 1 << (R * (N - 1))) + sum((mask + (carry if i == k else 0)) << (R * i) for i in range(N - 1))
                if value >= 2 * p:
                    return fail("product output not below 2p")
                return done(colmax, slack, himax)
            slack = carry
        return fail("no fixed point for the unmasked limb")
    # Montgomery
    lim = [mask] * (N - 1) + [top]
    lmax = N if fp.E else N - 1
    ppw = list(fp.ppw) + [0] * (lmax + 1 - len(fp.ppw))
    if fp.ndash != 1 and not fp.pm and ppw[0] <= 0:
        return fail("full Montgomery reduction with a negative low limb")
    ncol = 2 * N if fp.E else 2 * N - 1
    neg = next((i for i, v in enumerate(ppw) if i > 0 and v == -1), 0)
    t = colmax = 0
    for c in range(ncol):
        if neg and c > neg:
            # monty_reduce's 32-bit scratch word of the columns past the negative limb: s = mask + (digits under +1 limbs) - (the digit
            # under the -1 limb).  It must not wrap upwards (the subtraction takes at most the mask it starts from)
            plus = sum(1 for l in range(1, lmax + 1) if ppw[l] == 1 and 0 <= c - l <= lmax and c - l < c)
            if mask * (1 + plus) >= W32:
                return fail("the scratch word of column %d: %d digits under +1 limbs on top of the mask" % (c, plus))
        lo, hi = (0, c) if c < N else (c - (N - 1), N - 1)
        t += sum(lim[j] * lim[c - j] for j in range(lo, hi + 1))
        if fp.pm and c >= 1:
            t += fp.m * mask
        for l in range(1, lmax + 1):
            j = c - l
            if 0 <= j <= lmax and j < c and ppw[l]:
                d = ppw[l]
                t += mask * d if d > 1 else Q              # (+-1 limbs: one word below 2^Radix, or the borrow word)
        if c <= lmax:
            if fp.ndash != 1:
                t += fp.m * Q if fp.pm else mask * ppw[0]
        if t >= W64:
            return fail("column %d" % c)
        colmax = max(colmax, t)
        t >>= R
    a = (1 << (n + 1)) - 1
    if a * a // fp.R + p >= 2 * p:
        return fail("(a b + q p) / R is not below 2p for a, b below 2^(Nbits+1): R = 2^%d leaves %d spare bits" % (fp.R.bit_length() - 1, fp.R.bit_length() - 1 - n))
    return done(colmax)
