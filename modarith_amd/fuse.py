"""Fused chains: a sequence of field.c calls per element compiled into ONE streaming kernel.

A C caller of the reference writes `modadd(x,y,t); modsub(x,y,w); modmul(t,w,s); modsqr(s,s); modinv(s,NULL,z);`
(the generators' acceptance chain, pseudo.py:1783-1796; the bodies of rfc7748.c:190-223, edwards.c:73-145) and the C
compiler keeps every intermediate in registers -- field.c's functions are `static inline`.  Batched over HBM-resident
arrays, the same five calls are five kernels and 520 bytes of traffic per element where 120 are needed (two arrays in,
one out): on a memory-bound engine the round trips are the whole cost.  This module gives the batched caller what the C
compiler gives the scalar one: the chain is written once with the reference's function names,

    ch = Chain("X25519", "accept")             # any built-in prime or generated tag
    x, y = ch.input(), ch.input()
    s = ch.modsqr(ch.modmul(ch.modadd(x, y), ch.modsub(x, y)))
    ch.output(ch.modinv(s))
    f = ch.build()                              # one hipcc unit (seconds), cached
    z, = f(xa, ya)                              # device batches, flat or tiled

and hipcc instantiates the same `Field<P>` functions the library's kernels are made of, back to back, on registers:
one load per input array, one store per output array, no LDS, no interpreter.  Limbs are those of the call-by-call
sequence, bit for bit (the same functions on the same limbs; `modinv` returns the library's normalised form).  The
product policy is the library's wave vote (csrc/kernels.h OpMulAuto), taken once on the inputs: inside the limb contract
the whole chain runs the split products -- every intermediate is a field-function output and stays inside it -- otherwise
the exact ones.  C-ABI of the built plug-in (modarith_amd/plugins/libmodarith_amd_chain_<name>_<TAG>.so):

    int chain_<name>_<TAG>_batch(const void *const *in, void *const *out, size_t n, size_t ld, void *stream);
    int chain_<name>_<TAG>_aos(const void *const *in, void *const *out, size_t n, void *stream);     /* element-major x[n][Nlimbs] */

The order of the arrays in `in` and `out` is stated once on each side: `Chain.layout()` below for Python (the Python call takes and
returns the arrays in that order; every check, the metadata record and the printed prototype derive from it), the header comment of
csrc/chain.inc for the entry points; docs/fused_chains.md points to both.
`ch.shared()` is an operand that is the same for every element of the batch -- a curve's d, a base point's coordinate, a blinding factor:
Nlimbs words on the host, read by the entry point before it returns and passed by value in the kernel arguments (wave-uniform: scalar
registers, no array to stream; a call under stream capture bakes the value in), at most 8 a chain; `ch.modint(k)`, `ch.modone()`, `ch.modzer()`
are the field's constants as Field<P>::modint / modone / modzer make them.  Operations: modmul modsqr modadd modsub modneg
modmli nres redc modcpy modinv modpro modsqrt modnsqr modhaf modcmv modcsw and the generic=False forms modadd_lazy modsub_lazy
modneg_lazy (one level of laziness between reductions, which is how rfc7748.c uses them).

A chain can decide (edwards.c:271, 313-325): `ch.modis0(a)`, `ch.modis1(a)`, `ch.modsign(a)`, `ch.modcmp(a, b)`, `ch.modqr(x, h=None)` are
Field<P>'s functions of those names and return a `Pred`, an int computed inside the chain; `ch.lnot(d)`, `ch.land(d, e)`, `ch.lor(d, e)`,
`ch.lxor(d, e)` are the reference's own `1 - d`, `d & e`, `d | e`, `d ^ e` on predicates and selectors -- defined for operands that are 0 or 1,
as they are there; `modcmv` / `modcsw` take a `Pred` where they take a selector (still lane predication: no branch, no `?:`, no loop on a
computed int); `ch.modsqrt(a, h)`, `ch.modinv(a, h)`, `ch.modqr(x, h)` pass the progenitor `h = ch.modpro(a)` where they pass NULL otherwise;
and `ch.output(p)` of a `Pred` is an int32 result of one entry per element (n contiguous entries, indexed by element for flat and tiled
batches alike, no alignment asked; it may be the array of a selector input: a lane reads its entries before it stores), and a chain may
have no other output: `oncurve_chain()` below reads two coordinate arrays and writes 4 bytes per element, `decompress_chain()` is
edwards.c:290-334 as one kernel.

A chain can speak bytes: `v, ok = ch.input_bytes()` is a byte-record input -- uint8 [n, Nbytes], big-endian, the layout of modimp_<P>_batch --
with v what Field.modimp leaves (the integer the bytes spell, modfsb, nres) and ok its return value as a `Pred` (1 where the integer was
below p); `ch.output_bytes(v)` is a byte-record output, modexp(v).  modimp and modexp then run inside the kernel: `c = a * b` on wire values
moves 96 bytes an element over X25519 where the four calls move 344.  Records are 8-byte aligned where Nbytes is a multiple of 8 (the
rule of modimp_<P>_batch) and may be anywhere otherwise; a byte output may be the array of a byte input.  A chain needs at least one element batch or one byte input: without
element arrays on either side `ld` is ignored.  There is no element-major entry for such a chain (`_aos` refuses).  `pubkey_chain()` below
checks an uncompressed P-256 public key as it arrives, 64 bytes in and 4 out.  docs/fused_chains.md, "Chains that speak bytes", has the
kernels' two ways to the bytes and their rates.

Records may be little-endian and carry a sign: `ch.input_bytes(little=True)` reads records least significant byte first (the RFC 7748 /
RFC 8032 wire formats, which the reference reverses on the host), `ch.input_bytes(sign=True)` returns (v, ok, s) with s the record's most
significant bit as an int of the chain, cleared before modfsb sees the integer (rfc7748.c:172's mask, RFC 8032's x_0);
`ch.output_bytes(v, little=True, sign=d)` writes such records, d << 7 OR-ed into the most significant byte.  Byte order and sign are
compile-time properties of each array (CHAIN_BIN_LE / CHAIN_BIN_SIGN / CHAIN_BOUT_LE / CHAIN_BOUT_SIGN, emitted only by a chain that
uses them); the bit moves in registers.  `rfc8032_decode_chain()`, `rfc8032_encode_chain()` and `edwards_to_montgomery_chain()` below are
written with them.  The rest of field.c: `ch.modshl(a, k)`, `v, r = ch.modshr(a, k)` (r: the bits shifted out), `ch.mod2r(r)`,
`v, f = ch.modfsb(a)`, `v, f = ch.flatten(a)`; modshl leaves the limb contract, so a 64-bit chain with one runs the exact products.
Out of scope: the 57-byte records of Ed448 (a record is Nbytes long), and prop, which is static.  docs/fused_chains.md, "Little-endian
records and sign bits" and "The rest of field.c".

Word length 32: `Chain(prime, name, wl=32)` is the same chain over the 32-bit word form of X25519, NIST256 and X448 (csrc/kernels32.h,
namespace ma32; int32 batches of `Field(prime, wl=32)`): what a port of the reference's per-thread CUDA form (simd/pseudo_cuda.py 32)
runs per element.  One product policy, so no vote; one, two or four elements per lane (the library's pick_ept rules), by default one
in workgroups of 256 (measured: profiles/w32_chain_rate.json, docs/fused_chains.md); every operation above except the generic=False forms, which that word length does not
offer, and no element-major entry (convert with modarith_amd_w32_aos_to_soa).  Symbol, library and object names carry `_w32`:

    int chain_<name>_<TAG>_w32_batch(const void *const *in, void *const *out, size_t n, size_t ld, void *stream);

Like the generator mode (modarith_amd/generate.py) this needs hipcc where the chain is built and has no CPU path.
"""
from __future__ import annotations

import ctypes
import os
import re
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

from . import _lib, emit
from . import generate as _gen
from .plugin import build_plugin

_NAME_RE = re.compile(r"^[A-Za-z][A-Za-z0-9_]*$")
# op -> (Field<P> function, operand count, takes an int immediate)
_OPS = {"modmul": 2, "modadd": 2, "modsub": 2, "modsqr": 1, "modneg": 1, "nres": 1, "redc": 1, "modcpy": 1, "modinv": 1, "modmli": 1,
        "modadd_lazy": 2, "modsub_lazy": 2, "modneg_lazy": 1, "modnsqr": 1, "modpro": 1, "modsqrt": 1, "modhaf": 1, "modcmv": 2, "modcsw": 2,
        "modint": 0, "modone": 0, "modzer": 0, "modshl": 1, "modshr": 1, "mod2r": 0, "modfsb": 1, "flatten": 1,
        "modis0": 1, "modis1": 1, "modsign": 1, "modcmp": 2, "modqr": 1, "lnot": 0, "land": 0, "lor": 0, "lxor": 0}
_HEAVY = ("modinv", "modpro", "modsqrt", "modqr")  # long exponentiation chains: one element per lane
_PREDS = ("modis0", "modis1", "modsign", "modcmp", "modqr")      # Field<P> functions that return an int: the result is a Pred
_INT_OPS = ("lnot", "land", "lor", "lxor")        # the plain C the reference writes on its 0/1 ints
_INT_RET = ("modshr", "modfsb", "flatten")        # in-place functions of field.c that return an int beside the element they leave: Op.sdst
# an operation as a line of body<F>, over the fields of its Op (h: the progenitor b, or nullptr); the rest: F::op(operands, result), by operand count
_CALLS = {"modcsw": "F::modcpy(v{a}, v{dst}); F::modcpy(v{b}, v{dst2}); F::modcsw(s{sa}, v{dst}, v{dst2});",
          "modcmv": "F::modcpy(v{b}, v{dst}); F::modcmv(s{sa}, v{a}, v{dst});",
          "modnsqr": "F::modcpy(v{a}, v{dst}); F::modnsqr(v{dst}, {imm});", "modhaf": "F::modcpy(v{a}, v{dst}); F::modhaf(v{dst});",
          "modsqrt": "F::modsqrt(v{a}, {h}, v{dst});", "modinv": "F::modinv(v{a}, {h}, v{dst}); inv_normalise<F>(v{dst});",
          "modqr": "s{dst} = F::modqr({h}, v{a});", "modmli": "F::modmli(v{a}, {imm}, v{dst});", "modint": "F::modint({imm}, v{dst});",
          "modshl": "F::modcpy(v{a}, v{dst}); F::modshl({imm}, v{dst});", "modshr": "F::modcpy(v{a}, v{dst}); s{sdst} = F::modshr({imm}, v{dst});",
          "mod2r": "F::mod2r({imm}, v{dst});", "modfsb": "F::modcpy(v{a}, v{dst}); s{sdst} = (int)F::modfsb(v{dst});",
          "flatten": "F::modcpy(v{a}, v{dst}); s{sdst} = (int)F::flatten(v{dst});",
          "lnot": "s{dst} = 1 - s{sa};", "land": "s{dst} = s{sa} & s{sb};", "lor": "s{dst} = s{sa} | s{sb};", "lxor": "s{dst} = s{sa} ^ s{sb};",
          0: "F::{op}(v{dst});", 1: "F::{op}(v{a}, v{dst});", 2: "F::{op}(v{a}, v{b}, v{dst});"}
_WITH_H = ("modinv", "modsqrt", "modqr")          # take an optional progenitor h = modpro(a)
_LAZY = ("modadd_lazy", "modsub_lazy", "modneg_lazy")
MAX_OPS = 256
MAX_SHARED = 8                                    # shared operands of a chain: they travel in the kernel arguments (csrc/chain.inc)
# 32-bit word form: elements per lane and workgroup size of a chain without an inversion.  Measured (tools/w32_chain_rate.py,
# profiles/w32_chain_rate.json: the four-call chain at 2^24 elements on tiles of 4096, share of the HBM peak over its own bytes): one
# element per lane in workgroups of 256 runs at 0.770 / 0.770 / 0.763-0.774 for X25519 / NIST256 / X448 against 0.760 / 0.780 / 0.732 at
# two and 0.728 / 0.752 / 0.697 at four elements per lane, workgroups of 128 behind 256 at every width -- the streaming kernels'
# shape, ahead for X25519 and X448 and 1.3 % behind two elements per lane for NIST256.  build(ept=, block=) overrides them
W32_EPT_DEFAULT = 1
# Byte records (input_bytes / output_bytes): which of the two ways to the bytes of csrc/chain.inc a call on 16-byte aligned record arrays
# takes, per word length.  Measured (tools/chain_bytes_rate.py, profiles/chain_bytes_rate.json, docs/fused_chains.md); the environment
# variable MA_CHAIN_BYTES=staged|direct overrides it at every call
BYTES_IO_DEFAULT = {64: "direct", 32: "direct"}
W32_BLOCK_DEFAULT = 256


class Val:
    """one element-valued intermediate of a chain (an SSA value: written once)"""
    def __init__(self, chain: "Chain", idx: int):
        self.chain, self.idx = chain, idx


class Sel:
    """a per-element int selector input of a chain"""
    def __init__(self, chain: "Chain", idx: int):
        self.chain, self.idx = chain, idx


class Pred:
    """an int-valued intermediate of a chain (0 / 1), computed inside it: the result of modis0 / modis1 / modsign / modcmp / modqr or of
    lnot / land / lor / lxor.  A selector of modcmv / modcsw, an operand of the int expressions, an int32 output.  Ints share one index
    space (s<k> in the emitted text): the selector inputs first, then the computed ones"""
    def __init__(self, chain: "Chain", idx: int):
        self.chain, self.idx = chain, idx


class Op(NamedTuple):
    """one operation of a chain.  Element values and ints are two index spaces (v<k> and s<k> in the emitted text); -1 = no such operand"""
    op: str
    dst: int                # what it defines: a value, or for the predicates and the int expressions an int
    a: int = -1             # element operands; b of modinv / modsqrt / modqr is the optional progenitor
    b: int = -1
    sa: int = -1            # int operands: of lnot / land / lor / lxor, and sa the selector of modcmv / modcsw
    sb: int = -1
    imm: int = 0            # the C int of modmli / modint / modnsqr / modshl / modshr / mod2r
    dst2: int = -1          # modcsw: the second value it defines
    sdst: int = -1          # modshr / modfsb / flatten: the int they return, beside the value dst


class BIn(NamedTuple):
    """one byte-record input"""
    v: int                  # the value modimp leaves
    ok: int                 # modimp's return value: its place among the computed ints
    little: bool = False    # byte 0 of a record is the least significant
    sign: int = -1          # the record's top bit, taken out of the integer: its place among the computed ints; -1 = the bit is part of the value


class BOut(NamedTuple):
    """one byte-record output"""
    v: int                  # the value
    t: int                  # the value that holds its redc
    little: bool = False
    sign: int = -1          # the int (of the int space) OR-ed into the record's top bit; -1 = none


class Chain:
    def __init__(self, prime: str, name: str, wl: int = 64):
        if not _NAME_RE.match(name):
            raise ValueError("chain name %r cannot be part of a C identifier" % (name,))
        if wl not in (64, 32):
            raise ValueError("word length must be 64 or 32 (got %r)" % (wl,))
        self.wl = wl
        found = _gen.find_field(prime, wl=wl, built=True)
        if found is None and wl == 32:
            raise ValueError("the 32-bit word form is built for %s (got %r) and generated for what `python -m modarith_amd.generate w32 <prime>` "
                             "has made; every other field is 64-bit only" % (", ".join(_lib.W32_PRIMES), prime))
        if found is None:
            raise ValueError("prime %r is neither built in nor generated (python -m modarith_amd.generate 64 <prime>)" % (prime,))
        self.params, self.builtin = found[0], found[1] is None      # (generated: params_<TAG>.h / params_<TAG>_w32.h next to its plug-in)
        self.prime, self.name = prime, name
        self.nin = 0
        self.in_idx: List[int] = []         # the values that are element batches, in the order of in[]
        self.sh_idx: List[int] = []         # the values that are shared operands (one element for the whole batch), in the order of in[]
        self.nsel = 0                       # per-element int selectors (modcmv / modcsw): int32 arrays after the element inputs
        self.lazy = set()                   # values produced by a generic=False operation
        self.ops: List[Op] = []
        self.outs: List[int] = []
        self.npred = 0                      # ints computed inside the chain (Pred): s<nsel> .. s<nsel + npred - 1>
        self.pouts: List[int] = []          # the ints that are outputs (indices of the int space), in the order of out[] after the element outputs
        self.nvals = 0
        self.bins: List[BIn] = []           # byte-record inputs, in the order of in[]
        self.bouts: List[BOut] = []         # byte-record outputs, in the order of out[]

    # ------------------------------------------------------------------ building
    def _new(self) -> Val:
        v = Val(self, self.nvals)
        self.nvals += 1
        return v

    def _declaring(self) -> None:                     # every kind of input: the ints' places (selectors first) and the vote rest on it
        if self.ops or any(b.sign >= 0 for b in self.bouts):     # (a byte output with a sign has fixed that int's place)
            raise ValueError("declare every input before the first operation")

    def _room(self) -> None:                          # every operation
        if len(self.ops) >= MAX_OPS:
            raise ValueError("chains are limited to %d operations" % MAX_OPS)

    def layout(self) -> Tuple[Dict[str, int], Dict[str, int]]:
        """THE ARRAYS OF A CALL: (in, out), each the kinds of array in the order they are passed, with how many of the kind.  The one statement
        of that order on the Python side -- FusedChain's argument checks, the metadata record and prototype() derive from it -- and the
        same list as the header comment of csrc/chain.inc, whose entry points take them as `in[]` and `out[]`.
        in:  element batches, byte-record arrays (uint8 [n, Nbytes]), shared operands (HOST: Nlimbs words each), int32 selector arrays;
        out: element batches, byte-record arrays, int32 arrays of n entries"""
        return ({"elements": self.nin, "bytes": len(self.bins), "shared": self.nshared, "selectors": self.nsel},
                {"elements": len(self.outs), "bytes": len(self.bouts), "ints": len(self.pouts)})

    def input(self) -> Val:
        self._declaring()
        self.nin += 1
        v = self._new()
        self.in_idx.append(v.idx)
        return v

    def shared(self) -> Val:
        """an element operand that is the same for every element of the batch: Nlimbs words on the host"""
        self._declaring()
        if len(self.sh_idx) >= MAX_SHARED:
            raise ValueError("a chain takes at most %d shared operands" % MAX_SHARED)
        v = self._new()
        self.sh_idx.append(v.idx)
        return v

    @property
    def nshared(self) -> int:
        return len(self.sh_idx)

    def input_bytes(self, little: bool = False, sign: bool = False):
        """a byte-record input: n records of Nbytes bytes, big-endian, or with little=True least significant byte first (the integer that
        reverse() + modimp would read).  Returns (v, ok): v is what Field.modimp leaves (the integer the bytes spell, modfsb, nres), ok its
        return value as a Pred: 1 where the integer was below p.  With sign=True returns (v, ok, s): s is the record's most significant
        bit -- bit 8 Nbytes - 1 of the integer -- as an int of the chain, and the bit is cleared before modfsb / nres see the integer
        (rfc7748.c:172's mask, RFC 8032's x_0).  Where 8 Nbytes == Nbits that is simply the value's top bit"""
        self._declaring()
        v, ok = self._new(), Pred(self, self.npred)
        self.npred += 1
        s = None
        if sign:
            s = Pred(self, self.npred)
            self.npred += 1
        self.bins.append(BIn(v.idx, ok.idx, bool(little), s.idx if sign else -1))
        return (v, ok, s) if sign else (v, ok)

    def output_bytes(self, v: Val, little: bool = False, sign=None) -> None:
        """a byte-record output, modexp(v): redc, then Nbytes bytes a record, big-endian or with little=True least significant byte first.
        sign=d, a Pred or Sel of this chain, ORs d << 7 into the record's most significant byte (`pub[56] = (char)(sign << 7)`): defined
        for d = 0 / 1"""
        self._own(v)
        if v.idx in self.sh_idx:
            raise ValueError("a shared operand is not a per-element array: output_bytes modcpy() of it")
        if sign is not None and (not isinstance(sign, (Sel, Pred)) or sign.chain is not self):
            raise ValueError("the sign of a byte output is an int of this chain: a predicate, a selector, the sign of a byte input")
        self.bouts.append(BOut(v.idx, self._new().idx, bool(little), self._sel(sign) if sign is not None else -1))

    def inputs(self, k: int) -> List[Val]:
        return [self.input() for _ in range(k)]

    def _own(self, *vs: Val):
        for v in vs:
            if isinstance(v, (Pred, Sel)):
                raise ValueError("an int value (a predicate or a selector) is not an element operand")
            if not isinstance(v, Val) or v.chain is not self:
                raise ValueError("operands must be values of this chain")

    def _op(self, op: str, a: Optional[Val], b: Optional[Val] = None, **fields) -> Val:
        """an operation on element values that defines one; fields: its immediate or its selector"""
        self._own(*[v for v in (a, b) if v is not None])
        self._room()
        d = self._new()
        self.ops.append(Op(op, d.idx, a.idx if a is not None else -1, b.idx if b is not None else -1, **fields))
        return d

    def modmul(self, a, b): return self._op("modmul", a, b)
    def modadd(self, a, b): return self._op("modadd", a, b)
    def modsub(self, a, b): return self._op("modsub", a, b)
    def modsqr(self, a): return self._op("modsqr", a)
    def modneg(self, a): return self._op("modneg", a)
    def nres(self, a): return self._op("nres", a)
    def redc(self, a): return self._op("redc", a)
    def modcpy(self, a): return self._op("modcpy", a)
    def modinv(self, a, h=None): return self._op("modinv", a, h)      # h: the progenitor modpro(a) where the caller has it (field.c passes NULL otherwise)

    def modmli(self, a, k: int):
        if not -(1 << 31) <= int(k) < (1 << 31):
            raise ValueError("modmli takes a C int")
        return self._op("modmli", a, imm=int(k))

    # the field's constants, as Field<P>::modint / modone / modzer make them (Montgomery form included): no operand
    def modint(self, k: int):
        if isinstance(k, bool) or not isinstance(k, int) or not -(1 << 31) <= k < (1 << 31):
            raise ValueError("modint takes a C int")
        return self._op("modint", None, imm=k)

    def mod2r(self, r: int):
        """the constant 2^r as Field<P>::mod2r makes it (Montgomery form included; zero for r >= 8 Nbytes, as there)"""
        if isinstance(r, bool) or not isinstance(r, int) or not 0 <= r < (1 << 31):
            raise ValueError("mod2r takes an unsigned C int")
        return self._op("mod2r", None, imm=r)

    # field.c's shifts by less than a limb, and the functions that return an int beside the element they leave in place
    def _shift(self, k):
        if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= min(self.params.radix - 1, 31):
            raise ValueError("a shift count is a C immediate with 1 <= k < Radix (%d) and k <= 31 (got %r)" % (self.params.radix, k))
        return k

    def modshl(self, a, k: int):
        """a << k on the limbs (field.c's modshl: no reduction -- the top limb grows by k bits, so a 64-bit chain with a modshl runs the
        exact products throughout)"""
        return self._op("modshl", a, imm=self._shift(k))

    def _with_int(self, op: str, a: Val, imm: int = 0):
        self._own(a)
        self._room()
        d, r = self._new(), Pred(self, self.npred)
        self.npred += 1
        self.ops.append(Op(op, d.idx, a.idx, imm=imm, sdst=self.nsel + r.idx))
        return d, r

    def modshr(self, a, k: int):
        """(a >> k, r): r the k bits shifted out, field.c's return value -- an int32 output like any other; as a selector or an operand of
        land / lor / lxor / lnot it is defined for 0 / 1 only, i.e. k = 1 (as the reference's own expressions are)"""
        return self._with_int("modshr", a, self._shift(k))

    def modfsb(self, a):
        """(the canonical limbs of a - p or, where that is negative, of a; 1 where a was below p): field.c's modfsb"""
        return self._with_int("modfsb", a)

    def flatten(self, a):
        """(a with its carries propagated, plus p where it was negative; that carry): field.c's flatten"""
        return self._with_int("flatten", a)

    def modone(self): return self._op("modone", None)
    def modzer(self): return self._op("modzer", None)

    # generic=False forms (pseudo.py:294-302, 315-324, 337-346: what rfc7748.c:20 asks for).  Their results carry up to two extra bits;
    # one level of them keeps the limb contract the split products rely on, a lazy sum of lazy sums need not -- refused here
    def _lazy(self, op, a, b=None):
        if self.wl == 32:
            raise ValueError("%s is not offered at word length 32 (include/modarith_amd_w32.h: the 29-bit limbs of X25519 leave no room for "
                             "an unreduced sum); use %s" % (op, op[:-5]))
        for v in (a, b):
            if v is not None and v.idx in self.lazy:
                raise ValueError("%s of a value that is itself a generic=False result: reduce in between (modadd / modsub / modmul ...)" % op)
        d = self._op(op, a, b)
        self.lazy.add(d.idx)
        return d

    def modadd_lazy(self, a, b): return self._lazy("modadd_lazy", a, b)
    def modsub_lazy(self, a, b): return self._lazy("modsub_lazy", a, b)
    def modneg_lazy(self, a): return self._lazy("modneg_lazy", a)
    def modpro(self, a): return self._op("modpro", a)
    def modsqrt(self, a, h=None): return self._op("modsqrt", a, h)
    def modhaf(self, a): return self._op("modhaf", a)

    def modnsqr(self, a, k: int):
        if not 0 <= int(k) <= 100000:
            raise ValueError("modnsqr count out of range")
        return self._op("modnsqr", a, imm=int(k))

    def selector(self) -> "Sel":
        """a per-element int input (0 / 1), as the `int b` of modcmv / modcsw: an int32 array"""
        self._declaring()
        self.nsel += 1
        return Sel(self, self.nsel - 1)

    def _sel(self, d):
        if not isinstance(d, (Sel, Pred)) or d.chain is not self:
            raise ValueError("the selector must come from this chain's selector() or be an int computed in this chain")
        return d.idx if isinstance(d, Sel) else self.nsel + d.idx

    # ints computed inside the chain.  A Pred's place in the int space is nsel + its own count: selectors are declared before the first operation
    def _pred(self, op: str, **operands) -> Pred:
        self._room()
        d = Pred(self, self.npred)
        self.npred += 1
        self.ops.append(Op(op, self.nsel + d.idx, **operands))
        return d

    def _test(self, op: str, a: Val, b: Optional[Val] = None) -> Pred:
        self._own(*[v for v in (a, b) if v is not None])
        return self._pred(op, a=a.idx, b=b.idx if b is not None else -1)

    def modis0(self, a): return self._test("modis0", a)
    def modis1(self, a): return self._test("modis1", a)
    def modsign(self, a): return self._test("modsign", a)
    def modcmp(self, a, b): return self._test("modcmp", a, b)

    def modqr(self, x, h=None):
        """1 where x is a quadratic residue or zero (field.c's modqr(h, x)); h: the progenitor modpro(x) where the caller has it"""
        return self._test("modqr", x, h)

    # the reference's own expressions on such ints (`1 - d`, `d & e`, ...): defined for operands that are 0 or 1, as they are there
    def _ints(self, *ds):
        for d in ds:
            if not isinstance(d, (Sel, Pred)):
                raise ValueError("int expressions take predicates and selectors, not element values")
        return dict(zip(("sa", "sb"), (self._sel(d) for d in ds)))

    def lnot(self, d): return self._pred("lnot", **self._ints(d))
    def land(self, d, e): return self._pred("land", **self._ints(d, e))
    def lor(self, d, e): return self._pred("lor", **self._ints(d, e))
    def lxor(self, d, e): return self._pred("lxor", **self._ints(d, e))

    def modcmv(self, d, g, f):
        """f' = d ? g : f  (constant time: lane-predicated selects, pseudo.py:1017-1048)"""
        return self._op("modcmv", g, f, sa=self._sel(d))

    def modcsw(self, d, g, f):
        """(g', f') = d ? (f, g) : (g, f)  (pseudo.py:979-1014)"""
        k = self._sel(d)
        self._own(g, f)
        self._room()
        g2, f2 = self._new(), self._new()
        self.ops.append(Op("modcsw", g2.idx, g.idx, f.idx, sa=k, dst2=f2.idx))
        return g2, f2

    def output(self, v) -> None:
        """an element value: a limb array like the inputs; a Pred: an int32 array of one entry per element"""
        if isinstance(v, Sel):
            raise ValueError("a selector is the caller's own array: there is nothing to output")
        if isinstance(v, Pred):
            if v.chain is not self:
                raise ValueError("operands must be values of this chain")
            self.pouts.append(self.nsel + v.idx)
            return
        self._own(v)
        if v.idx in self.sh_idx:
            raise ValueError("a shared operand is not a per-element array: output modcpy() of it")
        self.outs.append(v.idx)

    # ------------------------------------------------------------------ emission
    def _long(self) -> bool:                          # an inversion, a progenitor or a square root in the chain: one element per lane
        return any(o.op in _HEAVY for o in self.ops)

    def default_ept(self) -> int:
        return 1 if self._long() else 2 if self.wl == 64 else W32_EPT_DEFAULT

    @property
    def _tag(self) -> str:
        """what follows the chain's name in its symbol, library and object names"""
        return self.prime if self.wl == 64 else self.prime + "_w32"

    @property
    def symbol(self) -> str:
        return "chain_%s_%s_batch" % (self.name, self._tag)

    def traffic_bytes(self) -> int:
        """HBM bytes per element of the fused kernel; the call-by-call sequence moves sum(w N (operands + 1)) instead (w = 8 or 4 bytes a limb).
        A shared operand costs the fused kernel nothing (it is in the kernel arguments); call by call it is an array like any other operand"""
        return ((self.wl // 8) * self.params.nlimbs * (self.nin + len(self.outs)) + 4 * self.nsel + 4 * len(self.pouts)
                + self.params.nbytes * (len(self.bins) + len(self.bouts)))

    def unfused_traffic_bytes(self) -> int:
        """a predicate call reads its operand arrays and writes 4 bytes; a selector, streamed in or computed, is a 4-byte read of the call that
        uses it; a progenitor passed as h is one more operand array.  The int expressions are not counted (a caller's own elementwise passes).
        A byte input is a modimp call (Nbytes in, an element and the 4-byte flag out), a byte output a modexp call; a little-endian record
        costs one more read and write of Nbytes (the reversal), a sign on either side 4 bytes (its own int array).  modshr / modfsb /
        flatten write their 4-byte int"""
        w = (self.wl // 8) * self.params.nlimbs
        total = len(self.bins) * (self.params.nbytes + w + 4) + len(self.bouts) * (w + self.params.nbytes)
        recs = self.bins + self.bouts
        total += 2 * self.params.nbytes * sum(r.little for r in recs) + 4 * sum(r.sign >= 0 for r in recs)
        for o in self.ops:
            op = o.op
            if op in _INT_OPS:
                continue
            arrays = _OPS[op] + (1 if op in _WITH_H and o.b >= 0 else 0)
            if op in _PREDS:
                total += w * arrays + 4
            else:
                total += w * (arrays + (2 if op == "modcsw" else 1)) + (4 if op in ("modcmv", "modcsw") + _INT_RET else 0)
        return total

    def _body_lines(self) -> List[str]:
        """the chain as Field<P> calls on registers, one line per operation"""
        L = ["    F::nres(v%d, v%d);" % (i, i) for i in (b.v for b in self.bins)]      # io.imp() left the canonical limbs: the rest of modimp, on the voted products
        tested = set()                                        # values a predicate has read
        for o in self.ops:
            op, d, a, b = o.op, o.dst, o.a, o.b
            if op in _PREDS and op != "modqr":
                # Every predicate starts with redc of its operands.  A second one on the same value would share the pure part of that
                # redc with the first (the products; the pinned accumulations are not shareable) and keep every partial product live
                # in between: 392 instead of 72 registers for `modsign(u) ... modcmp(u, v)` over P-256.  It reads an opaque copy instead
                pre, ab = "", [a, b]
                for k, x in enumerate(ab):
                    if x >= 0 and x in tested:
                        pre += "spint t%d_%d[P::N]; opaque(v%d, t%d_%d); " % (d, k, x, d, k)
                        ab[k] = "t%d_%d" % (d, k)
                    elif x >= 0:
                        tested.add(x)
                        ab[k] = "v%d" % x
                L.append("    %ss%d = F::%s(%s);" % (pre, d, op, ", ".join(x for x in ab if x != -1)))
                continue
            L.append("    " + _CALLS.get(op, _CALLS[_OPS[op]]).format(h="nullptr" if b < 0 else "v%d" % b, **o._asdict()))
        return L + ["    F::redc(v%d, v%d);" % (a, d) for a, d in ((b.v, b.t) for b in self.bouts)]            # the first half of modexp; io.exp() makes the bytes

    # The unit, piece by piece; every helper returns lines, source() puts them in order
    def _shape(self, ept, policy, block):
        """what depends on the word length: (the includes and the namespace, the constants of the build's shape, HEAVY)"""
        P, N = self.prime, self.params.nlimbs
        if self.wl == 32:
            if policy != "vote":
                raise ValueError("word length 32 has one product policy: there is nothing to force")
            heavy = self._long()
            cap = 1 if heavy else (ept or self.default_ept())
            if cap not in (1, 2, 4):
                raise ValueError("elements per lane at word length 32: 1, 2 or 4")
            if not self.builtin:
                cap = min(cap, emit.w32_ept_max(N))       # (the width a generated field's limb count leaves in registers)
            block = block or W32_BLOCK_DEFAULT
            if block not in (64, 128, 256):
                raise ValueError("workgroup size: 64, 128 or 256")
            head = ['#include "%s"' % ("w32_%s.h" % P if self.builtin else "params_%s_w32.h" % P), '#include "modarith_amd_w32.h"', '#include "capi_common.h"', '#include "kernels32.h"', "#include <utility>", "",
                    "namespace {", "using namespace ma32;", "using P = ma32::P_%s_W32;" % P]
            return head, ["constexpr int EPT_CAP = %d;   // widest access of this build in elements per lane (4 = 16 bytes, 2 = 8, 1 = 4); wider kernels are not instantiated" % cap,
                          "constexpr int CBLOCK = %d;   // workgroup size" % block], heavy
        if block is not None:
            raise ValueError("the workgroup size is a parameter of the 32-bit word form only")
        heavy = (ept or self.default_ept()) == 1          # (default_ept() is 1 where an operation of _HEAVY is in the chain)
        # one LDS image per input array of the element-major kernel while they fit 64 KB (512 (N | 1) words each), else one shared
        # image; none above 14 limbs, where a single image does not fit (as k_convert_lds)
        images = 0 if N > 14 else self.nin if self.nin * 512 * (N | 1) * 8 <= 65536 else 1
        head = ['#include "params_%s.h"' % P, '#include "modarith_amd.h"', '#include "capi_common.h"', '#include "kernels.h"', "#include <utility>", "",
                "namespace {", "using namespace ma;", "using P = ma::P_%s;" % P]
        return head, ([] if self.bins or self.bouts else ["#define CHAIN_AOS_IMAGES %d   // LDS images of the element-major kernel: one per input array, 1 = one shared image, 0 = no kernel (more than 14 limbs)" % images]), heavy

    def _defines(self, waves: int) -> List[str]:
        """the optional #defines csrc/chain.inc reads: only those of what the chain has"""
        L = []
        if self.sh_idx:
            L.append("#define CHAIN_NSHARED %d   // operands that are one element for the whole batch: host pointers after the element batches in in[], by value in the kernel arguments" % self.nshared)
        if self.pouts:
            L.append("#define CHAIN_NPRED %d   // int32 results, one entry per element: device arrays after the element outputs in out[]" % len(self.pouts))
        if self.bins:
            L.append("#define CHAIN_NBIN %d   // byte-record inputs: arrays of n records of P::NBYTES %s after the element batches in in[]"
                     % (len(self.bins), "bytes (byte order and sign: below)" if any(b.little or b.sign >= 0 for b in self.bins) else "big-endian bytes"))
        if self.bins or self.bouts:
            L.append("#define CHAIN_BYTES_STAGED %d   // the way to the bytes of a call on 16-byte aligned record arrays: 1 = staged through LDS, 0 = direct (fuse.BYTES_IO_DEFAULT)"
                     % (BYTES_IO_DEFAULT[self.wl] == "staged"))
        if self.bouts:
            L.append("#define CHAIN_NBOUT %d   // byte-record outputs: arrays of n records after the element outputs in out[]" % len(self.bouts))
        for what, recs in (("BIN", self.bins), ("BOUT", self.bouts)):      # (per-array bitmasks; a chain of big-endian records without signs names none)
            le, sg = (sum(1 << k for k, r in enumerate(recs) if on(r)) for on in (lambda r: r.little, lambda r: r.sign >= 0))
            if le:
                L.append("#define CHAIN_%s_LE 0x%x   // bit j: the records of byte %s j are little-endian (byte 0 the least significant)" % (what, le, "input" if what == "BIN" else "output"))
            if sg:
                L.append("#define CHAIN_%s_SIGN 0x%x   // bit j: the most significant bit of the records of byte %s j is a sign, %s" % (
                    what, sg, "input" if what == "BIN" else "output", "taken out before modfsb" if what == "BIN" else "OR-ed in after redc"))
        if waves:
            L.append("#define CHAIN_KERNEL_ATTR __attribute__((amdgpu_waves_per_eu(%d, %d)))" % (waves, waves))
        return L

    def _body(self) -> List[str]:
        """body<F>: the chain on one element's registers, behind the helper that some of its lines call"""
        consts = set(self.in_idx) | set(self.sh_idx)      # what the body only reads: the element inputs and the shared operands
        calls = self._body_lines()
        L = [""]
        if any("opaque(" in l for l in calls):
            L += ["// a copy of an element that the compiler cannot see through (for a value that a second predicate reads: Chain._body_lines)",
                  'MA_DEV void opaque(const spint* a, spint* c) { static_for<0, P::N>([&](auto I) { spint x = a[I]; asm volatile("" : "+v"(x)); c[I] = x; }); }', ""]
        L += ["// the chain on one element's registers; F = %s" % ("Field<P> (one product policy at this word length: no vote)" if self.wl == 32 else "Field<P, FAST>"),
              "template <class F> MA_DEV void body(%s) {" % ", ".join([("const spint* v%d" if i in consts else "spint* v%d") % i for i in range(self.nvals)] + ["int s%d" % k for k in range(self.nsel)] + ["int& s%d" % (self.nsel + k) for k in range(self.npred)])]
        return L + calls + ["}"]

    def _vote(self, policy: str) -> List[str]:
        """the lines of chain_step that run body<F> on each of the lane's elements: at word length 64 under the wave's vote on the inputs"""
        shared = set(self.sh_idx)                         # one element for the whole batch: a pointer into the kernel arguments, not a per-lane array
        args = ", ".join([("v%d" if i in shared else "v%d[E]") % i for i in range(self.nvals)] + ["s%d[E]" % k for k in range(self.nsel + self.npred)])
        if self.wl == 32:
            return ["    static_for<0, EPT>([&](auto E) { body<Field<P>>(%s); });" % args]
        # modint of a negative int is the word (spint)k, outside the limb contract at 64 bits: such a chain runs the exact products, as Field.modint does
        # modshl does not reduce: the top limb of its result grows by k bits and leaves the contract in the same way
        if policy == "vote" and any((o.op == "modint" and o.imm < 0) or o.op == "modshl" for o in self.ops):
            policy = "exact"
        return ["    bool fast = %s;" % ("true" if policy == "fast" else "false"),
                "    if constexpr (P::SPLIT > 0 && %s) {" % ("true" if policy == "vote" else "false"),
                "        bool ok = %s;" % (" && ".join("in_split_contract<P>(v%d)" % i for i in self.sh_idx) or "true"),
                "        static_for<0, EPT>([&](auto E) { ok = ok && " + " && ".join("in_split_contract<P>(v%d[E])" % i for i in self.in_idx + [b.v for b in self.bins]) + "; });",
                "        fast = __all(ok);",
                "    }",
                "    if (fast) {",
                "        static_for<0, EPT>([&](auto E) { body<Field<P, true>>(%s); });" % args,
                "    } else {",
                "        static_for<0, EPT>([&](auto E) { body<Field<P, false>>(%s); });" % args,
                "    }"]

    def _step(self, policy: str) -> List[str]:
        """chain_step<EPT, IO>: the lane's elements in through io, the chain, the results out through io"""
        L = ["", "// EPT elements of a lane through the chain; io is how the calling kernel of csrc/chain.inc reaches them in memory",
             "template <int EPT, class IO> MA_DEV void chain_step(IO io) {",
             "    " + " ".join("spint v%d[EPT][P::N];" % i for i in range(self.nvals) if i not in self.sh_idx)]
        L += ["    io.load(%d, v%d);" % (k, i) for k, i in enumerate(self.in_idx)]
        L += ["    const spint* v%d = io.shared(%d);" % (i, k) for k, i in enumerate(self.sh_idx)]
        L += ["    int s%d[EPT]; io.sel(%d, s%d);" % (k, k, k) for k in range(self.nsel)]
        L += ["    int s%d[EPT];" % (self.nsel + k) for k in range(self.npred)]
        L += ["    io.imp(%d, v%d, s%d%s);" % (k, b.v, self.nsel + b.ok, ", s%d" % (self.nsel + b.sign) if b.sign >= 0 else "") for k, b in enumerate(self.bins)]
        L += self._vote(policy)
        L += ["    io.store(%d, v%d);" % (k, o) for k, o in enumerate(self.outs)]
        L += ["    io.exp(%d, v%d%s);" % (k, b.t, ", s%d" % b.sign if b.sign >= 0 else "") for k, b in enumerate(self.bouts)]
        L += ["    io.pred(%d, s%d);" % (k, o) for k, o in enumerate(self.pouts)]
        return L + ["}"]

    def source(self, ept: Optional[int] = None, policy: str = "vote", waves: int = 0, block: Optional[int] = None) -> str:
        """The unit: what depends on the chain -- constants, body<F> and chain_step<EPT, IO> -- around csrc/chain.inc, which holds the
        kernels (k_chain<EPT>, k_chain_aos) and the bodies of the entry points for both word lengths.
        ept: elements per lane on aligned batches (2 = 16-byte accesses, 1 = 8-byte; at word length 32: 4 / 2 / 1 = 16 / 8 / 4 bytes);
        None = the measured default.  block: workgroup size, word length 32 only"""
        if not (self.nin or self.bins) or not (self.outs or self.pouts or self.bouts):
            raise ValueError("a chain needs at least one input and one output")
        w32, nbytes = self.wl == 32, len(self.bins) + len(self.bouts)
        head, shape, heavy = self._shape(ept, policy, block)
        entry = "const void* const* in, void* const* out, size_t n, "
        L = ["// GENERATED by modarith_amd/fuse.py -- do not edit.  Chain %r over %s%s: %d inputs%s, %d operations, %d outputs%s; kernels and entry bodies: csrc/chain.inc"
             % (self.name, self.prime, ", 32-bit word form" if w32 else "", self.nin, ", %d shared" % self.nshared if self.sh_idx else "", len(self.ops), len(self.outs),
                (", %d int outputs" % len(self.pouts) if self.pouts else "") + (", %d byte inputs, %d byte outputs" % (len(self.bins), len(self.bouts)) if nbytes else ""))]
        L += head + ['#define CHAIN_SYMBOL "%s"   // the entry points: <this>_batch%s' % (self.symbol[:-6], "" if w32 else ", <this>_aos"),
                     "constexpr int NIN = %d, NOUT = %d, NSEL = %d;" % (self.nin, len(self.outs), self.nsel),
                     "constexpr bool HEAVY = %s;   // one element per lane on every batch: an inversion, a progenitor or a square root in the chain%s"
                     % ("true" if heavy else "false", "" if w32 else ", or build(ept=1)")]
        L += shape + self._defines(waves) + self._body() + self._step(policy)
        L += ['#include "chain.inc"', "}  // namespace", "",
              'extern "C" int %s(%ssize_t ld, void* stream) { return chain_batch(in, out, n, ld, stream); }' % (self.symbol, entry)]
        if not w32:
            L += ['extern "C" int %s(%svoid* stream) { return chain_aos(in, out, n, stream); }' % (self.aos_symbol, entry)]
        return "\n".join(L + [""])

    @property
    def aos_symbol(self) -> str:
        if self.wl == 32:
            raise ValueError("the element-major entry is not built at word length 32: convert with modarith_amd_w32_aos_to_soa and call %s" % self.symbol)
        return "chain_%s_%s_aos" % (self.name, self.prime)

    def prototype(self) -> str:
        """the C declaration of the _batch entry, with what layout() says `in` and `out` hold"""
        ins, outs = self.layout()
        recs = ", then %%d arrays of n records of %d bytes" % self.params.nbytes
        say = lambda kinds, texts: "".join(t % kinds[kind] for kind, t in texts if kinds[kind])
        rest = say(outs, (("bytes", recs), ("ints", ", then %d int32 arrays of n entries")))
        return ("int %s(const void *const *in /* %d element batches%s */, void *const *out /* %d%s */, size_t n, size_t ld, void *stream);"
                % (self.symbol, ins["elements"], say(ins, (("bytes", recs), ("shared", ", then %%d host pointers to shared operands of %d limbs" % self.params.nlimbs),
                                                           ("selectors", ", then %d int32 selector arrays"))), outs["elements"], " element batches" + rest if rest else ""))

    # ------------------------------------------------------------------ building the plug-in
    def lib_path(self, plugin_dir: Optional[str] = None) -> str:
        return os.path.join(plugin_dir or _gen.PLUGIN_DIR, "libmodarith_amd_chain_%s_%s.so" % (self.name, self._tag))

    def build(self, plugin_dir: Optional[str] = None, force: bool = False, verbose: bool = False, ept: Optional[int] = None, policy: str = "vote", waves: int = 0,
              block: Optional[int] = None) -> "FusedChain":
        """one hipcc unit, installed and reused as every plug-in is (modarith_amd/generate.py, modarith_amd/plugin.py)"""
        d = plugin_dir or _gen.PLUGIN_DIR
        os.makedirs(d, exist_ok=True)
        src_text = self.source(ept, policy, waves, block)
        base = "chain_%s_%s" % (self.name, self._tag)
        src, obj, meta = (os.path.join(d, base + e) for e in (".hip", ".o", ".json"))
        lib = self.lib_path(d)
        emit._write(src, src_text)
        ins, outs = self.layout()
        record = {"chain": self.name, "prime": self.prime, "wl": self.wl, "inputs": ins["elements"], "shared": ins["shared"], "selectors": ins["selectors"],
                  "outputs": outs["elements"], "preds": outs["ints"], "ops": [o.op for o in self.ops], "symbol": self.symbol}
        if ins["bytes"] or outs["bytes"]:
            record.update(bytes_in=ins["bytes"], bytes_out=outs["bytes"])
        # A chain that computes ints is compiled without the SLP vectoriser: at two elements per lane it pairs the limbs of the two elements'
        # redc (they arrive as the halves of one 16-byte load) into vector operations and the kernel of four predicates over P-256 comes to
        # 380 registers instead of 119.  Chains without ints are compiled as they always were
        flags = ["-fno-slp-vectorize"] if self.npred else []
        built = build_plugin(d, lib, meta, record, _gen.key_of(src_text, emit.header_text(self.params)), [(src, obj, flags)], "chain", force, verbose)
        return FusedChain(self, lib, built)


class FusedChain:
    """a built chain: call it with the arrays of Chain.layout(), in its order -- element batches are flat [N, n] or tiled [n / tile, N,
    tile], all the same shape (int64 limbs, or int32 for a chain of the 32-bit word form), byte records uint8 [n, Nbytes], a shared
    operand Nlimbs ints or a CPU integer tensor (as Field.modmuls takes b0), selectors int32 [n] on the device.  Returns the output
    arrays in the layout's order; `out=` takes them in that order"""
    def __init__(self, chain: Chain, lib: str, built: bool):
        self.chain, self.path, self.built = chain, lib, built
        _lib.load()
        self.lib = ctypes.CDLL(lib)
        self.fn = getattr(self.lib, chain.symbol)
        self.fn.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
        self.fn.restype = ctypes.c_int
        self._fields = {}

    @staticmethod
    def _cut(arrays, kinds):
        """the arrays of one side of a call, one list per kind of that side of Chain.layout(); None where the count is not the layout's"""
        if len(arrays) != sum(kinds.values()):
            return None
        it = iter(arrays)
        return [[next(it) for _ in range(count)] for count in kinds.values()]

    def _split(self, inputs, what: str):
        ch = self.chain
        kinds = ch.layout()[0]
        cut = self._cut(inputs, kinds)
        if cut is None:
            raise ValueError("chain %s takes %d element %s%s followed by %d shared operands (%d limbs each, on the host) and %d int32 selector arrays"
                             % (ch.name, kinds["elements"], what, ", %d arrays of byte records (uint8 [n, %d])" % (kinds["bytes"], ch.params.nbytes) if kinds["bytes"] else "",
                                kinds["shared"], ch.params.nlimbs, kinds["selectors"]))
        elems, recs, shared, sels = cut
        return elems, recs, [self._limbs(b) for b in shared], sels

    def _limbs(self, b):
        """one shared operand as host words of the chain's word length: a sequence of Nlimbs ints or a CPU integer tensor, as Field.modmuls takes b0"""
        ch = self.chain
        if hasattr(b, "is_cuda"):
            if b.is_cuda or b.is_floating_point() or b.dim() != 1:
                raise ValueError("a shared operand is %d limbs on the host: a sequence of ints or a CPU integer tensor" % ch.params.nlimbs)
            b = b.tolist()
        b = [int(v) for v in b]
        if len(b) != ch.params.nlimbs:
            raise ValueError("a shared operand is %d limbs on the host (got %d)" % (ch.params.nlimbs, len(b)))
        word = ctypes.c_uint64 if ch.wl == 64 else ctypes.c_uint32
        return (word * len(b))(*[v & ((1 << ch.wl) - 1) for v in b])          # (signed tensors hold the same words)

    def _outs(self, out, n: int, like, fresh):
        """the output arrays of a call, one list per kind of Chain.layout(): the caller's, or new ones -- fresh() per element output, uint8
        [n, Nbytes] per byte output, int32 [n] per int output"""
        import torch
        ch = self.chain
        kinds = ch.layout()[1]
        make = {"elements": fresh, "bytes": lambda: torch.empty((n, ch.params.nbytes), dtype=torch.uint8, device=like.device),
                "ints": lambda: torch.empty(n, dtype=torch.int32, device=like.device)}
        cut = self._cut(list(out) if out is not None else [make[kind]() for kind, count in kinds.items() for _ in range(count)], kinds)
        if cut is None:
            raise ValueError("chain %s has %d outputs%s%s" % (ch.name, kinds["elements"], " followed by %d byte-record outputs" % kinds["bytes"] if kinds["bytes"] else "",
                                                              " followed by %d int32 outputs" % kinds["ints"] if kinds["ints"] else ""))
        return cut

    def _run(self, fn, symbol: str, ins, outs, n: int, *ld, device=None):
        """what both entries share: the checks of the arrays that are not element batches, the pointer arrays and the call on the current
        stream of the batches' device.  ins, outs: one list per kind, as _split and _outs give them.
        The entry point reads the shared operands' limbs before it returns: the host arrays need to live no longer than this call"""
        import torch
        elems, recs, _, sels = ins
        for d in sels:
            if d.dtype != torch.int32 or d.numel() != n or not d.is_cuda or not d.is_contiguous() or (device is not None and d.device != device):
                raise ValueError("selectors are contiguous int32 device tensors with one 0/1 entry per element")
        ch = self.chain
        dev = device if device is not None else (elems[0] if elems else recs[0]).device
        for r in recs + outs[1]:
            if r.dtype != torch.uint8 or r.dim() != 2 or tuple(r.shape) != (n, ch.params.nbytes) or not r.is_cuda or not r.is_contiguous() or r.device != dev:
                raise ValueError("byte records are contiguous uint8 tensors [n, %d] on the batches' device" % ch.params.nbytes)
        for d in outs[2]:
            if d.dtype != torch.int32 or d.dim() != 1 or d.numel() != n or not d.is_cuda or not d.is_contiguous() or d.device != dev:
                raise ValueError("int outputs are contiguous int32 tensors of n entries on the batches' device")
        flat = [t for kind in outs for t in kind]
        ptrs = [ctypes.addressof(t) if kind == "shared" else t.data_ptr() for kind, arrays in zip(ch.layout()[0], ins) for t in arrays]
        with torch.cuda.device(dev):
            _lib.check(fn((ctypes.c_void_p * len(ptrs))(*ptrs), (ctypes.c_void_p * len(flat))(*[t.data_ptr() for t in flat]), n, *ld,
                          torch.cuda.current_stream(dev).cuda_stream), symbol)
        return tuple(flat)

    def aos(self, *inputs, out: Optional[Sequence] = None):
        """the same chain over element-major device arrays int64 [n, Nlimbs] (`spint x[n][Nlimbs]`, how CPU callers of field.c hold
        elements): no aos_to_soa / soa_to_aos passes around it; the other arrays as in __call__"""
        import torch
        ch = self.chain
        N = ch.params.nlimbs
        if ch.bins or ch.bouts:
            raise ValueError("a chain with byte records has no element-major entry; call %s" % ch.symbol)
        if ch.wl == 32:
            raise ValueError("the element-major entry is not built at word length 32: convert with modarith_amd_w32_aos_to_soa and call %s" % ch.symbol)
        ins = self._split(inputs, "arrays")
        elems = ins[0]
        n = elems[0].shape[0]
        outs = self._outs(out, n, elems[0], lambda: torch.empty_like(elems[0]))
        for t in elems + outs[0]:
            if t.dtype != torch.int64 or t.dim() != 2 or tuple(t.shape) != (n, N) or not t.is_cuda or not t.is_contiguous():
                raise ValueError("expected contiguous int64 device tensors of shape [n, %d]" % N)
        fn = getattr(self.lib, ch.aos_symbol)
        fn.argtypes = [ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t, ctypes.c_void_p]
        fn.restype = ctypes.c_int
        return self._run(fn, ch.aos_symbol, ins, outs, n)

    def __call__(self, *inputs, out: Optional[Sequence] = None, device=None):
        from .field import Field
        ch = self.chain
        ins = self._split(inputs, "batches")
        inputs, recs = ins[:2]
        dev = device if device is not None else (inputs[0] if inputs else recs[0]).device
        F = self._fields.get(dev)
        if F is None:                                  # binding a Field derives the prime's constants: once per device, not per call
            F = self._fields[dev] = Field(ch.prime, dev, wl=ch.wl)
        if not inputs and ch.outs:                     # element results of byte records alone: batches as the field makes them
            n = recs[0].shape[0]
            outs = self._outs(out, n, recs[0], lambda: F.empty(n))
        else:
            n = F._chk(*inputs) if inputs else recs[0].shape[0]
            outs = self._outs(out, n, inputs[0] if inputs else recs[0], lambda: F._out(inputs[0], None))
        elems = inputs + outs[0]
        if elems and F._chk(*elems) != n:
            raise ValueError("the element batches hold %d elements, the byte records %d" % (F._chk(*elems), n))
        return self._run(self.fn, ch.symbol, ins, outs, n, F._ld(elems[0]) if elems else n, device=F.device)


def bench_chain(prime: str = "X25519") -> Chain:
    """the chain bench.py times beside the headline and __graft_entry__.build() pre-builds: z = ((a + b)(a - b))^2, four calls"""
    ch = Chain(prime, "bench_prod")
    u, v = ch.inputs(2)
    ch.output(ch.modsqr(ch.modmul(ch.modadd(u, v), ch.modsub(u, v))))
    return ch


def internal_limbs(prime: str, v: int, wl: int = 64) -> List[int]:
    """the value v as the limbs a shared operand takes: the field's internal form (times R for a Montgomery field), canonical"""
    from .params import derive
    fp = derive(prime, wl=wl)
    v %= fp.p
    return fp.to_limbs(v * fp.R % fp.p if fp.montgomery else v, masked_top=True)


def oncurve_chain(curve: str = "NIST256", wl: int = 64, name: str = "oncurve"):
    """"is (x, y) on the curve": modcmp(y^2, x^3 - 3x + b) for a short Weierstrass curve with a = -3 (the test of weierstrass.c's
    setxy), b shared, ONE int32 per element out and no limb array.  Returns (chain, [limbs of b]); f(x, y, b) -> (ok,)"""
    from .curves import wcurve
    c = wcurve(curve)
    if c.a != -3:
        raise ValueError("oncurve_chain is written for a = -3 (got %s)" % curve)
    ch = Chain(c.field, name, wl=wl)
    x, y = ch.inputs(2)
    b = ch.shared()
    lhs = ch.modsqr(y)
    ch.output(ch.modcmp(lhs, ch.modadd(ch.modsub(ch.modmul(ch.modsqr(x), x), ch.modmli(x, 3)), b)))
    return ch, [internal_limbs(c.field, c.b, wl)]


def pubkey_chain(curve: str = "NIST256", wl: int = 64, name: str = "pubkey"):
    """what a batched ECDSA verifier runs before it trusts an uncompressed public key Q = (x, y) as it arrives: two byte-record inputs, the
    affine coordinates (big-endian, Nbytes each), b shared, ONE int32 per key out:  ok = flag(x) & flag(y) & modcmp(y^2, x^3 - 3x + b)
    -- both coordinates below p and the point on the curve (a = -3).  64 bytes in and 4 out per P-256 key; oncurve_chain() needs two
    modimp passes in front of it.  Returns (chain, [limbs of b]); f(xbytes, ybytes, b) -> (ok,)"""
    from .curves import wcurve
    c = wcurve(curve)
    if c.a != -3:
        raise ValueError("pubkey_chain is written for a = -3 (got %s)" % curve)
    ch = Chain(c.field, name, wl=wl)
    (x, fx), (y, fy) = ch.input_bytes(), ch.input_bytes()
    b = ch.shared()
    on = ch.modcmp(ch.modsqr(y), ch.modadd(ch.modsub(ch.modmul(ch.modsqr(x), x), ch.modmli(x, 3)), b))
    ch.output(ch.land(ch.land(fx, fy), on))
    return ch, [internal_limbs(c.field, c.b, wl)]


def decompress_chain(curve: str = "ED25519", wl: int = 64, name: str = "decompress"):
    """point decompression, edwards.c:290-334 (ecnXXXset from y and the sign s of x) for a = -1 and a full-size d: x from
    x^2 = (1 - y^2) / (-1 - d y^2) with ONE progenitor shared by modqr, modsqrt and modinv, the sign fixed by a computed selector, and a y
    with no x turned into the point at infinity (0, 1, 1) by modcmv instead of the reference's early return.
    Returns (chain, [limbs of d]); f(y, d, s) -> (x, y, z, ok), ok = the modqr test: 1 - isinf of the point (for y = 1, whose x is 0, the
    point that was asked for IS the neutral element: ok = 1)"""
    c = _edwards(curve, "decompress_chain")
    ch = Chain(c.field, name, wl=wl)
    y = ch.input()
    d = ch.shared()
    s = ch.selector()
    _decompress(ch, y, d, s)
    return ch, [internal_limbs(c.field, c.d, wl)]


def _edwards(curve: str, what: str):
    from .curves import curve as _curve
    c = _curve(curve)
    if c.a != -1 or c.small_b:
        raise ValueError("%s is written for a = -1 and a full-size d (ED25519; got %s)" % (what, curve))
    return c


def _decompress(ch: Chain, y, d, s, valid=None) -> None:
    """the body and the outputs of decompress_chain() on a chain whose inputs are declared: y, the shared d, the int s; valid: an int
    that must be 1 beside the modqr test for the point to stand (the flag of a byte input)"""
    one = ch.modone()
    Y = ch.modsqr(y)
    U = ch.modsub(one, Y)                                   # 1 - y^2
    V = ch.modsub(ch.modneg(one), ch.modmul(Y, d))          # -1 - d y^2
    O = ch.modsqr(U)
    W = ch.modmul(ch.modmul(U, O), V)                       # U^3 V
    H = ch.modpro(W)
    ok = ch.modqr(W, H)
    if valid is not None:
        ok = ch.land(valid, ok)
    R = ch.modsqrt(W, H)
    X = ch.modmul(ch.modmul(ch.modinv(W, H), R), O)
    X = ch.modcmv(ch.lxor(ch.modsign(X), s), ch.modneg(X), X)        # (modsign(U) - s) & 1 on 0/1 ints
    bad = ch.lnot(ok)
    ch.output(ch.modcmv(bad, ch.modzer(), X))
    ch.output(ch.modcmv(bad, one, y))
    ch.output(ch.modcpy(one))
    ch.output(ok)


def rfc8032_decode_chain(curve: str = "ED25519", wl: int = 64, name: str = "rfc8032_decode"):
    """RFC 8032 5.1.3 as one kernel: ONE little-endian record with the sign of x in its top bit in, the point out -- decompress_chain()'s
    body on the y and the sign that the record holds, with ok = flag(y) & modqr(...): a record whose y has no x, or whose y is not below
    p, gives (0, 1, 1) and ok = 0.  32 bytes in, three element arrays and 4 bytes out.
    Returns (chain, [limbs of d]); f(record, d) -> (x, y, z, ok)"""
    c = _edwards(curve, "rfc8032_decode_chain")
    ch = Chain(c.field, name, wl=wl)
    y, fy, s = ch.input_bytes(little=True, sign=True)
    d = ch.shared()
    _decompress(ch, y, d, s, valid=fy)
    return ch, [internal_limbs(c.field, c.d, wl)]


def rfc8032_encode_chain(curve: str = "ED25519", wl: int = 64, name: str = "rfc8032_encode"):
    """RFC 8032 5.1.2: affine x, y element batches in, ONE record out -- y little-endian with modsign(x) in the top bit (ecnXXXget, reverse
    and `sign << 7` of the reference's callers).  Returns the chain; f(x, y) -> (record,)"""
    c = _edwards(curve, "rfc8032_encode_chain")
    ch = Chain(c.field, name, wl=wl)
    x, y = ch.inputs(2)
    ch.output_bytes(y, little=True, sign=ch.modsign(x))
    return ch


def edwards_to_montgomery_chain(curve: str = "ED25519", wl: int = 64, name: str = "ed_to_mont"):
    """RFC 7748 4.1, the birational map on wire values: a little-endian record of an Edwards y (the sign bit ignored) in, the
    little-endian record of u = (1 + y) / (1 - y) and ok = flag(y) out.  Bytes on both sides; one inversion (modinv of 0 is 0: y = 1 gives
    u = 0).  Returns the chain; f(record) -> (record, ok)"""
    c = _edwards(curve, "edwards_to_montgomery_chain")
    ch = Chain(c.field, name, wl=wl)
    y, fy, _ = ch.input_bytes(little=True, sign=True)
    one = ch.modone()
    ch.output_bytes(ch.modmul(ch.modadd(one, y), ch.modinv(ch.modsub(one, y))), little=True)
    ch.output(fy)
    return ch


# ---------------------------------------------------------------------------------------------------------------------
# command line: a chain written as text, for consumers that do not otherwise touch Python
#   python -m modarith_amd.fuse 32 X25519 accept "..."        (the same chain over the 32-bit word form)
#   python -m modarith_amd.fuse X25519 accept "in x, y; t = modadd(x, y); w = modsub(x, y); s = modsqr(modmul(t, w)); out modinv(s)"
def parse(prime: str, name: str, text: str, wl: int = 64) -> Chain:
    """statements separated by ';':  `in a, b`  (element inputs, in order) | `shared b, d` (operands that are one element for the whole
    batch) | `sel d` (int32 selector inputs) | `v = f(args)` |
    `g2, f2 = modcsw(d, g, f)` | `out expr, ...`.  Expressions nest: modsqr(modmul(a, b)).  Integers are accepted where the
    function takes one (modmli, modnsqr, modint); modone() and modzer() take nothing.  Function names are the chain's methods, i.e. field.c's.
    The predicates (modis0, modis1, modsign, modcmp, modqr) give ints; `not d`, `d & e`, `d | e`, `d ^ e` are lnot / land / lor / lxor on
    ints and selectors (0 / 1; `not` binds loosest: write `d & (not e)`); modsqrt(a, h), modinv(a, h), modqr(x, h) take the progenitor as
    an optional second argument; `out` takes ints as well: int32 results after the element results.
    `bytes a, b` declares byte-record inputs (a is what modimp leaves), `flag(a)` is modimp's return value for that input, an int like the
    predicates', and `outbytes expr, ...` outputs modexp of the expressions as byte records.
    `lebytes a` declares little-endian records, `sbytes a` / `lesbytes a` records whose top bit is taken out as `sign(a)`, an int beside
    `flag(a)`; `outlebytes expr, ...` writes little-endian records, `outsbytes (expr, int_expr), ...` / `outlesbytes (expr, int_expr), ...`
    records with the int in their top bit.  `v, r = modshr(a, 1)`, `v, f = modfsb(a)` and `v, f = flatten(a)` assign both results."""
    import ast
    ch = Chain(prime, name, wl)
    env, flags, signs = {}, {}, {}
    _INT_AST = {ast.BitAnd: "land", ast.BitOr: "lor", ast.BitXor: "lxor"}

    def ev(node):
        if isinstance(node, ast.Name):
            if node.id not in env:
                raise ValueError("unknown value %r" % node.id)
            return env[node.id]
        if isinstance(node, ast.Constant) and isinstance(node.value, int):
            return node.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub) and isinstance(node.operand, ast.Constant):
            return -node.operand.value
        if isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.Not):
            return ch.lnot(ev(node.operand))
        if isinstance(node, ast.BinOp) and type(node.op) in _INT_AST:
            return getattr(ch, _INT_AST[type(node.op)])(ev(node.left), ev(node.right))
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "flag" and not node.keywords:
            if len(node.args) != 1 or not isinstance(node.args[0], ast.Name) or node.args[0].id not in flags:
                raise ValueError("flag() takes the name of a byte input: %r" % ast.unparse(node))
            return flags[node.args[0].id]
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and node.func.id == "sign" and not node.keywords:
            if len(node.args) != 1 or not isinstance(node.args[0], ast.Name) or node.args[0].id not in signs:
                raise ValueError("sign() takes the name of a byte input declared with sbytes or lesbytes: %r" % ast.unparse(node))
            return signs[node.args[0].id]
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Name) and not node.keywords:
            fn = node.func.id
            if fn not in _OPS or not hasattr(ch, fn):
                raise ValueError("unknown operation %r (available: %s)" % (fn, ", ".join(sorted(_OPS))))
            return getattr(ch, fn)(*[ev(a) for a in node.args])
        raise ValueError("cannot parse %r" % ast.unparse(node))

    declare = {"in": ch.input, "shared": ch.shared, "sel": ch.selector}
    records = {"bytes": {}, "lebytes": {"little": True}, "sbytes": {"sign": True}, "lesbytes": {"little": True, "sign": True}}
    emit_as = {"out": ch.output, "outbytes": ch.output_bytes, "outlebytes": lambda v: ch.output_bytes(v, little=True)}
    signed = {"outsbytes": False, "outlesbytes": True}
    for st in [t.strip() for t in text.split(";") if t.strip()]:
        head, _, rest = st.partition(" ")
        if head in declare:
            for nm in [t.strip() for t in rest.split(",")]:
                env[nm] = declare[head]()
        elif head in records:
            for nm in [t.strip() for t in rest.split(",")]:
                got = ch.input_bytes(**records[head])           # (the value, modimp's return value and, where asked for, the sign)
                env[nm], flags[nm] = got[:2]
                signs.update({nm: got[2]} if len(got) == 3 else {})
        elif head in emit_as:
            for node in ast.parse("(%s,)" % rest, mode="eval").body.elts:
                emit_as[head](ev(node))
        elif head in signed:
            for node in ast.parse("(%s,)" % rest, mode="eval").body.elts:
                if not isinstance(node, ast.Tuple) or len(node.elts) != 2:
                    raise ValueError("%s takes pairs (expression, int expression): %r" % (head, ast.unparse(node)))
                ch.output_bytes(ev(node.elts[0]), little=signed[head], sign=ev(node.elts[1]))
        else:
            node = ast.parse(st).body[0]
            if not isinstance(node, ast.Assign) or len(node.targets) != 1:
                raise ValueError("expected `name = expression`: %r" % st)
            val = ev(node.value)
            tgt = node.targets[0]
            if isinstance(tgt, ast.Tuple):
                if not isinstance(val, tuple) or len(val) != len(tgt.elts):
                    raise ValueError("%r does not produce %d values" % (st, len(tgt.elts)))
                for t, v in zip(tgt.elts, val):
                    env[t.id] = v
            else:
                env[tgt.id] = val
    return ch


def main(argv: List[str]) -> int:
    args = [a for a in argv if not a.startswith("--")]
    wl = 64
    if len(args) == 4 and args[0] in ("32", "64"):      # the word length first, as the reference's generators take it
        wl, args = int(args[0]), args[1:]
    if len(args) != 3:
        print('usage: python -m modarith_amd.fuse [32] <prime or tag> <name> "in a, b; t = modadd(a, b); out modsqr(t)" [--force] [--source]')
        return 2
    try:
        ch = parse(*args, wl=wl)
        if "--source" in argv:
            print(ch.source())
            return 0
        f = ch.build(force="--force" in argv, verbose=True)
    except ValueError as e:
        print(e)
        return 2
    print("%s %s" % ("built" if f.built else "up to date:", f.path))
    print(ch.prototype())
    if ch.wl == 64 and not (ch.bins or ch.bouts):
        print("int %s(const void *const *in, void *const *out, size_t n, void *stream);   /* the same over element-major arrays x[n][Nlimbs] */" % ch.aos_symbol)
    print("HBM bytes per element: %d fused, %d call by call" % (ch.traffic_bytes(), ch.unfused_traffic_bytes()))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main(sys.argv[1:]))
