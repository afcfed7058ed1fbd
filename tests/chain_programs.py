"""Seeded random programs for the chain compiler (modarith_amd/fuse.py) and three interpreters of a chain.  TEST INFRASTRUCTURE ONLY.

    ch = random_chain("X25519", 64, 7, "light")      # a Chain built through the builder API; ch.text is the same program for fuse.parse
    python -m tests.chain_programs X25519 64 7 light  # prints that text and the emitted body<F>

The generator draws from random.Random(seed) alone, through Random.random() (so that a program's shape does not depend on the field),
knows the builder's rules and never retries on a ValueError.  Three truths for what a chain computes, all walking Chain.ops / bins /
bouts / outs / pouts with the semantics fuse._CALLS writes down:

    run_oracle   element by element through the scalar functions of the CPU oracle (tests/oracle_binding.py) on 64-bit limb rows:
                 independent of every kernel in the tree.  X25519, NIST256, X448 at 64 bits
    run_calls    the same walk through the methods of Field(P, wl) on device batches: "fusing changed nothing"
    run_model    Python integers: the internal-form value mod p and, where the limbs are known digit for digit, the exact integer;
                 what cannot be said from those is "undetermined" (None)

The progenitor (modpro) and what is made of it without a reduction to canonical form (modsqrt, products of either) have the limbs of the
library's own addition chain, not the reference's: values agree, words need not (docs/oracle_and_parity.md).  `limb_free()` says
which values of a chain those are; the oracle's words for them are compared after redc.
"""
import random
import sys
from typing import List, NamedTuple, Optional

from modarith_amd import fuse
from modarith_amd.fuse import Chain, MAX_SHARED

PROFILES = ("light", "heavy", "bytes", "long", "unreduced")
ORACLE_PRIMES = ("X25519", "NIST256", "X448")
GENERATED = "2519"
CASES = [(P, wl) for P in ORACLE_PRIMES for wl in (64, 32)] + [(GENERATED, 64)]
LONG_OPS = 64
# The seed set: per (prime, word length) case every (profile, seed) below ('unreduced' at 64 bits on the oracle's primes only).  Chosen
# greedily among the first few hundred seeds so that the coverage conditions below (required() / covered()) hold for every case
SEEDS = {"light": (1, 3, 4, 16), "heavy": (10, 129), "bytes": (1, 22, 64), "long": (37,), "unreduced": (2,)}

ELEM_KINDS = ("in", "sh", "const", "byte", "res", "lazy")
INT_KINDS = ("sel", "modis0", "modis1", "modsign", "modcmp", "modqr", "modshr", "modfsb", "flatten", "flag", "sign", "lnot", "land", "lor", "lxor")
_BIN = ("modmul", "modadd", "modsub")
_LAZY_BIN = ("modadd_lazy", "modsub_lazy")
_UN = ("modsqr", "modneg", "nres", "redc", "modcpy", "modmli", "modnsqr", "modhaf")
_CONSTS = ("modint", "modone", "modzer", "mod2r")
_TESTS = ("modis0", "modis1", "modsign", "modcmp")


def programs(P: str, wl: int):
    """the (profile, seed) pairs of one case"""
    return [(pr, s) for pr in PROFILES for s in SEEDS[pr] if pr != "unreduced" or (wl == 64 and P in ORACLE_PRIMES)]


def units(P: str, wl: int):
    """every plug-in of one case: (profile, seed, ept); ept None: the chain's default, 2 and 4: the wider builds of the 32-bit word form
    for the programs without a long exponentiation"""
    u = [(pr, s, None) for pr, s in programs(P, wl)]
    if wl == 32:
        u += [(pr, s, ept) for pr, s in programs(P, wl) if pr in ("light", "bytes") for ept in (2, 4)]
    return u


def plugin_dir(ept=None):
    """where the programs' plug-ins go: a directory of their own under the library's, so that the library's register-budget guard
    (tests/test_kernel_resources.py reads the objects of the plug-in directory itself) keeps speaking of the library's kernels; a
    plug-in's name does not carry its launch shape: the explicit ones in the w32_ept<k> directories, as tests/test_gpu_fuse_pred.py"""
    import os
    from modarith_amd import generate as gen
    return os.path.join(gen.PLUGIN_DIR, "chain_programs" if ept is None else "w32_ept%d" % ept)


_BUILT = {}                                                      # (prime, wl) -> {(profile, seed, ept): FusedChain}


def _cost(case, unit):
    """about how long a unit takes to compile, as a sort key, longest first (seconds on one core over X448, measured one unit at a time:
    the 64-operation body 35, records 13-28 and 17-25 at four elements per lane, the long exponentiations 11-17, light programs 5-14
    and 4-7 at 32 bits; P-256 somewhat less, X25519 less than half)"""
    (P, wl), (pr, s, ept) = case, unit
    if wl == 64:
        t = {"long": 35, "bytes": 20, "heavy": 14, "light": 9, "unreduced": 5}[pr]
    else:
        t = {None: 6, 2: 5, 4: 7}[ept] * (3 if pr == "bytes" and ept else 1)
    return -t * {"X448": 1.0, "NIST256": 0.8, "X25519": 0.4}.get(P, 0.3)


def build_all(cases, workers: int = 16):
    """the plug-ins of several cases through ONE pool, the longest units first: independent hipcc units, and a case on its own leaves
    most of the pool waiting for its slowest one.  Results are kept: build_case() of a case built here compiles nothing"""
    import concurrent.futures as cf
    todo = sorted(((c, u) for c in cases if c not in _BUILT for u in units(*c)), key=lambda cu: _cost(*cu))
    with cf.ThreadPoolExecutor(max_workers=workers) as ex:
        jobs = [(c, u, ex.submit(lambda c=c, u=u: random_chain(c[0], c[1], u[1], u[0]).build(plugin_dir=plugin_dir(u[2]), **({"ept": u[2]} if u[2] else {})))) for c, u in todo]
        for c, u, j in jobs:
            _BUILT.setdefault(c, {})[u] = j.result()
    return {c: _BUILT[c] for c in cases}


def build_case(P: str, wl: int, workers: int = 16):
    """{(profile, seed, ept): FusedChain} of one case"""
    return build_all([(P, wl)], workers)[(P, wl)]


def available_cases():
    """CASES without the generated field where its plug-in is not in this tree"""
    from modarith_amd import generate as gen
    return [c for c in CASES if c[0] != GENERATED or gen.find_field(c[0], wl=64, built=True) is not None]


# ---------------------------------------------------------------------------------------------------------------- generator
class _V:
    """an element value of the program being generated"""
    def __init__(self, val, name, kind, free=False, wide=False, exact=False):
        self.val, self.name, self.kind, self.free, self.wide, self.exact, self.uses = val, name, kind, free, wide, exact, 0
        self.sink = False                                        # only ever output


class _I:
    """an int of the program being generated; bit: 0 or 1 by construction"""
    def __init__(self, obj, name, kind, bit=True):
        self.obj, self.name, self.kind, self.bit, self.uses = obj, name, kind, bit, 0


class _Gen:
    def __init__(self, prime, wl, seed, profile):
        if profile not in PROFILES:
            raise ValueError("profile: one of %s" % ", ".join(PROFILES))
        self.rng = random.Random(int(seed))
        self.profile, self.wl = profile, wl
        self.ch = Chain(prime, "rp_%s_%d" % (profile, seed), wl)
        self.mont = self.ch.params.montgomery
        self.vals: List[_V] = []
        self.ints: List[_I] = []
        self.stmts: List[str] = []
        self.seen, self.intuse, self.used_ops = set(), set(), set()
        self.notes = {"progenitor_of": {}, "features": set()}
        self.want = None

    # every draw goes through Random.random(): the number of draws does not depend on the range
    def r(self):
        return self.rng.random()

    def below(self, k):
        return min(int(self.r() * k), k - 1)

    def pick(self, seq):
        return seq[self.below(len(seq))]

    def shuffled(self, seq):
        seq = list(seq)
        for i in range(len(seq) - 1, 0, -1):
            j = self.below(i + 1)
            seq[i], seq[j] = seq[j], seq[i]
        return seq

    # ---- declarations: every input before the first operation
    def declare(self):
        ch, pr = self.ch, self.profile
        nin, nb = (self.below(3), 1 + self.below(2)) if pr == "bytes" else (1 + self.below(3), 0)
        nsh, nsel = self.below(3), self.below(3)
        if pr == "heavy":
            nsh = 2 + self.below(2)
        if pr == "long":
            nin, nsh, nsel = 3, 2, 2
        assert nsh <= MAX_SHARED
        for what in self.shuffled(["in"] * nin + ["sh"] * nsh + ["sel"] * nsel + ["byte"] * nb):
            if what == "in":
                v = ch.input()
                self.vals.append(_V(v, "x%d" % v.idx, "in", exact=True))
                self.stmts.append("in x%d" % v.idx)
            elif what == "sh":
                v = ch.shared()
                self.vals.append(_V(v, "c%d" % v.idx, "sh", exact=True))
                self.stmts.append("shared c%d" % v.idx)
            elif what == "sel":
                s = ch.selector()
                self.ints.append(_I(s, "s%d" % s.idx, "sel"))
                self.stmts.append("sel s%d" % s.idx)
            else:
                little, sign = self.r() < 0.5, self.r() < 0.5
                got = ch.input_bytes(little=little, sign=sign)
                name = "b%d" % got[0].idx
                self.vals.append(_V(got[0], name, "byte", exact=not self.mont))
                self.ints.append(_I(got[1], "flag(%s)" % name, "flag"))
                if sign:
                    self.ints.append(_I(got[2], "sign(%s)" % name, "sign"))
                self.stmts.append("%s%sbytes %s" % ("le" if little else "", "s" if sign else "", name))
        if pr == "heavy":                                        # the first two shared operands: an element and its progenitor
            sh = [v for v in self.vals if v.kind == "sh"]
            self.notes["progenitor_of"][sh[1].val.idx] = sh[0].val.idx
            self.shx, self.shh = sh[0], sh[1]
            sh[1].kind = "pro"                                   # (an operand of the h slot only)

    # ---- operands
    def elem(self, pos, lazy=False, wide=False, free=True, exact=False, plain=False, other=None):
        """an element operand for position pos ('l', 'r' of a binary operation, 'u' under a unary one); other: not this one, if there is a choice"""
        c = [v for v in self.vals if v.kind != "pro" and not v.sink and (lazy or v.kind != "lazy") and (wide or not v.wide) and (free or not v.free)]
        c = [v for v in c if v is not other] or c
        if exact and self.r() < 0.85:
            c = [v for v in c if v.exact] or c
        if plain and self.r() < 0.6:                             # predicates: what comes from outside takes both answers
            c = [v for v in c if v.kind in ("in", "byte")] or c
        fresh = [v for v in c if (v.kind, pos) not in self.seen]
        idle = [v for v in c if not v.uses and v.kind in ("res", "lazy")]
        t = self.r()
        v = self.pick(fresh) if fresh and t < 0.35 else self.pick(idle) if idle and t < 0.8 else self.pick(c[-4:]) if t < 0.9 else self.pick(c)
        self.seen.add((v.kind, pos))
        v.uses += 1
        return v

    def bit(self, use):
        """an int that is 0 or 1, for use as 'cmv' / 'csw' selector, operand of an int expression ('expr') or 'sign' of a record"""
        c = [i for i in self.ints if i.bit]
        fresh = [i for i in c if (i.kind, use) not in self.intuse]
        i = self.pick(fresh) if fresh and self.r() < 0.8 else self.pick(c)
        if self.want is not None:                                # (step() has an int in mind)
            i, self.want = self.want, None
        self.intuse.add((i.kind, use))
        i.uses += 1
        return i

    # ---- results
    def res(self, val, kind="res", **kw):
        v = _V(val, "v%d" % val.idx, kind, **kw)
        self.vals.append(v)
        return v

    def newint(self, obj, kind, bit=True):
        i = _I(obj, "d%d" % obj.idx, kind, bit)
        self.ints.append(i)
        return i

    def menu(self):
        m = list(_BIN) + list(_UN) + list(_CONSTS) + list(_TESTS) + ["modshr", "modfsb", "flatten"]
        if self.wl == 64:
            m += list(_LAZY_BIN) + ["modneg_lazy"]
        if any(i.bit for i in self.ints):
            m += ["modcmv", "modcsw", "lnot", "land", "lor", "lxor"]
        # modshl: the 'unreduced' profile, whose truth is the oracle; elsewhere (one product policy at 32 bits; a field the oracle does not
        # have) only where no other profile would hold it, and there its result is output and nothing else
        if self.profile == "unreduced" or self.wl == 32 or self.ch.prime not in ORACLE_PRIMES:
            m.append("modshl")
        return m

    def step(self, op=None):
        ch = self.ch
        pend = [(i, u) for i in self.ints if i.bit for u in ("cmv", "csw") if (i.kind, u) not in self.intuse]
        if op is None and pend and self.r() < 0.3:               # an int source that has not selected yet: every source is to steer both
            self.want, u = self.pick(pend)
            op = "mod" + u
        if op is None:
            m = self.menu()
            unused = [o for o in m if o not in self.used_ops]
            op = self.pick(unused) if unused and self.r() < 0.75 else self.pick(m)
        self.used_ops.add(op)
        say = self.stmts.append
        widen = self.profile == "unreduced"
        if op in _BIN:
            # a generic=False result goes into a product and nowhere else, as in rfc7748.c: modneg of one is reduced by the builder's
            # rule, and modadd_lazy of that has come out as a negative element (top limb below zero) on the oracle
            # ... and so does what modshl or a negative modint leave: modadd takes 2p off once, which does not reduce 4a
            a = self.elem("l", lazy=op == "modmul", wide=widen and op == "modmul")
            b = a if self.r() < 0.08 else self.elem("r", lazy=op == "modmul", wide=widen and op == "modmul")
            d = self.res(getattr(ch, op)(a.val, b.val), free=a.free or b.free)
            say("%s = %s(%s, %s)" % (d.name, op, a.name, b.name))
        elif op in _LAZY_BIN:
            a, b = self.elem("l", free=False), self.elem("r", free=False)       # (not of a value of limb_free(): it is compared after redc)
            d = self.res(getattr(ch, op)(a.val, b.val), "lazy")
            say("%s = %s(%s, %s)" % (d.name, op, a.name, b.name))
        elif op == "modneg_lazy":
            a = self.elem("u", free=False)
            d = self.res(ch.modneg_lazy(a.val), "lazy")
            say("%s = modneg_lazy(%s)" % (d.name, a.name))
        elif op in ("modsqr", "modneg", "modcpy"):
            a = self.elem("u", lazy=op != "modneg", wide=widen and op == "modsqr")
            d = self.res(getattr(ch, op)(a.val), "lazy" if op == "modcpy" and a.kind == "lazy" else "res", free=a.free, exact=op == "modcpy" and a.exact)
            say("%s = %s(%s)" % (d.name, op, a.name))
        elif op in ("nres", "redc", "modhaf"):
            a = self.elem("u")
            d = self.res(getattr(ch, op)(a.val), free=a.free and op != "redc", exact=op == "redc" or (op == "nres" and a.exact and not self.mont))
            say("%s = %s(%s)" % (d.name, op, a.name))
        elif op in ("modmli", "modnsqr"):
            a = self.elem("u")
            k = self.pick((0, 1, 2, 3, 19, 121665, (1 << 20) + 7)) if op == "modmli" else self.below(5)
            d = self.res(getattr(ch, op)(a.val, k), free=a.free)
            say("%s = %s(%s, %d)" % (d.name, op, a.name, k))
        elif op in ("modone", "modzer"):
            d = self.res(getattr(ch, op)(), "const", exact=op == "modzer" or not self.mont)
            say("%s = %s()" % (d.name, op))
        elif op == "modint":
            k = self.pick((0, 1, 2, 5, 486662, (1 << 31) - 1))
            neg = self.profile == "unreduced" and self.r() < 0.6
            if neg:
                k = -self.pick((1, 3, 121666))
                self.notes["features"].add("negative modint")
            d = self.res(ch.modint(k), "const", wide=neg, exact=not self.mont and not neg)
            say("%s = modint(%d)" % (d.name, k))
        elif op == "mod2r":
            fp = ch.params
            # (field.c's mod2r writes limb r / Radix for every r below 8 Nbytes: between Nbits and that there is no such limb.  Not asked for)
            k = self.pick((0, 1, fp.radix - 1, fp.radix, fp.radix + 1, fp.n - 1, 8 * fp.nbytes, 8 * fp.nbytes + 3))
            d = self.res(ch.mod2r(k), "const", exact=not self.mont)
            say("%s = mod2r(%d)" % (d.name, k))
        elif op == "modshl":
            a = self.elem("u", free=False, exact=True)
            big = self.r() < 0.3                                 # the whole range of _shift, for a result that is only output
            k = min(ch.params.radix - 1, 31) if big else 1 + self.below(2)
            d = self.res(ch.modshl(a.val, k), wide=True, exact=a.exact)
            d.sink = big or not widen
            assert d.sink or self.profile == "unreduced"
            say("%s = modshl(%s, %d)" % (d.name, a.name, k))
            self.notes["features"].add("modshl")
        elif op in ("modshr", "modfsb", "flatten"):
            a = self.elem("u", free=False, exact=True)
            if op == "modshr":
                k = 1 if self.r() < 0.7 else 2 + self.below(min(ch.params.radix - 1, 31) - 1)
                val, r = ch.modshr(a.val, k)
                say("v%d, d%d = modshr(%s, %d)" % (val.idx, r.idx, a.name, k))
            else:
                k = 1
                val, r = getattr(ch, op)(a.val)
                say("v%d, d%d = %s(%s)" % (val.idx, r.idx, op, a.name))
            self.res(val, exact=a.exact)
            self.newint(r, op, bit=k == 1)
        elif op in _TESTS:
            a = self.elem("l" if op == "modcmp" else "u", plain=True)
            if op == "modcmp":
                b = a if self.r() < 0.15 else self.elem("r", plain=True)
                i = self.newint(ch.modcmp(a.val, b.val), op)
                say("%s = modcmp(%s, %s)" % (i.name, a.name, b.name))
            else:
                i = self.newint(getattr(ch, op)(a.val), op)
                say("%s = %s(%s)" % (i.name, op, a.name))
        elif op == "lnot":
            d = self.bit("expr")
            i = self.newint(ch.lnot(d.obj), op)
            say("%s = not %s" % (i.name, d.name))
        elif op in ("land", "lor", "lxor"):
            d, e = self.bit("expr"), self.bit("expr")
            i = self.newint(getattr(ch, op)(d.obj, e.obj), op)
            say("%s = %s %s %s" % (i.name, d.name, {"land": "&", "lor": "|", "lxor": "^"}[op], e.name))
        elif op == "modcmv":
            # (a generic=False result and a value of limb_free() are not mixed under a selector: the latter is compared after redc,
            # which leaves an unreduced sum unreduced)
            d, g = self.bit("cmv"), self.elem("l", lazy=True)
            f = self.elem("r", lazy=not g.free, free=g.kind != "lazy", other=g)
            z = self.res(ch.modcmv(d.obj, g.val, f.val), "lazy" if "lazy" in (g.kind, f.kind) else "res", free=g.free or f.free, exact=g.exact and f.exact)
            say("%s = modcmv(%s, %s, %s)" % (z.name, d.name, g.name, f.name))
        elif op == "modcsw":
            d, g = self.bit("csw"), self.elem("l", lazy=True)
            f = g if self.r() < 0.1 else self.elem("r", lazy=not g.free, free=g.kind != "lazy", other=g)
            g2, f2 = ch.modcsw(d.obj, g.val, f.val)
            for z in (g2, f2):
                self.res(z, "lazy" if "lazy" in (g.kind, f.kind) else "res", free=g.free or f.free, exact=g.exact and f.exact)
            say("v%d, v%d = modcsw(%s, %s, %s)" % (g2.idx, f2.idx, d.name, g.name, f.name))
        else:
            raise AssertionError(op)

    # ---- the long exponentiations: a progenitor passed on, a shared progenitor, none
    def heavy(self, plan):
        ch, say = self.ch, self.stmts.append
        for what in plan:
            self.used_ops.add(what[0])
            if what == ("modpro",):
                a = self.elem("u", free=False)
                self.pro_a = a
                self.pro_h = self.res(ch.modpro(a.val), "pro", free=True)
                say("%s = modpro(%s)" % (self.pro_h.name, a.name))
                continue
            op, how = what
            a, h = {"h": lambda: (self.pro_a, self.pro_h), "sh": lambda: (self.shx, self.shh), "0": lambda: (self.elem("u", free=False), None)}[how]()
            a.uses += 1
            if h is not None:
                h.uses += 1
                self.notes["features"].add("h: progenitor" if how == "h" else "h: shared")
            args = a.name + (", " + h.name if h is not None else "")
            if op == "modqr":
                i = self.newint(ch.modqr(a.val, h.val if h else None), op)
                say("%s = modqr(%s)" % (i.name, args))
                for sel in ("modcmv", "modcsw"):                 # the rarest int source: it selects both ways at once
                    self.want = i
                    self.step(sel)
            else:
                d = self.res(getattr(ch, op)(a.val, h.val if h else None), free=op == "modsqrt", exact=op == "modinv" and not self.mont)
                say("%s = %s(%s)" % (d.name, op, args))

    def body(self):
        pr = self.profile
        nops = LONG_OPS if pr == "long" else 8 + self.below(17)
        forced = {}
        if pr == "heavy":
            use = lambda how: (self.pick(("modinv", "modsqrt", "modqr")), how)
            plan = self.pick(([use("sh")], [("modpro",), use("h")], [("modpro",), use("h"), use("sh")], [use("sh"), use("0")], [("modpro",), use("h"), use("h")]))
            at = 2 + self.below(max(nops - 6, 1))
            forced[at] = plan
            nops -= len(plan)
        if pr == "unreduced":
            forced[1 + self.below(3)] = "modshl" if self.r() < 0.5 else "modint"
            forced[5] = "modshl"
        k = 0
        while len(self.ch.ops) < nops:
            f = forced.pop(k, None)
            k += 1
            if isinstance(f, list):
                self.heavy(f)
            else:
                self.step(f)
        for f in forced.values():                                # (a plan whose turn did not come)
            self.heavy(f) if isinstance(f, list) else self.step(f)

    # ---- outputs, after the last operation
    def finish(self):
        ch, pr, say = self.ch, self.profile, self.stmts.append
        feats = self.notes["features"]
        leaves = [v for v in self.vals if not v.uses and v.kind in ("res", "lazy", "const")]
        elems, recs = [], []
        only_ints = pr == "light" and self.r() < 0.2 and any(i.kind != "sel" for i in self.ints)
        if not only_ints:
            keep = leaves[-5:]
            if len(keep) > 2 and self.r() < 0.3:
                keep = keep[1:]
            elems = list(keep)
            # what a selector or a subtraction leaves is shown as it is: whatever is computed from it may be the same for both
            # answers (x + y after a swap), and a wrong selector would go unseen
            vd = defined_by(ch)[0]
            shown = [v for v in self.vals if v.val.idx in vd and vd[v.val.idx].op in ("modcmv", "modcsw", "modsub") and v not in elems]
            # (up to a number of arrays: every output stays in registers until the chain has run, and docs/fused_chains.md's "nothing in
            # scratch at one element per lane" does not hold for 14 arrays of P-256 results: 84 bytes, measured on one such program)
            elems += shown[-((16 if pr == "long" else 8) - len(elems)):]
            if not elems:
                elems = [self.vals[-1]] if self.vals[-1].kind not in ("sh", "pro") else []
            t = self.r()
            ins = [v for v in self.vals if v.kind == "in"]
            if t < 0.25 and ins:
                elems.append(self.pick(ins))
                feats.add("input output unchanged")
            elif t < 0.5 and elems:
                elems.append(self.pick(elems))
                feats.add("value output twice")
            if pr == "bytes":
                n = 1 + self.below(max(len(elems), 1))
                recs = [v for v in elems[:n] if v.kind != "lazy"]            # (modexp starts with redc, which is for reduced operands)
                elems = [v for v in elems if not any(v is w for w in recs)]
                bys = [v for v in self.vals if v.kind == "byte"]
                if self.r() < 0.5:
                    recs.append(self.pick(bys))
                    feats.add("byte input to byte output")
                if not recs:
                    recs = [self.pick(bys)]
        if only_ints:
            feats.add("only int outputs")
        if [v for v in leaves if v not in elems and v not in recs]:
            feats.add("dead value")
        for v in elems:
            v.uses += 1
        if elems:
            for v in elems:
                ch.output(v.val)
            say("out " + ", ".join(v.name for v in elems))
        for v in recs:
            little = self.r() < 0.5
            sign = self.bit("sign") if self.r() < 0.5 else None
            ch.output_bytes(v.val, little=little, sign=sign.obj if sign else None)
            say("out%s%sbytes %s" % ("le" if little else "", "s" if sign else "", "(%s, %s)" % (v.name, sign.name) if sign else v.name))
        picked = []                                              # ints: those that have not been an output, are not 0 / 1, or are not used
        for i in self.ints:
            if i.kind != "sel" and (not i.bit or not i.uses or (i.kind, "out") not in self.intuse):
                self.intuse.add((i.kind, "out"))
                picked.append(i)
        if not (picked or elems or recs):
            picked = [i for i in self.ints if i.kind != "sel"][-1:]
            if not picked:
                elems = [[v for v in self.vals if v.kind not in ("sh", "pro")][-1]]
                ch.output(elems[0].val)
                say("out " + elems[0].name)
        picked = picked[-8:]
        for i in picked:
            ch.output(i.obj)
        if picked:
            say("out " + ", ".join(i.name for i in picked))
        self.notes["intuse"] = sorted(self.intuse)
        self.notes["seen"] = sorted(self.seen)


def random_chain(prime: str, wl: int, seed: int, profile: str) -> Chain:
    """the program (prime, wl, seed, profile) names, built through the builder API.  The returned Chain carries `text`, the same program
    in the language of fuse.parse (None where that language cannot say it), and `notes`: which shared operand has to be the
    progenitor of which (`progenitor_of`), and what the generator did on purpose (`features`)"""
    g = _Gen(prime, wl, seed, profile)
    g.declare()
    g.body()
    g.finish()
    g.ch.text = "; ".join(g.stmts)
    g.ch.notes = g.notes
    g.ch.profile = profile
    return g.ch


# ---------------------------------------------------------------------------------------------------------------- what a chain is made of
def defined_by(ch: Chain):
    """{value index: Op} and {int index: Op} of the results of operations"""
    vd, sd = {}, {}
    for o in ch.ops:
        if o.op in fuse._PREDS or o.op in fuse._INT_OPS:
            sd[o.dst] = o
        else:
            vd[o.dst] = o
            if o.dst2 >= 0:
                vd[o.dst2] = o
            if o.sdst >= 0:
                sd[o.sdst] = o
    return vd, sd


def limb_free(ch: Chain):
    """the values whose limbs are those of the library's own addition chains (module docstring): modpro, modsqrt, and what is computed
    from them short of a reduction to canonical limbs (redc; modinv, which returns the normalised form)"""
    free = set()
    for o in ch.ops:
        if o.op in fuse._PREDS or o.op in fuse._INT_OPS:
            continue
        if o.op in ("modpro", "modsqrt") or (o.op not in ("redc", "modinv") and (o.a in free or (o.b in free and o.op not in fuse._WITH_H))):
            free.add(o.dst)
            if o.dst2 >= 0:
                free.add(o.dst2)
    return free


def live_ops(ch: Chain):
    """indices of the operations a result of which reaches an output"""
    vlive = set(ch.outs) | {b.v for b in ch.bouts}
    slive = set(ch.pouts) | {b.sign for b in ch.bouts if b.sign >= 0}
    live = []
    for k in range(len(ch.ops) - 1, -1, -1):
        o = ch.ops[k]
        isint = o.op in fuse._PREDS or o.op in fuse._INT_OPS
        if (o.dst in slive if isint else (o.dst in vlive or o.dst2 in vlive or o.sdst in slive)):
            live.append(k)
            vlive |= {x for x in (o.a, o.b) if x >= 0}
            slive |= {x for x in (o.sa, o.sb) if x >= 0}
    return sorted(live)


def _walk(ch: Chain, dom, elems, shared, sels, recs):
    """the chain on one domain: (element outputs, byte outputs, int outputs)"""
    v, s = {}, {}
    for k, i in enumerate(ch.in_idx):
        v[i] = elems[k]
    for k, i in enumerate(ch.sh_idx):
        v[i] = shared[k]
    for k in range(ch.nsel):
        s[k] = sels[k]
    for k, b in enumerate(ch.bins):
        v[b.v], s[ch.nsel + b.ok], sg = dom.imp(recs[k], b.little, b.sign >= 0)
        if b.sign >= 0:
            s[ch.nsel + b.sign] = sg
    for o in ch.ops:
        dom.op(o, v, s)
    return ([v[i] for i in ch.outs], [dom.exp(v[b.v], b.little, s[b.sign] if b.sign >= 0 else None) for b in ch.bouts], [s[i] for i in ch.pouts])


# ---------------------------------------------------------------------------------------------------------------- the oracle
class _OracleDom:
    def __init__(self, oracle, P):
        self.o, self.P, self.nb = oracle, P, oracle.primes[P][3]
        self.f = lambda name: oracle.fn(name, P)

    def new(self, src=None):
        return self.o.arr(self.P, list(src) if src is not None else None)

    def imp(self, rec, little, sign):
        b = bytes(rec)[::-1] if little else bytes(rec)
        sg = b[0] >> 7
        if sign:
            b = bytes([b[0] & 0x7f]) + b[1:]
        z = self.new()
        ok = self.f("modimp")(b, z)
        return z, int(ok), sg

    def exp(self, val, little, sign):
        import ctypes
        buf = ctypes.create_string_buffer(self.nb)
        self.f("modexp")(val, buf)
        b = buf.raw
        if sign is not None:
            b = bytes([b[0] | ((sign << 7) & 0xff)]) + b[1:]
        return b[::-1] if little else b

    def op(self, o, v, s):
        f, op = self.f, o.op
        a, b = v.get(o.a), v.get(o.b)
        z = self.new()
        if op in ("modmul", "modadd", "modsub", "modadd_lazy", "modsub_lazy"):
            f(op)(a, b, z)
        elif op in ("modsqr", "modneg", "nres", "redc", "modcpy", "modneg_lazy", "modpro"):
            f(op)(a, z)
        elif op == "modinv":                                     # followed by the library's normalisation: redc, nres
            t = self.new()
            f(op)(a, b, z)
            f("redc")(z, t)
            f("nres")(t, z)
        elif op == "modsqrt":
            f(op)(a, b, z)
        elif op == "modqr":
            s[o.dst] = int(f(op)(b, a))
            return
        elif op == "modmli":
            f(op)(a, o.imm, z)
        elif op in ("modint", "mod2r"):
            f(op)(o.imm, z)
        elif op in ("modone", "modzer"):
            f(op)(z)
        elif op in ("modnsqr", "modhaf", "modshl", "modshr", "modfsb", "flatten"):      # a copy and an in-place call
            z = self.new(a)
            r = f(op)(z) if op in ("modhaf", "modfsb", "flatten") else f(op)(z, o.imm) if op == "modnsqr" else f(op)(o.imm, z)
            if o.sdst >= 0:
                s[o.sdst] = int(r)
        elif op == "modcmv":                                     # copy f, then move g over it under d
            z = self.new(b)
            f(op)(s[o.sa], a, z)
        elif op == "modcsw":
            z, z2 = self.new(a), self.new(b)
            f(op)(s[o.sa], z, z2)
            v[o.dst2] = z2
        elif op in ("modis0", "modis1", "modsign"):
            s[o.dst] = int(f(op)(a))
            return
        elif op == "modcmp":
            s[o.dst] = int(f(op)(a, b))
            return
        elif op in fuse._INT_OPS:
            d, e = s[o.sa], s.get(o.sb)
            s[o.dst] = {"lnot": lambda: 1 - d, "land": lambda: d & e, "lor": lambda: d | e, "lxor": lambda: d ^ e}[op]()
            return
        else:
            raise AssertionError(op)
        v[o.dst] = z


def run_oracle(ch: Chain, oracle, rows, shared, sels, records):
    """rows[k][j]: the limbs of element j of input batch k; shared[k]: limbs; sels[k][j]: 0 / 1; records[k][j]: bytes, as the chain's
    declaration of that input reads them.  Returns (element outputs [k][j] as lists of words, byte outputs [k][j] as bytes, int outputs
    [k][j]); the words of a value of limb_free() are those of its redc"""
    assert ch.wl == 64 and ch.prime in ORACLE_PRIMES
    dom = _OracleDom(oracle, ch.prime)
    n = len(rows[0]) if rows else len(records[0])
    free = limb_free(ch)
    sh = [dom.new(r) for r in shared]
    E, B, I = [[] for _ in ch.outs], [[] for _ in ch.bouts], [[] for _ in ch.pouts]
    for j in range(n):
        e, b, i = _walk(ch, dom, [dom.new(r[j]) for r in rows], sh, [int(d[j]) for d in sels], [r[j] for r in records])
        for k, x in enumerate(e):
            if ch.outs[k] in free:
                t = dom.new()
                dom.f("redc")(x, t)
                x = t
            E[k].append(list(x))
        for k, x in enumerate(b):
            B[k].append(x)
        for k, x in enumerate(i):
            I[k].append(x)
    return E, B, I


# ---------------------------------------------------------------------------------------------------------------- call by call through Field
class _CallsDom:
    def __init__(self, F, n):
        import torch
        self.F, self.n, self.torch = F, n, torch

    def imp(self, rec, little, sign):
        torch = self.torch
        b = torch.flip(rec, [1]).contiguous() if little else rec.clone()
        sg = (b[:, 0] >> 7).to(torch.int32)
        if sign:
            b[:, 0] &= 0x7f
        val, ok = self.F.modimp(b)
        return val, ok, sg

    def exp(self, val, little, sign):
        torch = self.torch
        b = self.F.modexp(val)
        if sign is not None:
            b[:, 0] |= (sign << 7).to(torch.uint8)
        return torch.flip(b, [1]).contiguous() if little else b

    def op(self, o, v, s):
        F, op, n = self.F, o.op, self.n
        a, b = v.get(o.a), v.get(o.b)
        if op in ("modmul", "modadd", "modsub", "modadd_lazy", "modsub_lazy", "modcmp"):
            z = getattr(F, op)(a, b)
        elif op in ("modsqr", "modneg", "nres", "redc", "modcpy", "modneg_lazy", "modpro", "modis0", "modis1", "modsign"):
            z = getattr(F, op)(a)
        elif op in ("modinv", "modsqrt"):
            z = getattr(F, op)(a, b)
        elif op == "modqr":
            z = F.modqr(b, a)
        elif op == "modmli":
            z = F.modmli(a, o.imm)
        elif op in ("modint", "mod2r"):
            z = getattr(F, op)(o.imm, n)
        elif op in ("modone", "modzer"):
            z = getattr(F, op)(n)
        elif op in ("modnsqr", "modhaf", "modshl", "modshr", "modfsb", "flatten"):
            z = a.clone()
            r = getattr(F, op)(z) if op in ("modhaf", "modfsb", "flatten") else F.modnsqr(z, o.imm) if op == "modnsqr" else getattr(F, op)(o.imm, z)
            if o.sdst >= 0:
                s[o.sdst] = r
        elif op == "modcmv":
            z = b.clone()
            F.modcmv(s[o.sa].contiguous(), a, z)
        elif op == "modcsw":
            z, z2 = a.clone(), b.clone()
            F.modcsw(s[o.sa].contiguous(), z, z2)
            v[o.dst2] = z2
        elif op in fuse._INT_OPS:
            d, e = s[o.sa], s.get(o.sb)
            z = {"lnot": lambda: 1 - d, "land": lambda: d & e, "lor": lambda: d | e, "lxor": lambda: d ^ e}[op]()
        else:
            raise AssertionError(op)
        (s if op in fuse._PREDS or op in fuse._INT_OPS else v)[o.dst] = z


def run_calls(ch: Chain, F, elems, shared, sels, recs):
    """the same walk through the methods of Field(P, wl): elems flat contiguous device batches [N, n], shared: broadcast batches of that
    shape, sels int32 [n], recs uint8 [n, Nbytes].  Returns (element outputs, byte outputs, int outputs) as device tensors; inputs are
    left as they were"""
    n = elems[0].shape[1] if elems else recs[0].shape[0]
    return _walk(ch, _CallsDom(F, n), elems, shared, sels, recs)


# ---------------------------------------------------------------------------------------------------------------- the model
class MV(NamedTuple):
    """what the model knows of an element value: v the internal-form integer mod p (None: undetermined), x the exact integer the limbs
    spell where that is known, sq (modsqrt): the internal-form value whose root this is"""
    v: Optional[int]
    x: Optional[int] = None
    sq: Optional[int] = None


_UNKNOWN = MV(None)
_NOINT = None                                                    # an int the model cannot say


class _ModelDom:
    def __init__(self, fp):
        self.fp, self.p = fp, fp.p
        self.R = fp.R % fp.p if fp.montgomery else 1
        self.Ri = pow(self.R, -1, fp.p)
        self.mont = fp.montgomery

    def elem(self, row):
        """an operand given as limbs: the exact integer where the limbs are digits"""
        fp = self.fp
        x = fp.from_limbs(row)
        return MV(x % self.p, x if all(0 <= l < (1 << fp.radix) for l in row[:-1]) and row[-1] >= 0 else None)

    def plain(self, v):
        return v * self.Ri % self.p

    def qr(self, v):
        x = self.plain(v)
        return int(x == 0 or pow(x, (self.p - 1) // 2, self.p) == 1)

    def imp(self, rec, little, sign):
        x = int.from_bytes(bytes(rec), "little" if little else "big")
        top = 8 * self.fp.nbytes - 1
        sg = x >> top
        if sign:
            x &= (1 << top) - 1
        ok = int(x < self.p)
        y = x if ok else x - self.p
        if x >= 2 * self.p:                                      # modfsb takes p off once: beyond 2p what modimp leaves is not a reduced element, and
            return _UNKNOWN, ok, sg                              # what field.c makes of one (modis0's test of the upper limbs, say) is its own
        return MV(y * self.R % self.p, None if self.mont else y), ok, sg

    def exp(self, val, little, sign):
        if val.v is None or sign is _NOINT:
            return None
        x = self.plain(val.v)
        if sign is not None:
            x |= (sign & 1) << (8 * self.fp.nbytes - 1)
        return x.to_bytes(self.fp.nbytes, "little" if little else "big")

    def op(self, o, v, s):
        p, R, Ri, op = self.p, self.R, self.Ri, o.op
        a, b = v.get(o.a), v.get(o.b)
        isint = op in fuse._PREDS or op in fuse._INT_OPS
        unknown = (a is not None and a.v is None) or (b is not None and b.v is None and op not in fuse._WITH_H)
        if isint:
            if op in fuse._INT_OPS:
                d, e = s[o.sa], s.get(o.sb, 0)
                s[o.dst] = None if d is None or e is None else {"lnot": 1 - d, "land": d & e, "lor": d | e, "lxor": d ^ e}[op]
            elif unknown:
                s[o.dst] = None
            elif op == "modqr":
                s[o.dst] = self.qr(a.v)
            elif op == "modcmp":
                s[o.dst] = int(a.v == b.v)
            else:
                x = self.plain(a.v)
                s[o.dst] = {"modis0": int(x == 0), "modis1": int(x == 1), "modsign": x & 1}[op]
            return
        z = _UNKNOWN
        if op == "modcmv":
            d = s[o.sa]
            z = _UNKNOWN if d is None else a if d else b
        elif op == "modcsw":
            d = s[o.sa]
            z, v[o.dst2] = (_UNKNOWN, _UNKNOWN) if d is None else (b, a) if d else (a, b)
        elif op in ("modone", "modzer", "modint", "mod2r"):
            if op == "mod2r":
                x = 0 if o.imm >= 8 * self.fp.nbytes else 1 << o.imm
            else:
                x = {"modone": 1, "modzer": 0}.get(op, o.imm)
            if x >= 0:                                           # (a negative modint is the word (spint)k: not a field constant)
                z = MV(x * R % p, x if not self.mont or x == 0 else None)
        elif unknown:
            if o.sdst >= 0:
                s[o.sdst] = None
        elif op in ("modmul", "modsqr"):
            z = MV(a.v * (a.v if op == "modsqr" else b.v) * Ri % p)
        elif op in ("modadd", "modadd_lazy"):
            z = MV((a.v + b.v) % p)
        elif op in ("modsub", "modsub_lazy"):
            z = MV((a.v - b.v) % p)
        elif op in ("modneg", "modneg_lazy"):
            z = MV(-a.v % p)
        elif op == "modmli":
            z = MV(a.v * o.imm % p)
        elif op == "nres":
            z = MV(a.v * R % p, None if self.mont else a.x)
        elif op == "redc":
            z = MV(a.v * Ri % p, a.v * Ri % p)
        elif op == "modcpy":
            z = a
        elif op == "modnsqr":
            x = a.v
            for _ in range(o.imm):
                x = x * x * Ri % p
            z = MV(x, a.x if o.imm == 0 else None)
        elif op == "modhaf":
            z = MV(a.v * pow(2, -1, p) % p)
        elif op == "modinv":
            x = self.plain(a.v)
            y = (pow(x, -1, p) if x else 0) * R % p
            z = MV(y, None if self.mont else y)                  # (normalised: canonical where nres is a copy)
        elif op == "modpro":
            z = MV(pow(self.plain(a.v), self.fp.pe, p) * R % p)
        elif op == "modsqrt":
            z = MV(None, None, a.v) if self.qr(a.v) else _UNKNOWN
        elif op == "modshl":
            # the top limb takes the bits shifted up, in a word: beyond the word the integer is no longer a << k
            fp = self.fp
            top = (fp.n + 1 if a.x is None else max(a.x.bit_length(), 1)) - fp.radix * (fp.nlimbs - 1) + o.imm
            if top <= fp.wl - 1:
                z = MV((a.v << o.imm) % p, None if a.x is None else a.x << o.imm)
        elif op == "modshr":
            if a.x is None:
                s[o.sdst] = None
            else:
                z, s[o.sdst] = MV((a.x >> o.imm) % p, a.x >> o.imm), a.x & ((1 << o.imm) - 1)
        elif op == "modfsb":
            if a.x is None or a.x >= 2 * p:
                s[o.sdst] = None
            else:
                y = a.x - p if a.x >= p else a.x
                z, s[o.sdst] = MV(y, y), int(a.x < p)
        elif op == "flatten":
            if a.x is None:
                s[o.sdst] = None
            else:
                z, s[o.sdst] = a, 0
        else:
            raise AssertionError(op)
        v[o.dst] = z


def run_model(ch: Chain, fp, rows, shared, sels, records):
    """the chain on Python integers; the arguments of run_oracle (rows of unsigned words of the chain's word length).  Returns (element
    outputs [k][j] as MV, byte outputs [k][j] as bytes or None, int outputs [k][j] as int or None)"""
    dom = _ModelDom(fp)
    n = len(rows[0]) if rows else len(records[0])
    sh = [dom.elem(r) for r in shared]
    E, B, I = [[] for _ in ch.outs], [[] for _ in ch.bouts], [[] for _ in ch.pouts]
    for j in range(n):
        e, b, i = _walk(ch, dom, [dom.elem(r[j]) for r in rows], sh, [int(d[j]) for d in sels], [r[j] for r in records])
        for k, x in enumerate(e):
            E[k].append(x)
        for k, x in enumerate(b):
            B[k].append(x)
        for k, x in enumerate(i):
            I[k].append(x)
    return E, B, I


def model_agrees(fp, mv: MV, row, free=False) -> Optional[bool]:
    """one element output (unsigned words) against the model: None where the model is undetermined.  free: the words are those of redc"""
    dom = _ModelDom(fp)
    row = list(row)
    if row[-1] >> (fp.wl - 1):                                   # the top limb is a signed word (field.c's sspint)
        row[-1] -= 1 << fp.wl
    x = fp.from_limbs(row)
    if mv.sq is not None:                                        # a square root: through its square
        y = x % fp.p if not free else x * dom.R % fp.p
        return y * y * dom.Ri % fp.p == mv.sq
    if mv.v is None:
        return None
    if free:
        return x == dom.plain(mv.v)
    return x % fp.p == mv.v and (mv.x is None or x == mv.x)


# ---------------------------------------------------------------------------------------------------------------- the test batch
def fp_of(P, wl):
    from modarith_amd import generate as gen
    return gen.find_field(P, wl=wl, built=True)[0]


def progenitor_row(fp, row):
    """the limbs of modpro of the element `row` spells, canonical: what a shared operand passed as h holds"""
    dom = _ModelDom(fp)
    return fp.to_limbs(pow(dom.plain(fp.from_limbs(row) % fp.p), fp.pe, fp.p) * dom.R % fp.p)


def make_batch(ch: Chain, n: int, seed: int = 0):
    """the operands of one program on the CPU: (rows, shared, sels, records) as run_oracle takes them.  Elements: the pool of
    tests/test_gpu_fuse_pred.py (_pool_values, and _pairs for every second batch, so that modcmp takes both values), then seeded
    integers below 2p, as to_limbs spells them; records: the pools of tests/test_gpu_fuse_bytes.py (plain big-endian records) and of
    tests/test_gpu_fuse_le.py (little-endian or signed ones): the integers the records spell;
    shared operands: seeded integers below 2p, a progenitor where the program says so; selectors: seeded bits"""
    from tests.test_gpu_fuse_bytes import _pool as _bytes_pool
    from tests.test_gpu_fuse_le import _pool
    from tests.test_gpu_fuse_pred import _pairs
    P, wl = ch.prime, ch.wl
    fp = fp_of(P, wl)
    rng = random.Random(9000 + 131 * seed + fp.nlimbs + wl)
    vals, other = _pairs(P, wl)
    rows = []
    for k in range(ch.nin):
        base = (vals, other, vals[7:] + vals[:7])[k % 3]
        if k >= 3:
            base = base[::-1]
        ints = (list(base) * (n // len(base) + 1))[:n] if n <= len(base) else list(base) + [rng.randrange(0, 2 * fp.p) for _ in range(n - len(base))]
        if k == 1 and n > len(base):                             # equal pairs beyond the directed ones too
            first = [fp.from_limbs(r) for r in rows[0]]
            ints = [first[j] if j % 4 == 0 else x for j, x in enumerate(ints)]
        rows.append([fp.to_limbs(x) for x in ints])
    shared = [fp.to_limbs(rng.randrange(0, 2 * fp.p)) for _ in ch.sh_idx]
    for h, x in ch.notes["progenitor_of"].items():
        shared[ch.sh_idx.index(h)] = progenitor_row(fp, shared[ch.sh_idx.index(x)])
    sels = [[rng.randrange(2) for _ in range(n)] for _ in range(ch.nsel)]
    records = []
    for k, b in enumerate(ch.bins):
        if b.little or b.sign >= 0:
            ints = _pool(fp, 20 + k + seed, signed=b.sign >= 0, count=max(n, 16))[:n]
        else:                                                    # plain big-endian records: the pool of tests/test_gpu_fuse_bytes.py
            ints = _bytes_pool(P, wl, 10 + k + seed)[:n]
        records.append([x.to_bytes(fp.nbytes, "little" if b.little else "big") for x in ints])
    return rows, shared, sels, records


# ---------------------------------------------------------------------------------------------------------------- mutants
def _clone(ch: Chain, **changed) -> Chain:
    import copy
    m = copy.copy(ch)
    for k, val in changed.items():
        setattr(m, k, val)
    return m


def value_numbers(ch: Chain):
    """a number per value and per int such that two with the same number are the same by construction: modcpy(x) is x, modcmv(d, x, x)
    and both halves of modcsw(d, x, x) are x, d & d and d | d are d; operations that commute are numbered with sorted operands"""
    table, vn, sn = {}, {}, {}
    num = lambda key: table.setdefault(key, len(table))
    for i in ch.in_idx + ch.sh_idx + [b.v for b in ch.bins]:
        vn[i] = num(("v", i))
    for k in range(ch.nsel):
        sn[k] = num(("s", k))
    for b in ch.bins:
        sn[ch.nsel + b.ok] = num(("flag", b.v))
        if b.sign >= 0:
            sn[ch.nsel + b.sign] = num(("sign", b.v))
    for o in ch.ops:
        a, b, sa, sb = vn.get(o.a), vn.get(o.b), sn.get(o.sa), sn.get(o.sb)
        if o.op in ("land", "lor") and sa == sb:
            sn[o.dst] = sa
        elif o.op in fuse._INT_OPS:
            sn[o.dst] = num((o.op,) + tuple(sorted(x for x in (sa, sb) if x is not None)))
        elif o.op in fuse._PREDS:
            sn[o.dst] = num((o.op,) + (tuple(sorted((a, b))) if o.op == "modcmp" else (a, b)))
        elif o.op == "modcpy" or (o.op in ("modcmv", "modcsw") and a == b):
            vn[o.dst] = a
            if o.dst2 >= 0:
                vn[o.dst2] = a
        else:
            ab = tuple(sorted((a, b))) if o.op in ("modmul", "modadd", "modadd_lazy") else (a, b)
            vn[o.dst] = num((o.op, o.imm, sa) + ab)
            if o.dst2 >= 0:
                vn[o.dst2] = num((o.op, "second", sa) + ab)
            if o.sdst >= 0:
                sn[o.sdst] = num((o.op, "int", o.imm, a))
    return vn, sn


def mutants(ch: Chain):
    """single-operation mutants of the live operations: [(what, chain)].  Neutral ones (both operands the same value) are left out"""
    live = set(live_ops(ch))
    out = []
    swap = lambda k, o: _clone(ch, ops=ch.ops[:k] + [o] + ch.ops[k + 1:])
    _, sd = defined_by(ch)
    vn, sn = value_numbers(ch)
    for k, o in enumerate(ch.ops):
        if k not in live or (o.b >= 0 and o.op not in fuse._WITH_H and vn[o.a] == vn[o.b]):
            continue
        if o.op in ("modsub", "modcmv") and o.a != o.b:
            out.append(("op %d: operands of %s swapped" % (k, o.op), swap(k, o._replace(a=o.b, b=o.a))))
        if o.op == "modcsw" and o.a != o.b:
            out.append(("op %d: dst and dst2 of modcsw swapped" % k, swap(k, o._replace(dst=o.dst2, dst2=o.dst))))
        if o.op in ("modcmv", "modcsw") and o.a != o.b:
            # another int of the chain that is defined by then and is 0 / 1: the nearest one below, else the nearest above
            known = [i for i in range(ch.nsel + ch.npred) if sn.get(i) != sn[o.sa] and (i < ch.nsel or i not in sd or ch.ops.index(sd[i]) < k)
                     and not (i in sd and sd[i].op == "modshr" and sd[i].imm != 1)]
            if known:
                other = max([i for i in known if i < o.sa] or [min(known)])
                out.append(("op %d: selector s%d of %s replaced by s%d" % (k, o.sa, o.op, other), swap(k, o._replace(sa=other))))
        if len(ch.sh_idx) > 1:
            for side in ("a", "b"):
                x = getattr(o, side)
                if x in ch.sh_idx and o.op not in fuse._INT_OPS:
                    other = ch.sh_idx[(ch.sh_idx.index(x) + 1) % len(ch.sh_idx)]
                    if other != (o.b if side == "a" else o.a) or o.op in fuse._WITH_H:
                        out.append(("op %d: shared operand v%d of %s replaced by v%d" % (k, x, o.op, other), swap(k, o._replace(**{side: other}))))
    for k, b in enumerate(ch.bouts):
        out.append(("byte output %d: little flipped" % k, _clone(ch, bouts=ch.bouts[:k] + [b._replace(little=not b.little)] + ch.bouts[k + 1:])))
    vlive = {x for j in live for x in (ch.ops[j].a, ch.ops[j].b)} | set(ch.outs) | {b.v for b in ch.bouts}
    for k, b in enumerate(ch.bins):
        if b.v in vlive:
            out.append(("byte input %d: little flipped" % k, _clone(ch, bins=ch.bins[:k] + [b._replace(little=not b.little)] + ch.bins[k + 1:])))
    return out


# ---------------------------------------------------------------------------------------------------------------- coverage of a set of programs
_PRED_KINDS = fuse._PREDS + fuse._INT_OPS


def value_kinds(ch: Chain):
    """{value index: its kind as an operand, one of ELEM_KINDS} and {int index: its source, one of INT_KINDS}"""
    vd, sd = defined_by(ch)
    vk = {}
    for i in range(ch.nvals):
        vk[i] = ("in" if i in ch.in_idx else "sh" if i in ch.sh_idx else "byte" if any(b.v == i for b in ch.bins) else "lazy" if i in ch.lazy
                 else "const" if i in vd and vd[i].op in _CONSTS else "res")
    sk = {k: "sel" for k in range(ch.nsel)}
    for b in ch.bins:
        sk[ch.nsel + b.ok] = "flag"
        if b.sign >= 0:
            sk[ch.nsel + b.sign] = "sign"
    sk.update({i: o.op for i, o in sd.items()})
    return vk, sk


def required(P: str, wl: int):
    """the conditions the seed set of one case has to meet, as tokens"""
    lazy = [o for o in fuse._OPS if o.endswith("_lazy")]
    need = {("op", o) for o in fuse._OPS if wl == 64 or o not in lazy}
    need |= {("operand", k, pos) for k in ELEM_KINDS if wl == 64 or k != "lazy" for pos in "lru"}
    # (a selector is the caller's own array: the builder refuses it as an output)
    need |= {("int", k, use) for k in INT_KINDS for use in ("cmv", "csw", "out") if (k, use) != ("sel", "out")}
    need |= {("feature", f) for f in ("same operand twice", "value output twice", "input output unchanged", "byte input to byte output", "dead value",
                                      "only int outputs", "h: progenitor", "h: shared")}
    need |= {(side, what, on) for side in ("bin", "bout") for what in ("little", "sign") for on in (False, True)}
    need |= {("both", k) for k in _PRED_KINDS}
    return need


def covered(ch: Chain, ints_of=None):
    """the tokens of required() one program meets.  ints_of(chain) -> the int outputs of an interpreter over the test batch, for the
    `both` tokens (every predicate and int expression takes 0 and 1): called with a copy of the chain that outputs every such int"""
    vk, sk = value_kinds(ch)
    vd, sd = defined_by(ch)
    got = set()
    for o in ch.ops:
        got.add(("op", o.op))
        if o.op in fuse._INT_OPS:
            continue
        two = fuse._OPS[o.op] == 2
        if o.a >= 0:
            got.add(("operand", vk[o.a], "l" if two else "u"))
        if o.b >= 0 and two:
            got.add(("operand", vk[o.b], "r"))
            if o.a == o.b:
                got.add(("feature", "same operand twice"))
        if o.op in ("modcmv", "modcsw"):
            got.add(("int", sk[o.sa], o.op[3:]))
        if o.op in fuse._WITH_H and o.b >= 0:
            got.add(("feature", "h: shared" if o.b in ch.sh_idx else "h: progenitor"))
    got |= {("int", sk[i], "out") for i in ch.pouts}
    shown = ch.outs + [b.v for b in ch.bouts]
    if len(set(ch.outs)) < len(ch.outs) or len({b.v for b in ch.bouts}) < len(ch.bouts):
        got.add(("feature", "value output twice"))
    if set(ch.in_idx) & set(ch.outs):
        got.add(("feature", "input output unchanged"))
    if {b.v for b in ch.bins} & {b.v for b in ch.bouts}:
        got.add(("feature", "byte input to byte output"))
    if len(live_ops(ch)) < len(ch.ops):
        got.add(("feature", "dead value"))
    if ch.pouts and not shown:
        got.add(("feature", "only int outputs"))
    for side, recs in (("bin", ch.bins), ("bout", ch.bouts)):
        got |= {(side, "little", r.little) for r in recs} | {(side, "sign", r.sign >= 0) for r in recs}
    if ints_of is not None:
        idx = [i for i, o in sd.items() if o.op in _PRED_KINDS]
        if idx:
            for i, col in zip(idx, ints_of(_clone(ch, outs=[], bouts=[], pouts=idx))):
                if {0, 1} <= set(col):
                    got.add(("both", sd[i].op))
    return got


# ---------------------------------------------------------------------------------------------------------------- command line
def body_of(ch: Chain) -> str:
    src = ch.source()
    return src[src.index("template <class F> MA_DEV void body("):src.index("// EPT elements of a lane")].rstrip()


RESOURCES = "profiles/chain_programs_resources.json"
_RES_KEYS = ("vgpr_count", "agpr_count", "vgpr_spill_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def resource_key(profile, seed, P, wl, ept=None):
    return "rp_%s_%d/%s/w%d%s" % (profile, seed, P, wl, "/ept%d" % ept if ept else "")


def write_resources(path=None):
    """builds every unit of every case (reused where current) and writes registers, spilled registers, scratch and LDS of each of its
    gfx950 kernels, as tools/kernel_resources.py reads them from the objects, to profiles/chain_programs_resources.json.  Recorded, not
    asserted -- tests/test_chain_programs_cpu.py asserts the one claim, and that this file names the units of the seed set"""
    import json
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_resources
    from modarith_amd import generate as gen
    out = {}
    for (P, wl), built in build_all(available_cases(), workers=min(16, len(os.sched_getaffinity(0)))).items():
        for (pr, s, ept), f in built.items():
            obj = f.path.replace("libmodarith_amd_chain_", "chain_")[:-3] + ".o"
            if not os.path.exists(obj):                          # (a plug-in that came without its object)
                f.chain.build(plugin_dir=plugin_dir(ept), force=True, **({"ept": ept} if ept else {}))
            out[resource_key(pr, s, P, wl, ept)] = {re.sub(r"\(.*", "", k["name"].replace("(anonymous namespace)::", "")): {x: k[x] for x in _RES_KEYS}
                                                   for k in kernel_resources.kernels_of(obj)}
    what = ("registers, spilled registers, scratch (private_segment_fixed_size, bytes) and LDS of the gfx950 kernels of every program of tests/chain_programs.py "
            "SEEDS; written by `python -m tests.chain_programs --resources`; recorded, not asserted, except: no scratch at one element per lane for a "
            "program without a long exponentiation (tests/test_chain_programs_cpu.py)")
    with open(path or os.path.join(root, RESOURCES), "w") as fh:
        json.dump({"what": what, "programs": out}, fh, indent=1, sort_keys=True)
        fh.write("\n")
    return out


def main(argv):
    if argv == ["--resources"]:
        print("%d units written to %s" % (len(write_resources()), RESOURCES))
        return 0
    if len(argv) != 4:
        print("usage: python -m tests.chain_programs <prime> <wl> <seed> <profile: %s>\n       python -m tests.chain_programs --resources" % " | ".join(PROFILES))
        return 2
    ch = random_chain(argv[0], int(argv[1]), int(argv[2]), argv[3])
    print(ch.text.replace("; ", ";\n"))
    print()
    print(body_of(ch))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
