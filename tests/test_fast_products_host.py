"""Every prime's FAST product forms (csrc/field.h Field<P, true>: operands cut at P::SPLIT, three or four 64-bit accumulators per column,
the 64-bit column chain, the half-limb forms) and its exact ones (Field<P, false>), compiled for the HOST (tools/field_fast_host.hip) and
compared limb for limb with the CPU oracle at the edge of the limb budget -- inputs: tests/edge_inputs.py, the all-maximal pair of
operands among them, which is what the overflow proofs of emit.split_point / chain_ok / sparse_terms are about.  The oracle itself is
checked against Python integers on the same records.  CPU only; the gfx950 objects meet the same inputs in
tests/test_gpu_edge_products.py.

No tolerance anywhere: equality of 64-bit words, or of integers modulo p.  Records per prime: 20 000 through modmul / modsqr / nres /
redc (both policies, every record), 400 through modnsqr(k = 1, 2, 5) / modinv / modsqrt / modqr / modmli.

Findings about the reference's domain, as explicit rules (see _congruence_domain): the emitted field.c computes its column sums in
128-bit and one-word arithmetic that wraps for limbs this large in a few forms; there the oracle (like the reference) returns words
that are not congruent to the product any more.  The exact form must still return the same words, and does; the Python-integer
congruence is asserted where the column sums fit.
"""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_int, c_size_t, c_uint64

import numpy as np
import pytest

from modarith_amd import emit
from modarith_amd import generate as gen
from tests import edge_inputs as ei
from tests.util import derive_any, generated_tags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
ALL = list(emit.BUILT_PRIMES) + generated_tags()
UNITS = 4                       # translation units, compiled side by side (one compiler process each)
N_CHEAP, N_CHAIN = 20000, 400
FFH_FACTS = ("FAST", "CHAINED", "SPLIT4", "HALF", "HALF_OV", "MHALF", "MHALF_TRI", "SPLIT_SPARSE", "FOLD52", "SPLIT", "N", "RADIX", "MONTGOMERY",
             "EXACT_FAST")
# the forms of Field<P, true> that differ from the exact products; every one must have at least one user among the built primes
FAST_FORMS = ("SPLIT3", "SPLIT3_SPARSE", "CHAIN_PSEUDO", "CHAIN_MONTY", "SPLIT4", "HALF", "HALF_OV", "FOLD52", "MHALF", "MHALF_TRI")
U64P = POINTER(c_uint64)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (host compile of the HIP headers)")


class HostFields:
    """the shared libraries built from tools/field_fast_host.hip, one per unit; a call goes to the unit that holds the prime"""

    def __init__(self, libs):
        self.libs = libs
        self.where = {}
        for lib in libs:
            for pol in ("exact", "fast"):
                getattr(lib, "ffh_%s_modmul" % pol).argtypes = [c_char_p, U64P, U64P, U64P, c_size_t]
                for op in ("modsqr", "nres", "redc", "modinv", "modsqrt", "modqr"):
                    getattr(lib, "ffh_%s_%s" % (pol, op)).argtypes = [c_char_p, U64P, U64P, c_size_t]
                for op in ("modnsqr", "modmli"):
                    getattr(lib, "ffh_%s_%s" % (pol, op)).argtypes = [c_char_p, U64P, c_int, U64P, c_size_t]
            lib.ffh_facts.argtypes = [c_char_p, POINTER(c_int)]

    def _lib(self, P):
        if P not in self.where:
            out = (c_int * len(FFH_FACTS))()
            hit = [lib for lib in self.libs if lib.ffh_facts(P.encode(), out) == 0]
            assert len(hit) == 1, "%s is in %d units" % (P, len(hit))
            self.where[P] = hit[0]
        return self.where[P]

    def facts(self, P):
        out = (c_int * len(FFH_FACTS))()
        assert self._lib(P).ffh_facts(P.encode(), out) == 0
        return dict(zip(FFH_FACTS, [int(v) for v in out]))

    def call(self, policy, op, P, a, b=None, k=None):
        a = np.ascontiguousarray(a)
        c = np.empty_like(a)
        n = a.shape[1]
        f = getattr(self._lib(P), "ffh_%s_%s" % (policy, op))
        p = lambda x: x.ctypes.data_as(U64P)
        if op == "modmul":
            b = np.ascontiguousarray(b)
            rc = f(P.encode(), p(a), p(b), p(c), n)
        elif op in ("modnsqr", "modmli"):
            rc = f(P.encode(), p(a), int(k), p(c), n)
        else:
            rc = f(P.encode(), p(a), p(c), n)
        assert rc == 0, (P, op)
        return c


def _params_dir(tmp):
    """parameter headers of the generator mode's example moduli, emitted as modarith_amd.generate does (emit.header_text of the resolved
    modulus); the built-in ones are included from csrc/generated"""
    d = os.path.join(tmp, "generated_examples")
    os.makedirs(d, exist_ok=True)
    for arg, fam in gen.EXAMPLES:
        fp = gen.resolve(arg, fam)
        emit._write(os.path.join(d, "params_%s.h" % fp.name), emit.header_text(fp))
    return d


def build_host_fields(tmp, primes=ALL, params_override=None):
    """compile tools/field_fast_host.hip for `primes`, split over UNITS translation units whose include lists are written here from the
    list of primes (nothing hand-maintained).  params_override: {prime: path of another params header} (a scratch experiment)."""
    cc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    gdir = _params_dir(tmp)
    csrc = os.path.join(ROOT, "modarith_amd", "csrc")
    procs, sos = [], []
    for u in range(UNITS):
        mine = list(primes)[u::UNITS]
        if not mine:
            continue
        lst = os.path.join(tmp, "ffh_list_%d.inc" % u)
        with open(lst, "w") as f:
            for P in mine:
                hdr = (params_override or {}).get(P) or os.path.join(emit.GEN_DIR if P in emit.BUILT_PRIMES else gdir, "params_%s.h" % P)
                f.write('#include "%s"\n' % hdr)
            f.write("#define FFH_PRIMES(X) %s\n" % " ".join("X(%s)" % P for P in mine))
        so = os.path.join(tmp, "libfield_fast_host_%d.so" % u)
        cmd = [cc, "-O1", "-std=c++17", "-w", "-shared", "-fPIC", "--offload-host-only", "-I", os.path.join(csrc, "generated"), "-I", csrc,
               '-DFFH_LIST="%s"' % lst, os.path.join(ROOT, "tools", "field_fast_host.hip"), "-o", so]
        procs.append(subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
        sos.append(so)
    for p in procs:
        out, _ = p.communicate(timeout=900)
        assert p.returncode == 0, out[-3000:]
    return HostFields([ctypes.CDLL(so) for so in sos])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return build_host_fields(str(tmp_path_factory.mktemp("ffh")))


def test_include_list_covers_every_built_prime(host):
    """the units are written from emit.BUILT_PRIMES + generate.EXAMPLES, and every csrc/generated/params_*.h is one of them"""
    on_disk = sorted(f[len("params_"):-2] for f in os.listdir(emit.GEN_DIR) if f.startswith("params_") and f.endswith(".h"))
    assert on_disk == sorted(emit.BUILT_PRIMES)
    assert len(ALL) == len(set(ALL)) == len(emit.BUILT_PRIMES) + len(gen.EXAMPLES)
    for P in ALL:
        fp, f = derive_any(P), host.facts(P)
        assert (f["N"], f["RADIX"], f["MONTGOMERY"], f["SPLIT"]) == (fp.nlimbs, fp.radix, int(fp.montgomery), emit.split_point(fp)), P


def forms_of(f):
    """the FAST forms (FAST_FORMS) a prime's Field<P, true> runs, from the exported compile-time facts"""
    out = []
    half = f["HALF"] or f["HALF_OV"] or f["MHALF"] or f["MHALF_TRI"]
    if f["FOLD52"]:
        out.append("FOLD52")
    elif f["HALF_OV"]:
        out.append("HALF_OV")
    for k in ("HALF", "MHALF", "MHALF_TRI", "SPLIT4"):
        if f[k]:
            out.append(k)
    if f["FAST"] and not half:
        if f["CHAINED"]:
            out.append("CHAIN_MONTY" if f["MONTGOMERY"] else "CHAIN_PSEUDO")
        else:
            out.append("SPLIT3_SPARSE" if f["SPLIT_SPARSE"] else "SPLIT3")
    return out


def test_form_table(host):
    """every prime with a provable cut reports FAST; CHAINED and SPLIT_SPARSE are what the driver proves; the exact policy never runs a FAST
    form; and every FAST form has at least one user among the built primes (a form that loses its last user would silently go untested)"""
    users = {k: [] for k in FAST_FORMS}
    for P in ALL:
        fp, f = derive_any(P), host.facts(P)
        assert f["EXACT_FAST"] == 0, P
        if emit.split_point(fp) > 0:
            assert f["FAST"] == 1, P
        assert f["CHAINED"] == int(emit.chain_ok(fp)), P
        assert f["SPLIT_SPARSE"] == int(emit.split_is_sparse(fp)), P
        assert f["FAST"] == int(f["SPLIT"] > 0 or f["FOLD52"]), P
        for k in forms_of(f):
            users[k].append(P)
    print("FAST forms:", {k: v for k, v in users.items()})
    for k in FAST_FORMS:
        assert users[k], "no built prime instantiates the %s form" % k


def fast_differs(f):
    """Field<P, true> is other code than Field<P, false> (F::FAST reads 0 for SPLIT4, which is selected by FAST_ && !FAST)"""
    return bool(forms_of(f))


def _minv(fp):
    """v(modmul(a, b)) = v(a) v(b) / M (mod p): M = the Montgomery constant (2^(Radix * Nlimbs), one limb more under a virtual limb), 1
    for the pseudo-Mersenne family"""
    return pow(fp.R, -1, fp.p) if fp.montgomery else 1


def _mismatch(P, op, policy, j, a, b, got, want, extra=""):
    return "%s %s policy=%s element %d%s\n  a    = %s\n  b    = %s\n  got  = %s\n  want = %s" % (
        P, op, policy, j, extra, ei.hexrec(a, j), ei.hexrec(b, j) if b is not None else "-", ei.hexrec(got, j), ei.hexrec(want, j))


def _assert_equal(P, op, policy, a, b, got, want, extra=""):
    j = ei.first_diff(got, want)
    assert j is None, _mismatch(P, op, policy, j, a, b, got, want, extra)


def _run_set(host, ref, P, fp, policies, a, b, info):
    """every operation on one input set: policies == oracle, oracle == Python integers"""
    N, R, p = fp.nlimbs, fp.radix, fp.p
    n = a.shape[1]
    Minv = _minv(fp)
    M = fp.R if fp.montgomery else 1
    T, top = min(R + 2, 64), info["top"]
    va, vb = ei.values(fp, a), ei.values(fp, b)
    want = {"modmul": ref.modmul(a, b), "modsqr": ref.un("modsqr", a), "nres": ref.un("nres", a), "redc": ref.un("redc", a)}
    for op, w in want.items():
        for pol in policies:
            _assert_equal(P, op, pol, a, b if op == "modmul" else None, host.call(pol, op, P, a, b), w)
    # the oracle against Python integers, and the budget of its outputs
    dom = _congruence_domain(fp, a, b, va, vb)
    vw = {op: ei.values(fp, w) for op, w in want.items()}
    for j in range(n):
        x, y = va[j], vb[j]
        if dom["modmul"][j]:
            assert (vw["modmul"][j] - x * y * Minv) % p == 0, _mismatch(P, "modmul", "oracle vs integers", j, a, b, want["modmul"], want["modmul"])
        if dom["modsqr"][j]:
            assert (vw["modsqr"][j] - x * x * Minv) % p == 0, _mismatch(P, "modsqr", "oracle vs integers", j, a, None, want["modsqr"], want["modsqr"])
        if dom["redc"][j]:
            assert (vw["redc"][j] - x * Minv) % p == 0, _mismatch(P, "redc", "oracle vs integers", j, a, None, want["redc"], want["redc"])
        if dom["nres"][j]:
            assert (vw["nres"][j] - x * M) % p == 0, _mismatch(P, "nres", "oracle vs integers", j, a, None, want["nres"], want["nres"])
    if T < 64:
        for op, w in want.items():
            ok = dom["budget"][op]
            assert int(w[:, ok].max(initial=0)) < 1 << T, "%s %s: an output limb of the oracle leaves the budget 2^%d" % (P, op, T)
    # the chains, on the directed records and a slice of the mixtures and of the uniform ones
    lo = info["mixture"][0]
    idx = np.r_[0:min(lo, N_CHAIN - 64), info["mixture"][0]:info["mixture"][0] + 32, n - 32:n]
    ca, cva = np.ascontiguousarray(a[:, idx]), [va[j] for j in idx]
    lim = np.uint64(top)
    for k in (1, 2, 5):
        # the FAST squaring is defined on limbs inside the contract, link by link: a Montgomery square of an operand with the maximum in every
        # limb leaves a top limb beyond 2^(Radix+2) (see _congruence_domain "budget"), so from the second link on the unguarded FAST form is
        # compared on the records whose intermediate values -- the oracle's -- are inside the contract (the kernel votes per link: k_nsqr)
        w, inside = ca, np.ones(ca.shape[1], dtype=bool)
        for _ in range(k):
            inside &= (w <= lim).all(axis=0)
            w = ref.un("modsqr", w)
        for pol in policies:
            sel = inside if pol == "fast" else np.ones_like(inside)
            got = host.call(pol, "modnsqr", P, ca, k=k)
            _assert_equal(P, "modnsqr", pol, ca[:, sel], None, got[:, sel], w[:, sel], " k=%d (of the %d records inside the contract at every link)" % (k, sel.sum()))
        assert inside[:4].all()                                   # (the smallest classes stay inside)
    for k in (3, 121665):
        w = _ref_mli(ref, ca, k)
        for pol in policies:
            _assert_equal(P, "modmli", pol, ca, None, host.call(pol, "modmli", P, ca, k=k), w, " k=%d" % k)
    # modinv / modsqrt / modqr: x^PE by an addition chain.  The reference takes its chain from an external tool, the oracle and the engine
    # each have their own: the VALUES agree wherever every link is integer arithmetic, the words only after redc.  A record whose first
    # square leaves the budget (or the congruence domain) feeds the chain an operand outside the reference's domain, and what comes out
    # depends on the chain -- the exact form and the oracle differ there (M2519, 2^51 - 1 in every limb).  Such records are compared for
    # no policy: rule "chain" below, computed from the inputs.
    cdom = dom["chain"][idx] & np.array([v <= 2 * p for v in cva])
    z0 = list(idx).index(info["zero_like"][0])
    assert cdom[:2].all() and cdom[z0] and cdom[z0 + 1]          # 0 and 1 in every limb; 0 and p written as limbs (2p too, but for CONGRUENCE_FINDINGS)
    # ... plus values inside the reference's domain in its own limb form (below 2p, top limb unmasked), the edges of that domain first
    rng = np.random.default_rng(99)
    vals = [0, 1, 2, p - 2, p - 1, p, p + 1, 2 * p - 1] + [int.from_bytes(rng.bytes(fp.nbytes + 8), "little") % (2 * p) for _ in range(N_CHAIN - 8)]
    cc = np.ascontiguousarray(np.concatenate([ca[:, cdom], ei._u64([fp.to_limbs(v) for v in vals])], axis=1))
    ccv = [v for v, ok in zip(cva, cdom) if ok] + vals
    winv, wsqrt, wqr = ref.un("redc", ref.un("modinv", cc)), ref.un("redc", ref.un("modsqrt", cc)), ref.modqr(cc)
    for pol in policies:
        red = lambda x: host.call(pol, "redc", P, x)
        _assert_equal(P, "redc(modinv)", pol, cc, None, red(host.call(pol, "modinv", P, cc)), winv)
        _assert_equal(P, "redc(modsqrt)", pol, cc, None, red(host.call(pol, "modsqrt", P, cc)), wsqrt)
        qr = host.call(pol, "modqr", P, cc)
        assert not qr[1:].any() and np.array_equal(qr[0].astype(np.int32), wqr), (P, "modqr", pol, int(np.nonzero(qr[0].astype(np.int32) != wqr)[0][0]))
    vinv, vsqrt = ei.values(fp, winv), ei.values(fp, wsqrt)
    for i, raw in enumerate(ccv):
        x = raw * Minv % p                                      # the value the limbs stand for
        assert vinv[i] == (pow(x, -1, p) if x else 0), (P, "modinv vs integers", ei.hexrec(cc, i))
        euler = pow(x, (p - 1) // 2, p)
        # finding: the reference's modqr ends with "| modis0(x)", and modis0 reads the limbs of redc(x) as canonical; for a pseudo-Mersenne
        # modulus redc is modfsb (one conditional subtraction of p), canonical for values below 2p only.  Beyond, modqr answers 1 for a
        # non-residue (X25519, 2^53 - 1 in every limb) and 0 for 2p = 0: its answer is compared with the oracle's (above), with Euler's
        # criterion only for values below 2p
        if fp.montgomery or raw < 2 * p:
            assert int(wqr[i]) == int(euler in (0, 1)), (P, "modqr vs integers", ei.hexrec(cc, i))
        if euler in (0, 1):
            assert vsqrt[i] * vsqrt[i] % p == x, (P, "modsqrt vs integers", ei.hexrec(cc, i))
    return n, len(idx)


def _ref_mli(ref, a, k):
    from tests.util import oracle_mli, vp
    if ref.per_prime:
        return oracle_mli(ref.oracle, ref.P, a, k)
    c = np.empty_like(a)
    ref.G.lib.gen_batch_mli(ref.G.R, vp(a), int(k), vp(c), a.shape[1], a.shape[1])
    return c


CONGRUENCE_FINDINGS = ei.CONGRUENCE_FINDINGS


def _congruence_domain(fp, a, b, va, vb):
    """boolean [n] per operation: the records on which the Python-integer checks are asserted.  Computed from the inputs alone.
      modmul / modsqr   every record; for the moduli of CONGRUENCE_FINDINGS the tight records
      nres / redc       every record; pseudo-Mersenne moduli with Radix + 2 >= 63 (M607): records with limbs below 2^62 -- redc is
                        modfsb there, whose carry chain adds limbs as SIGNED words (prop), and 2^63 - 1 plus a carry is negative
      budget            the output limbs are below 2^(Radix+2): Montgomery products leave the top limb unmasked, the result is below
                        v(a) v(b) / M + p, so its top limb is inside the budget whenever v(a) v(b) / M + p < 2^(Radix Nlimbs + 2) -- true
                        of every product of field-function outputs, not of two operands with 2^(Radix+2) - 1 in every limb
                        (value 4 * 2^(Radix Nlimbs), product 16 M): asserted where the bound holds
      chain             modinv / modsqrt / modqr against pow(): as modmul"""
    n, R, N, p = a.shape[1], fp.radix, fp.nlimbs, fp.p
    every = np.ones(n, dtype=bool)
    q = np.uint64(1 << R)
    tight = lambda x, vx: (x[:-1] < q).all(axis=0) & np.array([v < 2 * p for v in vx])
    ta, tb = tight(a, va), tight(b, vb)
    found = fp.name in CONGRUENCE_FINDINGS
    lin = every
    if not fp.montgomery and R + 2 >= 63:
        lin = (a < np.uint64(1 << 62)).all(axis=0)
    dom = {"modmul": ta & tb if found else every, "modsqr": ta if found else every, "nres": lin, "redc": lin, "chain": ta if found else every}
    if fp.montgomery:
        lim, M = 1 << (R * N + 2), fp.R
        r2 = fp.from_limbs(fp.r2)
        dom["budget"] = {"modmul": np.array([x * y // M + p < lim for x, y in zip(va, vb)]), "modsqr": np.array([x * x // M + p < lim for x in va]),
                         "nres": np.array([x * r2 // M + p < lim for x in va]), "redc": np.array([x // M + p < lim for x in va])}
    else:
        dom["budget"] = {"modmul": dom["modmul"], "modsqr": dom["modsqr"], "nres": lin, "redc": lin}
    return dom


@pytest.mark.parametrize("P", ALL)
def test_fast_and_exact_products_vs_oracle(oracle, host, P):
    fp, f = derive_any(P), host.facts(P)
    ref = ei.Ref(oracle, P)
    H = f["SPLIT"] or (fp.radix + 2) // 2
    a, b, info = ei.build_inputs(fp, H, N_CHEAP, seed=20260 + ALL.index(P))
    if f["MONTGOMERY"]:                                          # the directed reduction digits really occur
        Q1 = (1 << fp.radix) - 1
        for kind, b0, target in (("redc_max", 1, Q1), ("nres_max", fp.r2[0], Q1), ("zero", 1, 0), ("zero", fp.r2[0], 0)):
            s, e = info["directed"][kind]
            assert all(ei.first_digit(fp, int(a[0, j]), b0) == target for j in range(s, e)), (P, kind)
            assert e > s or (kind == "nres_max" and fp.r2[0] % 2 == 0), (P, kind)
    if f["FOLD52"]:
        # the folded half-limb form of the 5 x 52 pseudo-Mersenne primes with a small mm equals the reference for limbs up to (2^64 - 1) / mm
        # only (kernels.h in_limb_budget): the exact form on the whole budget, the FAST form on a set drawn against that limit
        _run_set(host, ref, P, fp, ("exact",), a, b, info)
        limit = ((1 << 64) - 1) // fp.mm
        a2, b2, info2 = ei.build_inputs(fp, H, N_CHEAP, seed=30260 + ALL.index(P), limit=limit)
        assert info2["top"] == limit and int(a2.max()) == limit
        _run_set(host, ref, P, fp, ("exact", "fast"), a2, b2, info2)
    else:
        _run_set(host, ref, P, fp, ("exact", "fast"), a, b, info)
