"""The 32-bit word form of csrc/field.h against the reference's emitted C at word length 32, on the HOST.

tools/field_w32_host.hip compiles ma32::Field<P_<PRIME>_W32> (MA_WL = 32: spint = uint32_t, dpint = uint64_t) for the CPU with hipcc;
tests/golden/field_w32_<PRIME>.json.xz holds, for the 28 functions the reference emits without the external addchain tool, its
outputs on a pool of canonical, [p, 2p), budget-edge, all-maximal and arbitrary 32-bit operands (tests/w32_inputs.py).  Every record
is compared word for word: no tolerance, none skipped (the number compared must equal the number in the fixture).  modpro / modinv /
modsqrt / modqr -- whose limbs depend on an addition chain the reference takes from that tool -- are pinned by VALUE after redc
against Python integers on the same pool."""
import ctypes
import os
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_long, c_ubyte, c_uint32

import pytest

from tests import w32_inputs as wi
from tests.golden import gio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
U32P = POINTER(c_uint32)

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (host compile of the HIP headers)")


class Host:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        self.lib.w32h_call.argtypes = [c_char_p, c_char_p, U32P, U32P, U32P, U32P, c_long, POINTER(c_ubyte)]
        self.lib.w32h_call.restype = c_long

    def call(self, prime, fn, a=None, b=None, k=0, data=None):
        """-> (ret, out0, out1, bytes)"""
        N, _, _, NB, _ = wi.SHAPES[prime]
        arr = lambda v: (c_uint32 * N)(*v) if v is not None else None
        o0, o1 = (c_uint32 * N)(), (c_uint32 * N)()
        buf = (c_ubyte * NB)(*(data or bytes(NB)))
        r = self.lib.w32h_call(prime.encode(), fn.encode(), arr(a), arr(b), o0, o1, k, buf)
        assert r > -1000, "%s %s: not dispatched (%d)" % (prime, fn, r)
        return r, list(o0), list(o1), bytes(buf)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("w32h"))
    cc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    csrc = os.path.join(ROOT, "modarith_amd", "csrc")
    so = os.path.join(tmp, "libfield_w32_host.so")
    cmd = [cc, "-O1", "-std=c++17", "-w", "-shared", "-fPIC", "--offload-host-only", "-I", os.path.join(csrc, "generated"), "-I", csrc,
           os.path.join(ROOT, "tools", "field_w32_host.hip"), "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    return Host(so)


def run_record(host, P, fn, row, pool):
    """run one fixture record; -> list of (got, expected) pairs"""
    U, M32 = wi.unpack, wi.M32
    if fn in ("modadd", "modsub", "modmul"):
        return [(host.call(P, fn, pool[row[0]], pool[row[1]])[1], U(row[2]))]
    if fn in ("modneg", "modsqr", "modcpy", "nres", "redc", "modhaf"):
        return [(host.call(P, fn, pool[row[0]])[1], U(row[1]))]
    if fn in ("prop", "flatten", "modfsb"):
        r, o, _, _ = host.call(P, fn, pool[row[0]])
        return [(o, U(row[1])), (r & M32, row[2])]
    if fn in ("modnsqr", "modmli"):
        return [(host.call(P, fn, pool[row[0]], k=row[1])[1], U(row[2]))]
    if fn in ("modis1", "modis0", "modsign"):
        return [(host.call(P, fn, pool[row[0]])[0], row[1])]
    if fn == "modcmp":
        return [(host.call(P, fn, pool[row[0]], pool[row[1]])[0], row[2])]
    if fn in ("modzer", "modone"):
        return [(host.call(P, fn)[1], U(row[0]))]
    if fn in ("modint", "mod2r"):
        return [(host.call(P, fn, k=row[0])[1], U(row[1]))]
    if fn == "modcmv":
        return [(host.call(P, fn, pool[row[1]], pool[row[2]], k=row[0])[1], U(row[3]))]
    if fn == "modcsw":
        _, g, f, _ = host.call(P, fn, pool[row[1]], pool[row[2]], k=row[0])
        return [(g, U(row[3])), (f, U(row[4]))]
    if fn == "modshl":
        return [(host.call(P, fn, pool[row[1]], k=row[0])[1], U(row[2]))]
    if fn == "modshr":
        r, o, _, _ = host.call(P, fn, pool[row[1]], k=row[0])
        return [(o, U(row[2])), (r, row[3])]
    if fn == "modexp":
        return [(host.call(P, fn, pool[row[0]])[3].hex(), row[1])]
    if fn == "modimp":
        r, o, _, _ = host.call(P, fn, data=bytes.fromhex(row[0]))
        return [(o, U(row[1])), (r, row[2])]
    raise AssertionError("no runner for " + fn)


EMITTED = ("prop", "flatten", "modfsb", "modadd", "modsub", "modneg", "modmli", "modmul", "modsqr", "modcpy", "modnsqr", "nres", "redc",
           "modis1", "modis0", "modzer", "modone", "modint", "modcmv", "modcsw", "modshl", "modshr", "modhaf", "mod2r", "modexp", "modimp",
           "modsign", "modcmp")


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_pool_is_the_shared_recipe(P):
    fx = gio.load("field_w32_%s.json" % P)
    assert [wi.unpack(s) for s in fx["pool"]] == wi.pool(P, fx["pool_extra"])
    N, R = wi.SHAPES[P][:2]
    pool = [wi.unpack(s) for s in fx["pool"]]
    top = (1 << (R + 2)) - 1
    assert [top] * N in pool and [wi.M32] * N in pool
    for pos in range(N):
        assert any(a[pos] == top and sum(v == top for v in a) == 1 for a in pool), "budget edge at limb %d" % pos


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_every_record_of_the_28_emitted_functions(host, P):
    fx = gio.load("field_w32_%s.json" % P)
    pool = [wi.unpack(s) for s in fx["pool"]]
    assert sorted(fx["records"]) == sorted(EMITTED)
    compared, bad = 0, []
    for fn in EMITTED:
        for k, row in enumerate(fx["records"][fn]):
            for got, want in run_record(host, P, fn, row, pool):
                if got != want:
                    bad.append((fn, k, row[:3], got, want))
            compared += 1
    assert not bad, "%d records differ, first: %r" % (len(bad), bad[:3])
    assert compared == fx["count"] == sum(len(v) for v in fx["records"].values())


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_chain_functions_by_value(host, P):
    """modpro modinv modsqrt modqr on the whole pool: x * inv == 1, sqrt^2 == x where modqr says so, modqr against Euler's criterion,
    modpro against x^PE; values after redc (which is exact for every representation the products return)"""
    N, R, n, _, p = wi.SHAPES[P]
    from modarith_amd.params import derive
    fp = derive(P, wl=32)
    Rinv = pow(fp.R, -1, p) if fp.montgomery else 1
    fx = gio.load("field_w32_%s.json" % P)
    val = lambda limbs: wi.value(P, host.call(P, "redc", limbs)[1])      # canonical for every product output (< 2p)
    done = skipped = 0
    for i, s in enumerate(fx["pool"]):
        a = wi.unpack(s)
        if wi.value(P, a) >= 2 * p or max(a[:-1]) >> R:
            # Pinned by value where the reference's arithmetic HAS a value: elements below 2p in digit form (limbs 0..N-2 below
            # 2^Radix, top limb unmasked) -- what its functions return and accept.  Beyond that the emitted C itself stops being
            # congruent mod p (X25519: hi = (spint)(tt >> 29) drops bits once a folded column passes 2^61, i.e. with a single limb at
            # 2^31 - 1; arbitrary words wrap the 64-bit columns).  Those elements are compared word for word through the 28 emitted
            # functions above -- modmul, modsqr and modnsqr, the only arithmetic the chains are made of, included.
            skipped += 1
            continue
        x = wi.value(P, a) * Rinv % p
        inv = val(host.call(P, "modinv", a)[1])
        assert inv * x % p == (1 if x else 0), (P, i)
        qr = host.call(P, "modqr", a)[0]
        assert qr == (1 if x == 0 or pow(x, (p - 1) // 2, p) == 1 else 0), (P, i)
        h = host.call(P, "modpro", a)[1]
        assert val(h) == pow(x, fp.pe, p), (P, i)
        if qr:
            rt = val(host.call(P, "modsqrt", a)[1])
            assert rt * rt % p == x, (P, i)
            assert val(host.call(P, "modsqrt", a, h)[1]) == rt
        # with the caller-supplied progenitor: the same values
        assert val(host.call(P, "modinv", a, h)[1]) == inv and host.call(P, "modqr", a, h)[0] == qr
        done += 1
    in_contract = sum(1 for t in wi.pool(P, fx["pool_extra"]) if wi.value(P, t) < 2 * p and not max(t[:-1]) >> R)
    assert done == in_contract and done + skipped == len(fx["pool"]) and done >= 25 + 2 * fx["pool_extra"]
