"""Generated fields of the 32-bit word form against the reference's emitted C at word length 32, on the HOST.

The emitted params_<TAG>_w32.h (modarith_amd.emit.header_text) of every example of modarith_amd.generate.EXAMPLES_W32 is compiled
with csrc/field.h at MA_WL = 32 for the CPU into one library (tools/field_w32_gen_host.hip); tests/golden/field_w32gen_<TAG>.json.xz
holds, for the 28 functions the reference emits without the external addchain tool, the outputs of `pseudo.py 32` / `monty.py 32` on
a pool of canonical, [p, 2p), budget-edge, all-maximal and arbitrary 32-bit operands (tests/w32_gen_inputs.py).  Every record is
compared word for word: no tolerance, none skipped (the number compared must equal the number in the fixture).  modpro / modinv /
modsqrt / modqr are pinned by VALUE after redc against Python integers on the in-contract part of the pool, and the closure the
driver claims for the shared inversion (params.w32_inv_closure) is exercised at the edge of what w32_inv_in_contract admits."""
import ctypes
import os
import random
import shutil
import subprocess
from ctypes import POINTER, c_char_p, c_int, c_long, c_ubyte, c_uint32

import pytest

from modarith_amd import emit
from modarith_amd.params import w32_inv_closure, w32_inv_in_contract
from tests import w32_gen_inputs as gi
from tests.golden import gio
from tests.test_w32_host import EMITTED

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
U32P = POINTER(c_uint32)
TAGS = [t for t, _, _ in gi.examples()]



class Host:
    def __init__(self, so):
        self.lib = ctypes.CDLL(so)
        self.lib.w32h_call.argtypes = [c_char_p, c_char_p, U32P, U32P, U32P, U32P, c_long, POINTER(c_ubyte)]
        self.lib.w32h_call.restype = c_long
        self.lib.w32h_facts.argtypes = [c_char_p, POINTER(c_int)]

    def call(self, tag, fn, a=None, b=None, k=0, data=None):
        """-> (ret, out0, out1, bytes)"""
        fp = gi.params(tag)
        N, NB = fp.nlimbs, fp.nbytes
        arr = lambda v: (c_uint32 * N)(*v) if v is not None else None
        o0, o1 = (c_uint32 * N)(), (c_uint32 * N)()
        buf = (c_ubyte * NB)(*(data or bytes(NB)))
        r = self.lib.w32h_call(tag.encode(), fn.encode(), arr(a), arr(b), o0, o1, k, buf)
        assert r > -1000, "%s %s: not dispatched (%d)" % (tag, fn, r)
        return r, list(o0), list(o1), bytes(buf)

    def facts(self, tag):
        out = (c_int * 7)()
        assert self.lib.w32h_facts(tag.encode(), out) == 0
        return list(out)


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("w32gh"))
    for tag in TAGS:
        with open(os.path.join(tmp, "params_%s_w32.h" % tag), "w") as f:
            f.write(emit.header_text(gi.params(tag), generated=True))
    with open(os.path.join(tmp, "fields.inc"), "w") as f:
        f.write("".join('#include "params_%s_w32.h"\n' % t for t in TAGS) + "#define W32G_FIELDS(X) " + " ".join("X(%s)" % t for t in TAGS) + "\n")
    cc = HIPCC if os.path.exists(HIPCC) else shutil.which("hipcc")
    assert cc, "hipcc not found: the host check compiles csrc/field.h with it (a missing compiler is a broken build, not a reason to skip)"
    csrc = os.path.join(ROOT, "modarith_amd", "csrc")
    so = os.path.join(tmp, "libfield_w32_gen_host.so")
    cmd = [cc, "-O1", "-std=c++17", "-w", "-shared", "-fPIC", "--offload-host-only", "-I", os.path.join(csrc, "generated"), "-I", csrc, "-I", tmp,
           '-DW32G_LIST="fields.inc"', os.path.join(ROOT, "tools", "field_w32_gen_host.hip"), "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-4000:]
    return Host(so)


def run_record(host, T, fn, row, pool):
    """run one fixture record; -> list of (got, expected) pairs (the layouts of tests/golden/make_golden_w32.py)"""
    U, M32 = gi.unpack, gi.M32
    if fn in ("modadd", "modsub", "modmul"):
        return [(host.call(T, fn, pool[row[0]], pool[row[1]])[1], U(row[2]))]
    if fn in ("modneg", "modsqr", "modcpy", "nres", "redc", "modhaf"):
        return [(host.call(T, fn, pool[row[0]])[1], U(row[1]))]
    if fn in ("prop", "flatten", "modfsb"):
        r, o, _, _ = host.call(T, fn, pool[row[0]])
        return [(o, U(row[1])), (r & M32, row[2])]
    if fn in ("modnsqr", "modmli"):
        return [(host.call(T, fn, pool[row[0]], k=row[1])[1], U(row[2]))]
    if fn in ("modis1", "modis0", "modsign"):
        return [(host.call(T, fn, pool[row[0]])[0], row[1])]
    if fn == "modcmp":
        return [(host.call(T, fn, pool[row[0]], pool[row[1]])[0], row[2])]
    if fn in ("modzer", "modone"):
        return [(host.call(T, fn)[1], U(row[0]))]
    if fn in ("modint", "mod2r"):
        return [(host.call(T, fn, k=row[0])[1], U(row[1]))]
    if fn == "modcmv":
        return [(host.call(T, fn, pool[row[1]], pool[row[2]], k=row[0])[1], U(row[3]))]
    if fn == "modcsw":
        _, g, f, _ = host.call(T, fn, pool[row[1]], pool[row[2]], k=row[0])
        return [(g, U(row[3])), (f, U(row[4]))]
    if fn == "modshl":
        return [(host.call(T, fn, pool[row[1]], k=row[0])[1], U(row[2]))]
    if fn == "modshr":
        r, o, _, _ = host.call(T, fn, pool[row[1]], k=row[0])
        return [(o, U(row[2])), (r, row[3])]
    if fn == "modexp":
        return [(host.call(T, fn, pool[row[0]])[3].hex(), row[1])]
    if fn == "modimp":
        r, o, _, _ = host.call(T, fn, data=bytes.fromhex(row[0]))
        return [(o, U(row[1])), (r, row[2])]
    raise AssertionError("no runner for " + fn)


def test_the_examples_are_one_per_class():
    shapes = {t: (gi.params(t).family, gi.params(t).nlimbs, gi.params(t).radix) for t in TAGS}
    assert shapes == {"2519": ("pseudo", 9, 28), "1305": ("pseudo", 5, 26), "BP256": ("monty", 9, 29), "NIST384": ("monty", 14, 28),
                      "GM240": ("monty", 9, 29), "PM512": ("pseudo", 18, 29), "Q25519": ("monty", 9, 29), "M2519": ("monty", 9, 29)}
    assert gi.params("BP256").ndash != 1 and gi.params("Q25519").ndash != 1 and min(gi.params("NIST384").ppw) < 0
    assert emit.w32_ept_max(18) == 2 and emit.w32_ept_max(16) == 4


@pytest.mark.parametrize("T", TAGS)
def test_fixture_is_the_shared_recipe_and_the_struct_is_the_fields(host, T):
    fx, fp = gio.load("field_w32gen_%s.json" % T), gi.params(T)
    assert fx["wordlength"] == 32 and fx["tag"] == T and int(fx["params"]["p"], 16) == fp.p
    assert [gi.unpack(s) for s in fx["pool"]] == gi.pool(fp, fx["pool_extra"])
    pool, top = gi.pool(fp, fx["pool_extra"]), (1 << (fp.radix + 2)) - 1
    assert [top] * fp.nlimbs in pool and [gi.M32] * fp.nlimbs in pool
    for pos in range(fp.nlimbs):
        assert any(a[pos] == top and sum(v == top for v in a) == 1 for a in pool), "budget edge at limb %d" % pos
    assert host.facts(T) == [fp.nlimbs, fp.radix, fp.n, fp.nbytes, int(fp.montgomery), 4, int(w32_inv_closure(fp)["closed"])]
    assert os.path.getsize(gio.path_of("field_w32gen_%s.json" % T)) < 175 * 1024


@pytest.mark.parametrize("T", TAGS)
def test_every_record_of_the_28_emitted_functions(host, T):
    fx = gio.load("field_w32gen_%s.json" % T)
    pool = [gi.unpack(s) for s in fx["pool"]]
    assert sorted(fx["records"]) == sorted(EMITTED)
    compared, bad = 0, []
    for fn in EMITTED:
        for k, row in enumerate(fx["records"][fn]):
            for got, want in run_record(host, T, fn, row, pool):
                if got != want:
                    bad.append((fn, k, row[:3], got, want))
            compared += 1
    assert not bad, "%d records differ, first: %r" % (len(bad), bad[:3])
    assert compared == fx["count"] == sum(len(v) for v in fx["records"].values()) and compared > 3000


@pytest.mark.parametrize("T", TAGS)
def test_chain_functions_by_value(host, T):
    """modpro modinv modsqrt modqr on the in-contract part of the pool (below 2p in digit form: where the reference's arithmetic HAS
    a value, tests/test_w32_host.py): x * inv == 1, sqrt^2 == x where modqr says so, modqr against Euler's criterion, modpro against
    x^PE; values after redc"""
    fp = gi.params(T)
    p = fp.p
    Rinv = pow(fp.R, -1, p) if fp.montgomery else 1
    fx = gio.load("field_w32gen_%s.json" % T)
    val = lambda limbs: gi.value(fp, host.call(T, "redc", limbs)[1])
    done = skipped = 0
    for i, s in enumerate(fx["pool"]):
        a = gi.unpack(s)
        if not gi.in_contract(fp, a):
            skipped += 1
            continue
        x = gi.value(fp, a) * Rinv % p
        inv = val(host.call(T, "modinv", a)[1])
        assert inv * x % p == (1 if x else 0), (T, i)
        qr = host.call(T, "modqr", a)[0]
        assert qr == (1 if x == 0 or pow(x, (p - 1) // 2, p) == 1 else 0), (T, i)
        h = host.call(T, "modpro", a)[1]
        assert val(h) == pow(x, fp.pe, p), (T, i)
        if qr:
            rt = val(host.call(T, "modsqrt", a)[1])
            assert rt * rt % p == x, (T, i)
            assert val(host.call(T, "modsqrt", a, h)[1]) == rt
        assert val(host.call(T, "modinv", a, h)[1]) == inv and host.call(T, "modqr", a, h)[0] == qr
        done += 1
    assert done + skipped == len(fx["pool"]) and done >= 25 + 2 * fx["pool_extra"]


@pytest.mark.parametrize("T", TAGS)
def test_products_at_the_edge_of_the_inversion_contract(host, T):
    """where the driver claims closure (INV_CLOSED): products of elements at the edge of what w32_inv_in_contract admits -- every
    limb at 2^Radix - 1, the top limb at 2^TOPB - 1, and random admitted elements -- and products of those products stay congruent,
    below 2p and admitted.  Where it does not (PM512: the bad_overflow form), the struct says so and nothing is claimed."""
    fp = gi.params(T)
    c = w32_inv_closure(fp)
    assert host.facts(T)[6] == int(c["closed"])
    if not c["closed"]:
        assert T == "PM512" and c["why"]
        return
    N, R, p = fp.nlimbs, fp.radix, fp.p
    topb = fp.n + 1 - R * (N - 1)
    assert c["topb"] == topb and c["column"] < 1 << 64
    edge = [(1 << R) - 1] * (N - 1) + [(1 << topb) - 1]
    rng = random.Random(77)
    elems = [edge, edge[:-1] + [0], [0] * (N - 1) + [edge[-1]]] + [[rng.randrange(0, 1 << R) for _ in range(N - 1)] + [rng.randrange(0, 1 << topb)] for _ in range(12)]
    assert all(w32_inv_in_contract(fp, e) for e in elems) and not w32_inv_in_contract(fp, edge[:-1] + [1 << topb])
    Rinv = pow(fp.R, -1, p) if fp.montgomery else 1
    slack_limb = 2 if fp.carry_on else 1
    for a in elems:
        for b in elems[:5]:
            z = host.call(T, "modmul", a, b)[1]
            assert gi.value(fp, z) % p == gi.value(fp, a) * gi.value(fp, b) * Rinv % p and gi.value(fp, z) < 2 * p
            assert all(v < (1 << R) + (c["slack"] if i == slack_limb else 0) for i, v in enumerate(z[:-1])) and z[-1] < 1 << topb
            zz = host.call(T, "modmul", z, z)[1]                            # a product of products (the prefix chain)
            assert gi.value(fp, zz) % p == gi.value(fp, z) ** 2 * Rinv % p and gi.value(fp, zz) < 2 * p
            s = host.call(T, "modsqr", z)[1]
            assert s == zz
            assert host.call(T, "modis0", z)[0] == (1 if gi.value(fp, z) % p == 0 else 0)
