"""Generated fields of the 32-bit word form on the GPU (modarith_amd.generate.generate_w32 -> Field(tag, wl=32)).

Every record of tests/golden/field_w32gen_<TAG>.json.xz -- what the reference's `pseudo.py 32` / `monty.py 32` emit for the eight
examples of modarith_amd.generate.EXAMPLES_W32, 28 functions -- goes through the batched entry points of the example's plug-in, word
for word, on flat rows and on tiles; the streaming functions again on n = 4096 + 3 elements (the records cycled) at MA_W32_EPT = 1,
2 and 4, so that body and tail run at every width the unit allows; a sample of every function through the _ct form.  Then: 2^255 - 19
generated under a tag of its own against the built-in X25519 entry points; the shared inversion against one inversion per element,
where the driver shows closure and where it does not; a fused chain; values against the 64-bit field of the same prime and Python
integers; a C consumer over the emitted shim."""
import ctypes
import os
import subprocess
import sys
from ctypes import c_char, c_int, c_uint, c_uint32

import pytest

from tests import w32_gen_inputs as gi
from tests import w32_inputs as wi
from tests.conftest import load_golden
from tests.test_gpu_w32_parity import run_function
from tests.w32_gen_inv_child import N_INV, inv_batch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXAMPLES = gi.examples()
TAGS = [t for t, _, _ in EXAMPLES]
N_STREAM = 4096 + 3


@pytest.fixture(scope="module")
def fields():
    """tag -> Field(tag, wl=32, tile=None); the plug-ins are build()'s (reused when current, generated here otherwise)"""
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from modarith_amd import generate as gen
    from modarith_amd.field import Field
    out = {}
    for tag, arg, fam in EXAMPLES:
        assert gen.generate_w32(arg, family=fam).tag == tag
        out[tag] = Field(tag, wl=32, tile=None)
    return out


def _launch():
    from modarith_amd import _lib
    return _lib.load().modarith_amd_last_launch().decode()


@pytest.mark.parametrize("layout", ("flat16", "tiled"))
@pytest.mark.parametrize("T", TAGS)
def test_every_record_through_the_batched_entry_points(fields, T, layout, monkeypatch):
    monkeypatch.delenv("MA_W32_EPT", raising=False)
    fx = load_golden("field_w32gen_%s.json" % T)
    pool = [gi.unpack(s) for s in fx["pool"]]
    F, fp = fields[T], gi.params(T)
    assert (F.N, F.radix, F.nbytes, F.params.p, F.wl) == (fp.nlimbs, fp.radix, fp.nbytes, fp.p, 32)
    compared = sum(run_function(F, fn, recs, pool, layout) for fn, recs in fx["records"].items())
    assert compared == fx["count"] and len(fx["records"]) == 28


def _flat_view(F, rows):
    """the rows as a view of n columns in a fresh buffer whose row stride is a multiple of four: 16-byte aligned rows, so the widest
    access the unit allows is taken (a contiguous [N, 4099] batch has an odd stride and runs one element per lane whatever is asked)"""
    import torch
    n = len(rows)
    ld = (n + 3) // 4 * 4 + 8
    big = torch.zeros((F.N, ld), dtype=torch.int32, device=F.device)
    view = big[:, :n]
    view.copy_(F.from_limbs(rows))
    return view


def _width(n, ld, ept, emax, *tensors):
    """elements per lane the library takes for this call: the rule of csrc/capi_field.inc pick_ept under the unit's cap"""
    for e in (4, 2):
        if e <= min(ept, emax) and n >= e and ld % e == 0 and all(t.data_ptr() % (4 * e) == 0 for t in tensors):
            return e
    return 1


@pytest.mark.parametrize("ept", (1, 2, 4))
@pytest.mark.parametrize("T", TAGS)
def test_streaming_functions_body_and_tail_at_every_width(fields, T, ept, monkeypatch):
    """n = 4096 + 3, the records cycled, on operands that allow every width: flat rows at a stride that is a multiple of four, and 33
    tiles of 128 of which the call is given the first n elements.  At width 4 the body takes 4096 elements and the tail kernel 3, at
    width 2 the tail takes one.  A unit whose limb count caps the width (PM512: two) clamps the request: asked for four it must run
    two -- it compiles no four-element kernel, so an unclamped pick would leave the body uncomputed.  The width each call takes
    follows from its layout by the library's rule and is asserted, so the test cannot quietly run one element per lane."""
    import torch
    from modarith_amd import emit
    from modarith_amd.field import Field, _stream
    monkeypatch.setenv("MA_W32_EPT", str(ept))
    fx = load_golden("field_w32gen_%s.json" % T)
    pool = [gi.unpack(s) for s in fx["pool"]]
    F, U = fields[T], gi.unpack
    G = Field(T, wl=32, tile=128)
    emax = emit.w32_ept_max(F.N)
    expect = min(ept, emax)
    assert emax == (2 if T == "PM512" else 4) and N_STREAM % 4 == 3
    n, SENT = N_STREAM, 0x5A5A5A5
    cyc = lambda rows: [rows[k % len(rows)] for k in range(n)]
    pad = lambda rows: rows + rows[:4224 - n]                                   # 33 whole tiles of 128
    rec = fx["records"]
    taken = set()

    def flat(fn, ins, want, k=None):
        vs = [_flat_view(F, r) for r in ins]
        out = getattr(F, fn)(*vs) if k is None else F.modmli(vs[0], k)
        assert out.stride(0) == vs[0].stride(0) and out.stride(0) % 4 == 0 and out.stride(0) > n
        w = _width(n, out.stride(0), ept, emax, out, *vs)
        assert w == expect, (fn, w)
        taken.add((w, n - n // w * w))
        assert F.to_limbs(out) == want, fn

    def tiles(fn, ins, want, k=None):
        """the batched entry point itself on whole tiles with n < 33 * 128: body, tail inside the last tile, nothing written past n"""
        ts = [G.from_limbs(pad(r)) for r in ins]
        out = torch.full_like(ts[0], SENT)
        assert ts[0].dim() == 3 and ts[0].shape == (33, F.N, 128)
        assert _width(n, 128, ept, emax, out, *ts) == expect
        args = [t.data_ptr() for t in ts] + ([k] if k is not None else []) + [out.data_ptr(), n, 128, _stream(G.device)]
        G._call(fn, *args)
        got = G.to_limbs(out)
        assert got[:n] == want, fn
        assert got[n:] == [[SENT] * F.N] * (4224 - n), fn

    for fn in ("modmul", "modadd", "modsub"):
        rs = cyc(rec[fn])
        a, b, want = [pool[r[0]] for r in rs], [pool[r[1]] for r in rs], [U(r[2]) for r in rs]
        flat(fn, [a, b], want)
        tiles(fn, [a, b], want)
    for fn in ("modsqr", "modneg", "modcpy", "nres", "redc"):
        rs = cyc(rec[fn])
        a, want = [pool[r[0]] for r in rs], [U(r[1]) for r in rs]
        flat(fn, [a], want)
        tiles(fn, [a], want)
    for k in (19, 121665, -1):
        rs = cyc([r for r in rec["modmli"] if r[1] == k])
        a, want = [pool[r[0]] for r in rs], [U(r[2]) for r in rs]
        flat("modmli", [a], want, k)
        tiles("modmli", [a], want, k)
    assert taken == {(expect, {1: 0, 2: 1, 4: 3}[expect])}                     # (width, elements left to the tail kernel)
    # a contiguous batch of an odd number of elements has an odd stride: one element per lane, the same words
    rs = cyc(rec["modmul"])
    a, b = F.from_limbs([pool[r[0]] for r in rs]), F.from_limbs([pool[r[1]] for r in rs])
    assert a.stride(0) == n and _width(n, n, ept, emax, a, b) == 1
    assert F.to_limbs(F.modmul(a, b)) == [U(r[2]) for r in rs]
    rs = cyc(rec["modcmv"])
    d = torch.tensor([r[0] for r in rs], dtype=torch.int32, device=F.device)
    f = F.from_limbs([pool[r[2]] for r in rs])
    F.modcmv(d, F.from_limbs([pool[r[1]] for r in rs]), f)
    assert F.to_limbs(f) == [U(r[3]) for r in rs]


@pytest.mark.parametrize("T", TAGS)
def test_scalar_form_on_a_sample_of_every_function(fields, T):
    """the first, the middle and the last record of every function through <fn>_<TAG>_w32_ct of the plug-in (host pointers), and the
    four chain functions by value"""
    from modarith_amd import _lib
    L = _lib.load_plugin(T, wl=32)
    ct = lambda fn: getattr(L, "%s_%s_w32_ct" % (fn, T))
    fx = load_golden("field_w32gen_%s.json" % T)
    pool = [gi.unpack(s) for s in fx["pool"]]
    fp = gi.params(T)
    N, NB, p = fp.nlimbs, fp.nbytes, fp.p
    A = lambda v=None: (c_uint32 * N)(*(v if v is not None else [7] * N))
    U = gi.unpack
    for fn in ("prop", "flatten", "modfsb"):
        ct(fn).restype = c_uint32
    done = 0
    for fn, recs in fx["records"].items():
        f = ct(fn)
        for r in (recs[0], recs[len(recs) // 2], recs[-1]):
            if fn in ("modadd", "modsub", "modmul"):
                z = A(); f(A(pool[r[0]]), A(pool[r[1]]), z); assert list(z) == U(r[2]), fn
            elif fn in ("modneg", "modsqr", "modcpy", "nres", "redc"):
                z = A(); f(A(pool[r[0]]), z); assert list(z) == U(r[1]), fn
            elif fn == "modhaf":
                z = A(pool[r[0]]); f(z); assert list(z) == U(r[1])
            elif fn in ("prop", "flatten", "modfsb"):
                z = A(pool[r[0]]); ret = f(z); assert list(z) == U(r[1]) and ret == r[2], fn
            elif fn == "modnsqr":
                z = A(pool[r[0]]); f(z, c_int(r[1])); assert list(z) == U(r[2])
            elif fn == "modmli":
                z = A(); f(A(pool[r[0]]), c_int(r[1]), z); assert list(z) == U(r[2])
            elif fn in ("modis1", "modis0", "modsign"):
                assert f(A(pool[r[0]])) == r[1], fn
            elif fn == "modcmp":
                assert f(A(pool[r[0]]), A(pool[r[1]])) == r[2]
            elif fn in ("modzer", "modone"):
                z = A(); f(z); assert list(z) == U(r[0]), fn
            elif fn == "modint":
                z = A(); f(c_int(r[0]), z); assert list(z) == U(r[1])
            elif fn == "mod2r":
                z = A(); f(c_uint(r[0]), z); assert list(z) == U(r[1])
            elif fn == "modcmv":
                g, t = A(pool[r[1]]), A(pool[r[2]]); f(c_int(r[0]), g, t); assert list(t) == U(r[3])
            elif fn == "modcsw":
                g, t = A(pool[r[1]]), A(pool[r[2]]); f(c_int(r[0]), g, t); assert list(g) == U(r[3]) and list(t) == U(r[4])
            elif fn == "modshl":
                z = A(pool[r[1]]); f(c_uint(r[0]), z); assert list(z) == U(r[2])
            elif fn == "modshr":
                z = A(pool[r[1]]); ret = f(c_uint(r[0]), z); assert list(z) == U(r[2]) and ret == r[3]
            elif fn == "modexp":
                out = (c_char * NB)(); f(A(pool[r[0]]), out); assert bytes(out).hex() == r[1]
            elif fn == "modimp":
                z = A(); ret = f((c_char * NB)(*bytes.fromhex(r[0])), z); assert list(z) == U(r[1]) and ret == r[2]
            else:
                raise AssertionError(fn)
            done += 1
    assert done == 3 * 28
    x = A(); ct("nres")(A(gi.split(fp, 1234567)), x)
    h, z, c = A(), A(), A()
    ct("modpro")(x, h)
    ct("modinv")(x, h, z)
    ct("redc")(z, c)
    assert gi.value(fp, list(c)) == pow(1234567, -1, p)
    ct("modinv")(x, None, c)
    assert list(c) == list(z)
    assert ct("modqr")(None, x) == ct("modqr")(h, x) == (1 if pow(1234567, (p - 1) // 2, p) == 1 else 0)
    sq = A(); ct("modsqr")(x, sq)
    rt = A(); ct("modsqrt")(sq, None, rt)
    ct("modsqr")(rt, rt); ct("redc")(rt, c)
    assert gi.value(fp, list(c)) == 1234567 ** 2 % p
    assert _lib.load().modarith_amd_status() == 0


@pytest.mark.parametrize("T", TAGS)
def test_chain_functions_by_value_and_refusals(fields, T):
    """modpro modinv modsqrt modqr on the in-contract part of the pool by value; modinv is the normalised inverse; the conversions,
    uniform and the W32_ABSENT refusals are the built-ins'"""
    import torch
    F, fp = fields[T], gi.params(T)
    p = fp.p
    fx = load_golden("field_w32gen_%s.json" % T)
    pool = [gi.unpack(s) for s in fx["pool"]]
    assert F.modlimbs(F.from_limbs(pool)).tolist() == [int(max(a) < 1 << (fp.radix + 2)) for a in pool]
    rows = [a for a in pool if gi.in_contract(fp, a)]
    Rinv = pow(fp.R, -1, p) if fp.montgomery else 1
    xs = [gi.value(fp, a) * Rinv % p for a in rows]
    a = F.from_limbs(rows)
    val = lambda t: F.to_ints(F.redc(t))
    inv = F.modinv(a)
    assert [i * x % p for i, x in zip(val(inv), xs)] == [1 if x else 0 for x in xs]
    assert F.to_limbs(inv) == F.to_limbs(F.nres(F.redc(inv)))
    h = F.modpro(a)
    assert val(h) == [pow(x, fp.pe, p) for x in xs]
    assert F.to_limbs(F.modinv(a, h)) == F.to_limbs(inv)
    qr = F.modqr(None, a).tolist()
    assert qr == [1 if x == 0 or pow(x, (p - 1) // 2, p) == 1 else 0 for x in xs] and F.modqr(h, a).tolist() == qr
    rt = val(F.modsqrt(a))
    assert all(r * r % p == x for r, x, q in zip(rt, xs, qr) if q) and sum(qr) > 10
    u = F.to_ints(F.uniform(257, seed=5))
    assert all(0 <= v < p for v in u) and len(set(u)) == 257
    assert torch.equal(F.to_flat(F.to_tiled(F.from_limbs((pool * 3)[:256]), 128)), F.from_limbs((pool * 3)[:256]))
    for call in (lambda: F.modmuls(a, pool[0]), lambda: F.modadd_lazy(a, a), lambda: F.modsub_lazy(a, a), lambda: F.modneg_lazy(a), lambda: F.time_protocol("modmul", a)):
        with pytest.raises(NotImplementedError, match="word length 32"):
            call()


def test_same_prime_two_tags(tmp_path, monkeypatch):
    """T25519 = 2^255 - 19 generated at word length 32 (on this box, in a scratch directory): the words of the built-in X25519 32-bit
    entry points on the whole pool of tests/w32_inputs.py, arbitrary words included"""
    import torch
    from modarith_amd import generate as gen
    from modarith_amd.field import Field
    monkeypatch.setattr(gen, "PLUGIN_DIR", str(tmp_path))
    F = Field.generate("T25519=2**255-19", wl=32)
    B = Field("X25519", wl=32, tile=None)
    assert F.prime == "T25519" and F.wl == 32 and (F.N, F.radix, F.nbytes) == (B.N, B.radix, B.nbytes) == (9, 29, 32)
    assert [m["tag"] for m in gen.installed(str(tmp_path), wl=32)] == ["T25519"] and gen.installed(str(tmp_path)) == []
    pool = wi.pool("X25519")
    pairs = wi.pairs("X25519", len(pool))
    a, b = B.from_limbs([pool[i] for i, _ in pairs]), B.from_limbs([pool[j] for _, j in pairs])
    for op in ("modmul", "modadd", "modsub"):
        assert torch.equal(getattr(F, op)(a, b), getattr(B, op)(a, b)), op
    for op in ("modsqr", "modneg", "nres", "redc", "modcpy", "modpro", "modinv", "modsqrt"):
        assert torch.equal(getattr(F, op)(a), getattr(B, op)(a)), op
    for k in (0, 19, 121665, -1):
        assert torch.equal(F.modmli(a, k), B.modmli(a, k)), k
    for op in ("modfsb", "flatten", "prop"):
        x, y = a.clone(), a.clone()
        assert torch.equal(getattr(F, op)(x), getattr(B, op)(y)) and torch.equal(x, y), op
    assert torch.equal(F.modqr(None, a), B.modqr(None, a)) and torch.equal(F.modexp(a), B.modexp(a))
    assert torch.equal(F.uniform(1000, seed=9), B.uniform(1000, seed=9))
    big = B.nres(B.uniform(N_INV, seed=3))
    assert torch.equal(F.modinv(big), B.modinv(big))


def _per_element_child(T, path):
    """modinv of the same batch in a fresh process with MA_INV_SIMUL=0 (the library reads that knob once per process): one inversion per
    element at every batch size.  tests/w32_gen_inv_child.py writes the words to `path`; returns the launch name the child saw"""
    env = dict(os.environ, MA_INV_SIMUL="0")
    r = subprocess.run([sys.executable, "-m", "tests.w32_gen_inv_child", T, path], capture_output=True, text=True, cwd=ROOT, env=env, timeout=300)
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-1500:]
    return r.stdout.strip().splitlines()[-1]


@pytest.mark.parametrize("T", ("BP256", "2519", "PM512"))
def test_shared_inversion_against_one_inversion_per_element(fields, T, monkeypatch, tmp_path):
    """the default path against MA_INV_SIMUL=0, word for word.  BP256 (Montgomery) and 2519 (pseudo-Mersenne): the driver shows
    closure, the batch shares inversions.  PM512: it does not, and the per-element kernel runs at every batch size, without a word"""
    import numpy as np
    import torch
    from modarith_amd.params import w32_inv_closure, w32_inv_in_contract
    F, fp = fields[T], gi.params(T)
    closed = w32_inv_closure(fp)["closed"]
    assert closed == (T != "PM512")
    x, special = inv_batch(torch, F, fp)
    keep = x.clone()
    monkeypatch.delenv("MA_INV_SIMUL", raising=False)
    got = F.modinv(x)
    assert _launch() == ("modinv(w32, simultaneous)" if closed else "modinv(w32)"), _launch()
    assert torch.equal(x, keep)
    path = str(tmp_path / "per_element.npy")
    assert _per_element_child(T, path) == "modinv(w32)"
    want = torch.from_numpy(np.load(path)).to(x.device)
    bad = (got != want).any(dim=0).nonzero().flatten().tolist()
    assert not bad, "%d elements differ, first at %r" % (len(bad), bad[:8])
    y = x.clone()
    F.modinv(y, out=y)                                                      # in place
    assert torch.equal(y, want)
    # values on a sample and on every special element that has one
    p = fp.p
    Rinv = pow(fp.R if fp.montgomery else 1, -1, p)
    sample = sorted(set(range(0, N_INV, 389)) | set(special))
    xl = [[int(v) & gi.M32 for v in col] for col in x[:, sample].T.tolist()]
    il = [[int(v) & gi.M32 for v in col] for col in got[:, sample].T.tolist()]
    zeros = ok = 0
    for q, a, b in zip(sample, xl, il):
        if q in special:
            assert a == special[q]
        if not w32_inv_in_contract(fp, a) or gi.value(fp, a) > 2 * p:
            continue                                          # no value to speak of: pinned word for word above
        v = gi.value(fp, a) * Rinv % p
        w = gi.value(fp, b) * Rinv % p
        if v == 0:
            assert b == [0] * fp.nlimbs
            zeros += 1
        else:
            assert v * w % p == 1, q
            ok += 1
    assert zeros >= 40 and ok >= 80


def test_fused_chain_on_a_generated_field(fields):
    """Chain("BP256", ..., wl=32) for ((x + y)(x - y))^2 against the four calls, n = 4096 + 3, flat and tiled"""
    import torch
    from modarith_amd.field import Field
    from modarith_amd.fuse import Chain
    F = fields["BP256"]
    ch = Chain("BP256", "w32gen", wl=32)
    u, v = ch.inputs(2)
    ch.output(ch.modsqr(ch.modmul(ch.modadd(u, v), ch.modsub(u, v))))
    f = ch.build()
    assert ch.symbol == "chain_w32gen_BP256_w32_batch"
    x, y = F.nres(F.uniform(N_STREAM, seed=1, array=1)), F.nres(F.uniform(N_STREAM, seed=1, array=2, plus_p=True))
    want = F.modsqr(F.modmul(F.modadd(x, y), F.modsub(x, y)))
    z, = f(x, y)
    assert torch.equal(z, want)
    G = Field("BP256", wl=32, tile=128)
    tx, ty = G.to_tiled(x[:, :4096].contiguous(), 128), G.to_tiled(y[:, :4096].contiguous(), 128)
    tz, = f(tx, ty)
    assert torch.equal(G.to_flat(tz), want[:, :4096])
    p = F.params.p
    assert F.to_ints(F.redc(z))[:64] == [((a + b) * (a - b)) ** 2 % p for a, b in zip(F.to_ints(F.redc(x))[:64], F.to_ints(F.redc(y))[:64])]


# the 64-bit field of the same prime: the plug-in of modarith_amd.generate.EXAMPLES where there is one, else the built-in prime
FIELD64 = {"2519": "2519", "1305": "1305", "BP256": "BP256", "M2519": "M2519", "NIST384": "NIST384", "GM240": "GM240", "PM512": "PM512", "Q25519": "ED25519Q"}


@pytest.mark.parametrize("T", TAGS)
def test_values_against_the_64_bit_field_and_python_integers(fields, T):
    """redc(modmul(nres a, nres b)) through Field(tag, wl=32) equals the same through the 64-bit field of that prime, and a * b mod p"""
    import random
    from modarith_amd.field import Field
    F = fields[T]
    F64 = Field(FIELD64[T], tile=None)
    p = F.params.p
    assert F64.params.p == p and F64.wl == 64
    rng = random.Random(41)
    n = 4096 + 3
    xs = [0, 1, p - 1, p, 2 * p - 1] + [rng.randrange(0, 2 * p) for _ in range(n - 5)]
    ys = [rng.randrange(0, 2 * p) for _ in range(n)]
    got = F.to_ints(F.redc(F.modmul(F.nres(F.from_ints(xs)), F.nres(F.from_ints(ys)))))
    got64 = F64.to_ints(F64.redc(F64.modmul(F64.nres(F64.from_ints(xs)), F64.nres(F64.from_ints(ys)))))
    assert got == got64
    assert got[:300] == [a * b % p for a, b in zip(xs[:300], ys[:300])]


def test_c_consumer_over_the_emitted_shim(fields, tmp_path):
    """examples/field_consumer_w32.c -- undecorated names and macros only -- compiled with gcc against field_BP256_w32.h, linked with
    the main library and the plug-in"""
    from modarith_amd import generate as gen
    fp = gi.params("BP256")
    d = gen.PLUGIN_DIR
    exe = str(tmp_path / "consumer_w32gen")
    lib = os.path.join(ROOT, "modarith_amd")
    cmd = ["gcc", "-O2", os.path.join(ROOT, "examples", "field_consumer_w32.c"), '-DFIELD_HEADER="field_BP256_w32.h"', "-I" + os.path.join(ROOT, "include"), "-I" + d,
           "-L" + lib, "-l:libmodarith_amd.so", "-L" + d, "-l:libmodarith_amd_BP256_w32.so", "-Wl,-rpath," + lib, "-Wl,-rpath," + d, "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-1000:]
    out = dict(l.split(" ", 1) for l in r.stdout.strip().splitlines())
    assert out["field"] == "Wordlength 32 Nlimbs 9 Radix 29 Nbits 256 Nbytes 32 sizeof(spint) 4"
    p, x, y = fp.p, 1234567, 7654321
    v = 39081 * pow((x * y) ** 2 + x - y, -1, p) % p
    assert out["value"] == "%064x" % v
    assert out["qr"] == str(1 if pow(v, (p - 1) // 2, p) == 1 else 0)
    assert out["import"] == "1 same 1" and out["zero"] == "1 one 0"

