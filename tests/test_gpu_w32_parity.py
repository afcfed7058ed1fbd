"""The batched and scalar entry points of the 32-bit word form on the GPU against the reference's emitted C at word length 32.

Every record of tests/golden/field_w32_<PRIME>.json.xz (28 functions; tests/golden/make_golden_w32.py) goes through
Field(P, wl=32), word for word, in five layouts so that every access width of csrc/kernels32.h runs: flat rows with a stride that is
a multiple of four on 16-byte aligned buffers, views that start 8 and 4 bytes into such rows, an odd limb stride and tiles of 128,
each with the widest access it allows (MA_W32_EPT: 16, 8 and 4 bytes per lane) and with the library's default launch shape.  Then the
scalar _ct form on a sample of every function, and in / out aliasing."""
import ctypes
from ctypes import POINTER, c_char, c_int, c_uint, c_uint32

import pytest

from tests import w32_inputs as wi
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
# (layout, MA_W32_EPT): the widest per-lane access the library may take for the call (None: its measured default).  The library reads
# the knob at every call and narrows the access by itself where a buffer or a stride does not allow it, so flat16 / tiled at 4 run
# 16 bytes per lane (global_load_dwordx4) plus the tail, at 2 and on off8 8 bytes, off4 / oddld 4 bytes
LAYOUTS = (("flat16", "4"), ("flat16", "2"), ("flat16", None), ("off8", "4"), ("off4", "4"), ("oddld", "4"), ("tiled", "4"), ("tiled", "2"), ("tiled", None))


def _place(F, rows, layout):
    """a batch holding `rows` (limb lists) in the given layout, and the number of elements it holds (tiled: padded to whole tiles)"""
    import torch
    n = len(rows)
    if layout == "tiled":
        rows = list(rows)
        while len(rows) < 256 or len(rows) % 128:            # whole tiles, at least two (Field.creates_tiled)
            rows.append(rows[len(rows) % n])
        t = Ftile(F).from_limbs(rows)
        assert t.dim() == 3 and t.shape[2] == 128
        return t, n
    src = Fflat(F).from_limbs(rows)
    ld = (n + 3) // 4 * 4 + 8
    if layout == "oddld":
        ld += 1
    big = torch.zeros((F.N, ld), dtype=torch.int32, device=F.device)
    off = {"flat16": 0, "oddld": 0, "off8": 2, "off4": 1}[layout]
    view = big[:, off:off + n]
    view.copy_(src)
    assert view.data_ptr() % 16 == (4 * off) % 16
    return view, n


_fields = {}


def Fflat(F):
    from modarith_amd.field import Field
    return _fields.setdefault((F.prime, None), Field(F.prime, wl=32, tile=None))


def Ftile(F):
    from modarith_amd.field import Field
    return _fields.setdefault((F.prime, 128), Field(F.prime, wl=32, tile=128))


def _limbs(F, t, n):
    return F.to_limbs(t)[:n] if t.dim() == 3 else [[int(v) & wi.M32 for v in col] for col in t.detach().cpu().T.tolist()][:n]


def _ints(t, n):
    return [int(v) for v in t.tolist()][:n]


def run_function(F, fn, recs, pool, layout):
    """all records of one function as batches; returns the number of records compared"""
    import torch
    U = wi.unpack
    put = lambda rows: _place(F, rows, layout)
    dev = F.device

    def groups(key):
        out = {}
        for r in recs:
            out.setdefault(key(r), []).append(r)
        return out.items()

    if fn in ("modadd", "modsub", "modmul"):
        a, n = put([pool[r[0]] for r in recs]); b, _ = put([pool[r[1]] for r in recs])
        assert _limbs(F, getattr(F, fn)(a, b), n) == [U(r[2]) for r in recs], fn
    elif fn in ("modneg", "modsqr", "modcpy", "nres", "redc"):
        a, n = put([pool[r[0]] for r in recs])
        assert _limbs(F, getattr(F, fn)(a), n) == [U(r[1]) for r in recs], fn
    elif fn == "modhaf":
        a, n = put([pool[r[0]] for r in recs])
        assert _limbs(F, F.modhaf(a), n) == [U(r[1]) for r in recs]
    elif fn in ("prop", "flatten", "modfsb"):
        a, n = put([pool[r[0]] for r in recs])
        flag = getattr(F, fn)(a)
        assert _limbs(F, a, n) == [U(r[1]) for r in recs], fn
        assert [v & wi.M32 for v in _ints(flag, n)] == [r[2] for r in recs], fn
    elif fn in ("modnsqr", "modmli"):
        for k, rs in groups(lambda r: r[1]):
            a, n = put([pool[r[0]] for r in rs])
            got = F.modnsqr(a, k) if fn == "modnsqr" else F.modmli(a, k)
            assert _limbs(F, got, n) == [U(r[2]) for r in rs], (fn, k)
    elif fn in ("modis1", "modis0", "modsign"):
        a, n = put([pool[r[0]] for r in recs])
        assert _ints(getattr(F, fn)(a), n) == [r[1] for r in recs], fn
    elif fn == "modcmp":
        a, n = put([pool[r[0]] for r in recs]); b, _ = put([pool[r[1]] for r in recs])
        assert _ints(F.modcmp(a, b), n) == [r[2] for r in recs]
    elif fn in ("modzer", "modone", "modint", "mod2r"):
        G = Ftile(F) if layout == "tiled" else Fflat(F)
        n = 256 if layout == "tiled" else {"flat16": 8, "off8": 6, "off4": 5, "oddld": 7}[layout]
        for r in recs:
            t = {"modzer": lambda: G.modzer(n), "modone": lambda: G.modone(n), "modint": lambda: G.modint(r[0], n), "mod2r": lambda: G.mod2r(r[0], n)}[fn]()
            assert _limbs(G, t, n) == [U(r[-1])] * n, (fn, r[0])
    elif fn in ("modcmv", "modcsw"):
        g, n = put([pool[r[1]] for r in recs]); f, _ = put([pool[r[2]] for r in recs])
        m = g.shape[0] * g.shape[2] if g.dim() == 3 else n
        d = torch.tensor([r[0] for r in recs] + [0] * (m - n), dtype=torch.int32, device=dev)
        if fn == "modcmv":
            F.modcmv(d, g, f)
            assert _limbs(F, f, n) == [U(r[3]) for r in recs]
            assert _limbs(F, g, n) == [pool[r[1]] for r in recs]
        else:
            F.modcsw(d, g, f)
            assert _limbs(F, g, n) == [U(r[3]) for r in recs] and _limbs(F, f, n) == [U(r[4]) for r in recs]
    elif fn in ("modshl", "modshr"):
        for k, rs in groups(lambda r: r[0]):
            a, n = put([pool[r[1]] for r in rs])
            if fn == "modshl":
                F.modshl(k, a)
            else:
                assert _ints(F.modshr(k, a), n) == [r[3] for r in rs], k
            assert _limbs(F, a, n) == [U(r[2]) for r in rs], (fn, k)
    elif fn == "modexp":
        a, n = put([pool[r[0]] for r in recs])
        got = F.modexp(a).cpu().numpy()
        assert [bytes(got[j]).hex() for j in range(n)] == [r[1] for r in recs]
    elif fn == "modimp":
        G = Ftile(F) if layout == "tiled" else Fflat(F)
        rows = [bytes.fromhex(r[0]) for r in recs]
        n = len(rows)
        if layout == "tiled":
            rows = (rows * (256 // n + 1))[:256]
        b = torch.tensor([list(x) for x in rows], dtype=torch.uint8, device=dev)
        a, flag = G.modimp(b)
        assert _limbs(G, a, n) == [U(r[1]) for r in recs] and _ints(flag, n) == [r[2] for r in recs]
    else:
        raise AssertionError("no runner for " + fn)
    return len(recs)


@pytest.mark.parametrize("layout,ept", LAYOUTS)
@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_every_record_through_the_batched_entry_points(P, layout, ept, monkeypatch):
    from modarith_amd.field import Field
    if ept is None:
        monkeypatch.delenv("MA_W32_EPT", raising=False)
    else:
        monkeypatch.setenv("MA_W32_EPT", ept)
    fx = load_golden("field_w32_%s.json" % P)
    pool = [wi.unpack(s) for s in fx["pool"]]
    F = Field(P, wl=32, tile=None)
    assert (F.N, F.radix, F.nbytes) == wi.SHAPES[P][:2] + (wi.SHAPES[P][3],)
    compared = sum(run_function(F, fn, recs, pool, layout) for fn, recs in fx["records"].items())
    assert compared == fx["count"] and len(fx["records"]) == 28


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_chain_functions_by_value_and_modlimbs(P):
    """modpro modinv modsqrt modqr on the in-contract part of the pool (tests/test_w32_host.py says why that part), by value; modinv is the
    normalised inverse nres(redc(1/x)); modlimbs on the whole pool"""
    from modarith_amd.field import Field
    from modarith_amd.params import derive
    fp = derive(P, wl=32)
    N, R, _, _, p = wi.SHAPES[P]
    fx = load_golden("field_w32_%s.json" % P)
    pool = [wi.unpack(s) for s in fx["pool"]]
    F = Field(P, wl=32, tile=None)
    assert F.modlimbs(F.from_limbs(pool)).tolist() == [int(max(a) < 1 << (R + 2)) for a in pool]
    rows = [a for a in pool if wi.value(P, a) < 2 * p and not max(a[:-1]) >> R]
    Rinv = pow(fp.R, -1, p) if fp.montgomery else 1
    xs = [wi.value(P, a) * Rinv % p for a in rows]
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
    assert val(F.modsqrt(a, h)) == rt


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_aliasing_conversions_and_refusals(P):
    import torch
    from modarith_amd.field import Field
    fx = load_golden("field_w32_%s.json" % P)
    pool = [wi.unpack(s) for s in fx["pool"]]
    F = Field(P, wl=32, tile=None)
    a = F.from_limbs(pool)
    want_mul = F.to_limbs(F.modmul(a, a))
    want_sqr = F.to_limbs(F.modsqr(a))
    recs = {r[0]: wi.unpack(r[1]) for r in fx["records"]["modsqr"]}
    assert want_sqr == [recs[i] for i in range(len(pool))]
    for i, j, out in fx["records"]["modmul"]:
        if i == j:
            assert want_mul[i] == wi.unpack(out)
    b = a.clone(); F.modmul(b, b, out=b); assert F.to_limbs(b) == want_mul          # modmul(a, a, a)
    b = a.clone(); F.modsqr(b, out=b); assert F.to_limbs(b) == want_sqr            # modsqr(a, a)
    b = a.clone(); F.modadd(b, b, out=b); assert F.to_limbs(b) == F.to_limbs(F.modadd(a, a))
    # AoS <-> SoA, tiled <-> flat, integers
    import numpy as np
    aos = torch.from_numpy(np.array(pool, dtype=np.uint32).view(np.int32)).to(F.device)
    assert F.to_limbs(F.from_aos(aos)) == pool and torch.equal(F.to_aos(a), aos)
    G = Field(P, wl=32, tile=128)
    rows = (pool * 4)[:256]
    t = G.from_limbs(rows)
    assert t.dim() == 3 and t.dtype == torch.int32 and G.to_limbs(t) == rows and torch.equal(G.to_tiled(G.to_flat(t), 128), t)
    assert torch.equal(G.to_flat(G.from_aos(G.to_aos(t))), G.to_flat(t))
    vals = [0, 1, F.params.p - 1, F.params.p, 2 * F.params.p - 1]
    assert F.to_ints(F.from_ints(vals)) == vals
    for call in (lambda: F.modmuls(a, pool[0]), lambda: F.modadd_lazy(a, a), lambda: F.modsub_lazy(a, a), lambda: F.modneg_lazy(a), lambda: F.time_protocol("modmul", a)):
        with pytest.raises(NotImplementedError, match="word length 32"):
            call()
    with pytest.raises(ValueError):
        Field("NIST521", wl=32)
    with pytest.raises(ValueError):
        F.modmul(a.to(torch.int64), a.to(torch.int64))


def _ct(lib, P, fn):
    return getattr(lib, "%s_%s_w32_ct" % (fn, P))


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_scalar_form_on_a_sample_of_every_function(P):
    """the first, the middle and the last record of every function through <fn>_<P>_w32_ct (host pointers, one element through the GPU)"""
    from modarith_amd import _lib
    L = _lib.load()
    fx = load_golden("field_w32_%s.json" % P)
    pool = [wi.unpack(s) for s in fx["pool"]]
    N, _, _, NB, _ = wi.SHAPES[P]
    A = lambda v=None: (c_uint32 * N)(*(v if v is not None else [7] * N))
    U = wi.unpack
    for fn in ("prop", "flatten", "modfsb"):
        _ct(L, P, fn).restype = c_uint32
    done = 0
    for fn, recs in fx["records"].items():
        f = _ct(L, P, fn)
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
    # the four chain functions: by value on one in-contract element
    p = wi.SHAPES[P][4]
    from modarith_amd.params import derive
    fp = derive(P, wl=32)
    x = A(); _ct(L, P, "nres")(A(wi.split(P, 1234567)), x)
    h, z, c = A(), A(), A()
    _ct(L, P, "modpro")(x, h)
    _ct(L, P, "modinv")(x, h, z)
    _ct(L, P, "redc")(z, c)
    assert wi.value(P, list(c)) == pow(1234567, -1, p)
    _ct(L, P, "modinv")(x, None, c)
    assert list(c) == list(z)
    assert _ct(L, P, "modqr")(None, x) == _ct(L, P, "modqr")(h, x) == (1 if pow(1234567, (p - 1) // 2, p) == 1 else 0)
    sq = A(); _ct(L, P, "modsqr")(x, sq)
    rt = A(); _ct(L, P, "modsqrt")(sq, None, rt)
    _ct(L, P, "modsqr")(rt, rt); _ct(L, P, "redc")(rt, c)
    assert wi.value(P, list(c)) == 1234567 ** 2 % p and fp.wl == 32
    assert L.modarith_amd_status() == 0
