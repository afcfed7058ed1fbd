"""What the launchers shared by both word lengths (csrc/capi_field.inc) decide, pinned through the C ABI: which kernel path a call
takes -- modarith_amd_last_launch() after it -- and that the body of a batch (several elements per lane) and its tail (one element per
lane at its own address) return the words of the same elements run one at a time.  X25519, NIST256 and X448 at 64 and 32 bits.  The
rows that set an environment knob run in a fresh child process: MA_FORCE_EXACT and MA_INV_SIMUL are read once per process."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
PRIMES = ("X25519", "NIST256", "X448")
FORMS = [(P, wl) for P in PRIMES for wl in (64, 32)]
SHARE_MIN = 32768               # modinv shares inversions from this batch size on (csrc/capi_field.inc INV_SIMUL_MIN)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Form:
    """one prime at one word length: its entry points and flat batches of its limbs"""

    def __init__(self, P, wl):
        import ctypes
        import torch
        from modarith_amd import _lib
        assert torch.cuda.is_available(), "these tests need the MI355X"
        self.torch, self.lib, self.P, self.wl = torch, _lib.load(), P, wl
        self.sfx = "" if wl == 64 else "(w32)"
        self.dtype, self.bytes = (torch.int64, 8) if wl == 64 else (torch.int32, 4)
        out = [ctypes.c_int() for _ in range(5)]
        info = self.lib.modarith_amd_field_info if wl == 64 else self.lib.modarith_amd_w32_field_info
        assert info(P.encode(), *[ctypes.byref(v) for v in out]) == 1
        self.N, self.montgomery = out[0].value, bool(out[4].value)
        self.st = torch.cuda.current_stream().cuda_stream

    def name(self, how=None):
        """the launch name of modinv taken the way `how`"""
        if how is None:
            return "modinv" + self.sfx
        return "modinv(%s)" % how if self.wl == 64 else "modinv(w32, %s)" % how

    def call(self, fn, *args):
        f = getattr(self.lib, "%s_%s%s_batch" % (fn, self.P, "" if self.wl == 64 else "_w32"))
        assert f(*args, self.st) == 0, (fn, self.lib.modarith_amd_last_error())
        return self.lib.modarith_amd_last_launch().decode()

    def empty(self, ld):
        return self.torch.zeros((self.N, ld), dtype=self.dtype, device="cuda")

    def uniform(self, n, ld, array):
        x = self.empty(ld)
        self.call("moduniform", 11, array, 0, 0, x.data_ptr(), n, ld)
        return x


def launch_names(P, wl, knob=None):
    """[(call, launch name reported, launch name expected)] for the rows of `knob` (None: no knob set)"""
    F = Form(P, wl)
    rows = []
    big = F.uniform(SHARE_MIN, SHARE_MIN, 1)
    zb = F.empty(SHARE_MIN)
    inv = lambda src, dst, n: F.call("modinv", src.data_ptr(), None, dst.data_ptr(), n, SHARE_MIN)
    if knob == "MA_INV_SIMUL":
        return [("modinv, %d elements, MA_INV_SIMUL=0" % SHARE_MIN, inv(big, zb, SHARE_MIN), F.name())]
    a, b, c = F.uniform(5, 8, 2), F.uniform(5, 8, 3), F.empty(8)
    binary = lambda fn: F.call(fn, a.data_ptr(), b.data_ptr(), c.data_ptr(), 5, 8)
    unary = lambda fn: F.call(fn, a.data_ptr(), c.data_ptr(), 5, 8)
    if knob == "MA_FORCE_EXACT":
        assert wl == 64
        return [("modmul, MA_FORCE_EXACT=1", binary("modmul"), "modmul(exact)"),
                ("modinv, %d elements, MA_FORCE_EXACT=1" % SHARE_MIN, inv(big, zb, SHARE_MIN), "modinv(exact)")]
    assert knob is None
    rows += [("modadd", binary("modadd"), "modadd" + F.sfx), ("modmul", binary("modmul"), "modmul" + F.sfx)]
    if wl == 64:
        exact = "" if F.montgomery else "(exact)"       # (nres / redc of a pseudo-Mersenne prime multiply nothing: no policy to vote on)
        rows += [("modsqr", unary("modsqr"), "modsqr"), ("nres", unary("nres"), "nres" + exact), ("redc", unary("redc"), "redc" + exact),
                 ("modpro", unary("modpro"), "modpro")]
    else:
        rows += [("nres", unary("nres"), "nres(w32)"), ("redc", unary("redc"), "redc(w32)")]
    rows.append(("modinv", F.call("modinv", a.data_ptr(), None, c.data_ptr(), 5, 8), F.name()))
    h = F.empty(8)
    F.call("modpro", a.data_ptr(), h.data_ptr(), 5, 8)
    rows.append(("modinv with progenitors", F.call("modinv", a.data_ptr(), h.data_ptr(), c.data_ptr(), 5, 8), F.name("h")))
    rows.append(("modinv, %d elements, output != input" % SHARE_MIN, inv(big, zb, SHARE_MIN), F.name("simultaneous")))
    y = big.clone()
    rows.append(("modinv, %d elements, in place" % SHARE_MIN, inv(y, y, SHARE_MIN), F.name("simultaneous, in place")))
    assert F.torch.equal(y, zb)
    rows.append(("modinv, %d elements" % (SHARE_MIN - 1), inv(big, zb, SHARE_MIN - 1), F.name()))
    F.torch.cuda.synchronize()
    return rows


def body_plus_tail(P, wl):
    """modmul and modmli on n = 1, 2, 3, 5, 7 elements -- n - 1 of moduniform and one of all-ones limbs, which no product contract
    admits: at 64 bits its wave runs the exact products in the voted body, next to the tail kernel that always does -- in rows that
    start on 16 bytes and in rows of an odd limb stride: the words of the same elements run one at a time (n = 1).
    Returns the number of batches compared."""
    F = Form(P, wl)
    torch = F.torch
    done = 0
    for ld in (8, 9):                                   # 8: every row 16-byte aligned (the widest access); 9: odd stride, one element per lane
        for n in (1, 2, 3, 5, 7):
            a, b = F.uniform(n, ld, 4), F.uniform(n, ld, 5)
            a[:, n // 2] = -1
            for fn in ("modmul", "modmli"):
                got, want = F.empty(ld), F.empty(ld)
                if fn == "modmul":
                    F.call(fn, a.data_ptr(), b.data_ptr(), got.data_ptr(), n, ld)
                else:
                    F.call(fn, a.data_ptr(), 77, got.data_ptr(), n, ld)
                for j in range(n):
                    o = j * F.bytes
                    if fn == "modmul":
                        F.call(fn, a.data_ptr() + o, b.data_ptr() + o, want.data_ptr() + o, 1, ld)
                    else:
                        F.call(fn, a.data_ptr() + o, 77, want.data_ptr() + o, 1, ld)
                assert torch.equal(got, want), (P, wl, fn, n, ld, got.tolist(), want.tolist())
                assert bool((got[:, :n] != 0).any()) and not bool((got[:, n:] != 0).any())      # something was written, and nothing beyond n
                done += 1
    return done


def child(what, knob):
    """entry of the child processes: `what` over every form the knob touches; prints one line per check"""
    if what == "names":
        for P, wl in FORMS:
            if knob == "MA_FORCE_EXACT" and wl == 32:
                continue                                # (the 32-bit form has one product policy and does not read the knob)
            for call, got, want in launch_names(P, wl, knob):
                assert got == want, (P, wl, call, got, want)
                print("NAME", P, wl, call, got)
    else:
        for P in PRIMES:
            print("TAIL", P, body_plus_tail(P, 32))


def _run_child(what, knob, value):
    code = "from tests.test_gpu_launch_paths import child\nchild(%r, %r)\nprint('DONE')\n" % (what, knob)
    p = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT, **{knob: value}), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and p.stdout.endswith("DONE\n"), p.stdout[-2000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("P,wl", FORMS)
def test_launch_names(P, wl):
    rows = launch_names(P, wl)
    assert len(rows) == (11 if wl == 64 else 9)
    for call, got, want in rows:
        assert got == want, (P, wl, call, got, want)


@pytest.mark.parametrize("knob,value,lines", [("MA_INV_SIMUL", "0", 6), ("MA_FORCE_EXACT", "1", 6)])
def test_launch_names_under_a_knob(knob, value, lines):
    out = _run_child("names", knob, value)
    assert out.count("NAME ") == lines, out


@pytest.mark.parametrize("P,wl", FORMS)
def test_body_plus_tail(P, wl):
    assert body_plus_tail(P, wl) == 20


@pytest.mark.parametrize("ept", ["4", "2"])
def test_body_plus_tail_w32_at_wider_accesses(ept):
    """MA_W32_EPT raises the widest access of the 32-bit streaming kernels from one element per lane to two or four"""
    out = _run_child("tail", "MA_W32_EPT", ept)
    assert out.count("TAIL ") == 3 and all(line.endswith(" 20") for line in out.splitlines() if line.startswith("TAIL ")), out
