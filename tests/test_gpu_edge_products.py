"""GPU parity at the edge of the limb budget, for EVERY built prime: the gfx950 objects of the FAST product forms (split at P::SPLIT,
column chain, half-limb forms: what every streaming kernel runs by default) and of the exact ones against the CPU oracle, limb for limb,
every element, on the inputs of tests/edge_inputs.py -- the same class in every limb of both operands (the all-maximal pair: the one
input the overflow proofs of emit.split_point / chain_ok / sparse_terms are about), the maximum in every limb but one, directed Montgomery
reduction digits, mixtures, uniform limbs below 2^(Radix+2).  The host build of the same arithmetic meets the same inputs in
tests/test_fast_products_host.py; the device build differs from it (SGPR-pinned constants, multiply-add forms of shifted terms).

Shapes: n = 2^14 + 3 (odd: scalar tail launch), flat rows, the tiled layout, an unaligned view.  One whole pair of waves (128 consecutive
elements: the kernels move two elements per lane) is all-maximal, one wave holds a single all-maximal lane among uniform ones, and the tail
is all-maximal: the policy vote is per wave.
Policies: the file passes under the default vote, and -- in child processes, the switches being process-static -- under MA_FORCE_FAST=1
and MA_FORCE_EXACT=1 (test_edge_products_under_forced_policy).  Every input is inside the limb contract, so nothing is skipped under
MA_FORCE_FAST=1.

Finding (fixed with this file): modnsqr voted once on its input and then ran k split squarings; the limb contract is not closed under
squaring for operands with the maximum in every limb (the Montgomery top limb is unmasked), and from the second squaring on the words
differed from the reference's (NIST256, k = 5).  k_nsqr now votes before every squaring.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import edge_inputs as ei
from tests.util import derive_any, generated_tags, to_dev, to_np

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = ["X25519", "NIST256", "X448"]
EXTRA = list(__import__("modarith_amd.emit", fromlist=["EXTRA_PRIMES"]).EXTRA_PRIMES) + generated_tags()
N = (1 << 14) + 3
WAVES = 4096                    # elements [WAVES, WAVES + 128): all-maximal
LONE = 12288 + 17               # one all-maximal lane in a wave of uniform ones
N_CHAIN = 300
N_SIMUL = 32768 + 3             # modinv shares inversions from 32 768 elements on (csrc/capi_prime.inc INV_SIMUL_MIN)
IN_CHILD = os.environ.get("MA_POLICY_CHILD") == "1"
CHILD_TIMEOUT = 360              # 3 x the 119 s measured for this file under the default policy (test_edge_products_under_forced_policy)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


class Ctx:
    pass


@pytest.fixture(scope="module", params=CORE + EXTRA)
def ctx(request, torch_cuda, oracle):
    from modarith_amd import emit
    from modarith_amd.field import Field
    c = Ctx()
    c.P = request.param
    c.fp = derive_any(c.P)
    c.F = Field(c.P, tile=None)                                  # flat rows; the tiled layout has a test of its own
    c.ref = ei.Ref(oracle, c.P)
    H = emit.split_point(c.fp) or (c.fp.radix + 2) // 2
    a, b, info = ei.build_inputs(c.fp, H, N, seed=7000 + (CORE + EXTRA).index(c.P))
    top = np.uint64(info["top"])
    assert info["mixture"][0] < WAVES and info["uniform"][0] <= LONE - 17 and LONE + 64 < N - 3
    for x in (a, b):
        x[:, WAVES:WAVES + 128] = top
        x[:, LONE] = top
        x[:, -3:] = top
    c.a, c.b, c.info = a, b, info
    c.A, c.B = to_dev(a), to_dev(b)
    return c


def test_products_flat(ctx):
    """modmul, modsqr, nres, redc (pseudo-Mersenne primes take their own path through the last two): flat rows, n odd"""
    c, F = ctx, ctx.F
    ei.assert_same(c.P, "modmul", c.a, c.b, to_np(F.modmul(c.A, c.B)), c.ref.modmul(c.a, c.b))
    for op in ("modsqr", "nres", "redc"):
        ei.assert_same(c.P, op, c.a, None, to_np(getattr(F, op)(c.A)), c.ref.un(op, c.a))


def test_products_tiled(ctx, torch_cuda):
    """the tiled layout [n / 4096, N, 4096] on the multiple-of-4096 prefix"""
    from modarith_amd.field import Field
    c = ctx
    Ft = Field(c.P, tile=4096)
    m = (N // 4096) * 4096
    a, b = np.ascontiguousarray(c.a[:, :m]), np.ascontiguousarray(c.b[:, :m])
    At, Bt = Ft.to_tiled(c.A[:, :m].contiguous()), Ft.to_tiled(c.B[:, :m].contiguous())
    assert At.dim() == 3
    ei.assert_same(c.P, "modmul (tiled)", a, b, to_np(Ft.to_flat(Ft.modmul(At, Bt))), c.ref.modmul(a, b))
    for op in ("modsqr", "nres", "redc"):
        ei.assert_same(c.P, op + " (tiled)", a, None, to_np(Ft.to_flat(getattr(Ft, op)(At))), c.ref.un(op, a))


def test_products_unaligned(ctx, torch_cuda):
    """an unaligned view (A[:, 1:] with out=): the 8-byte-per-lane kernels"""
    c, F = ctx, ctx.F
    a, b = np.ascontiguousarray(c.a[:, 1:]), np.ascontiguousarray(c.b[:, 1:])
    out = torch_cuda.empty_like(c.A)
    F.modmul(c.A[:, 1:], c.B[:, 1:], out=out[:, 1:])
    ei.assert_same(c.P, "modmul (unaligned)", a, b, to_np(out)[:, 1:], c.ref.modmul(a, b))
    for op in ("modsqr", "nres", "redc"):
        out = torch_cuda.empty_like(c.A)
        getattr(F, op)(c.A[:, 1:], out=out[:, 1:])
        ei.assert_same(c.P, op + " (unaligned)", a, None, to_np(out)[:, 1:], c.ref.un(op, a))


def test_modmuls_every_class(ctx):
    """shared multiplicand: each class in every limb as the common operand (all inside the contract: the host check of the common
    operand lets the FAST kernel run under the default policy)"""
    c, F = ctx, ctx.F
    for e in c.info["E"]:
        b0 = [int(e)] * c.fp.nlimbs
        bb = np.ascontiguousarray(np.repeat(np.array(b0, dtype=np.uint64)[:, None], N, axis=1))
        ei.assert_same(c.P, "modmuls(b0 = %x in every limb)" % e, c.a, bb, to_np(F.modmuls(c.A, b0)), c.ref.modmul(c.a, bb))


@pytest.mark.parametrize("k", [1, 2, 5])
def test_modnsqr(ctx, k):
    """k squarings in place; every element, the all-maximal ones included: from the second squaring on their operands are outside the limb
    contract (unmasked Montgomery top limb), and the kernel has to notice"""
    c, F = ctx, ctx.F
    x = c.A.clone()
    assert F.modnsqr(x, k).data_ptr() == x.data_ptr()
    ei.assert_same(c.P, "modnsqr(k = %d)" % k, c.a, None, to_np(x), c.ref.modnsqr(c.a, k))


def test_chains(ctx):
    """redc(modinv), redc(modsqrt), modqr on the records of edge_inputs.chain_records (why those: there), against the oracle and, for the
    inverse, Python integers; a value = 0 (the all-zero record, p and 2p as limbs) gives 0"""
    c, F, fp = ctx, ctx.F, ctx.fp
    x, vals = ei.chain_records(fp, c.a, c.info, N_CHAIN)
    X = to_dev(x)
    winv = c.ref.un("redc", c.ref.un("modinv", x))
    ei.assert_same(c.P, "redc(modinv)", x, None, to_np(F.redc(F.modinv(X))), winv)
    ei.assert_same(c.P, "redc(modsqrt)", x, None, to_np(F.redc(F.modsqrt(X))), c.ref.un("redc", c.ref.un("modsqrt", x)))
    got, want = F.modqr(None, X).cpu().numpy(), c.ref.modqr(x)
    assert np.array_equal(got, want), (c.P, "modqr", ei.policy_name(), int(np.nonzero(got != want)[0][0]))
    Minv = pow(fp.R, -1, fp.p) if fp.montgomery else 1
    for i, (v, w) in enumerate(zip(vals, ei.values(fp, winv))):
        xv = v * Minv % fp.p
        assert w == (pow(xv, -1, fp.p) if xv else 0), (c.P, "modinv vs integers", ei.hexrec(x, i))


def test_modinv_shared_inversions(ctx):
    """modinv from 32 768 elements on shares one inversion between elements (k_inv_simul): values below 2p with zeros among them (0, p, 2p
    as limbs, a whole wave of zeros, the tail) -- a zero gives 0 and does not disturb its neighbours"""
    c, F, fp = ctx, ctx.F, ctx.fp
    x, _ = ei.chain_records(fp, c.a, c.info, N_SIMUL, seed=5)
    x = np.ascontiguousarray(x[:, -N_SIMUL:])
    p = fp.p
    zeros = np.array([fp.to_limbs(0), fp.to_limbs(p), fp.to_limbs(2 * p)], dtype=np.uint64).T
    for j, z in ((0, 0), (1, 1), (77, 2), (16384 + 5, 1), (N_SIMUL - 1, 1), (N_SIMUL - 2, 0)):
        x[:, j] = zeros[:, z]
    x[:, 8192:8192 + 64] = 0
    X = to_dev(x)
    want = c.ref.un("redc", c.ref.un("modinv", x))
    assert not want[:, 8192:8192 + 64].any() and not want[:, 1].any()
    ei.assert_same(c.P, "redc(modinv), n = %d" % N_SIMUL, x, None, to_np(F.redc(F.modinv(X))), want)


PER_PRIME = [v for k, v in sorted(globals().items()) if k.startswith("test_") and callable(v)]


def expected_tests():
    """the number of tests this file collects for a forced-policy child: every per-prime test, times its own parameters, for every prime"""
    per = 0
    for f in PER_PRIME:
        marks = [m for m in getattr(f, "pytestmark", []) if m.name == "parametrize"]
        k = 1
        for m in marks:
            k *= len(m.args[1])
        per += k
    return per * len(CORE + EXTRA)


@pytest.mark.skipif(IN_CHILD, reason="already inside a forced-policy child")
@pytest.mark.parametrize("knob", ["MA_FORCE_FAST", "MA_FORCE_EXACT"])
def test_edge_products_under_forced_policy(knob):
    """MA_FORCE_FAST / MA_FORCE_EXACT are read once per process (csrc/capi_common.hip): this file again in a fresh pytest child per knob,
    one at a time; it must pass every test it collects.  Measured on the MI355X: 119 s for this file under the default policy (423 tests;
    most of it the oracle on the host); the child's limit is three times that, for a shared machine."""
    env = dict(os.environ, MA_POLICY_CHILD="1")
    env.pop("MA_FORCE_EXACT", None)
    env.pop("MA_FORCE_FAST", None)
    env[knob] = "1"
    p = subprocess.run([sys.executable, "-m", "pytest", "tests/test_gpu_edge_products.py", "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=CHILD_TIMEOUT)
    tail = p.stdout[-3000:] + p.stderr[-500:]
    assert p.returncode == 0, tail
    last = [l for l in p.stdout.splitlines() if " passed" in l][-1]
    assert int(last.split(" passed")[0].split()[-1]) == expected_tests(), tail

