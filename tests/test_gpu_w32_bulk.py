"""Wide comparison of the 32-bit word form with the reference on the GPU, with no oracle in between: modmul modsqr modadd modsub nres
redc over 2^18 elements x three operand classes per prime (tests/w32_inputs.py bulk_inputs) against the sha256 digests of the
reference's outputs (tests/golden/bulk_digests_w32.json.xz, made by tests/golden/make_golden_w32.py), flat and tiled; and a cross-check
between the two word lengths that needs no fixture: the same integers through Field(P, 32) and Field(P, 64)."""
import numpy as np
import pytest

from tests import w32_inputs as wi
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu


def _dev(F, soa):
    import torch
    return torch.from_numpy(np.ascontiguousarray(soa).view(np.int32)).to(F.device)


def _host(F, t):
    return F.to_flat(t).cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_bulk_digests_gpu(P):
    from modarith_amd.field import Field
    fx = load_golden("bulk_digests_w32.json")
    assert fx["n"] == wi.BULK_N and fx["block"] == wi.BULK_BLOCK and sorted(fx["primes"]) == sorted(wi.W32_PRIMES)
    F = Field(P, wl=32, tile=None)
    compared = 0
    for cls in wi.BULK_CLASSES:
        a, b = wi.bulk_inputs(P, cls)
        fa, fb = _dev(F, a), _dev(F, b)
        ta, tb = F.to_tiled(fa, 4096), F.to_tiled(fb, 4096)
        for op in wi.BULK_OPS:
            want = fx["primes"][P][cls][op]
            assert len(want) == wi.BULK_N // wi.BULK_BLOCK
            for x, y in ((fa, fb), (ta, tb)):
                got = getattr(F, op)(x, y) if op in ("modmul", "modadd", "modsub") else getattr(F, op)(x)
                assert wi.block_digests(_host(F, got)) == want, (P, cls, op, "tiled" if x.dim() == 3 else "flat")
                compared += 1
    assert compared == len(wi.BULK_CLASSES) * len(wi.BULK_OPS) * 2


@pytest.mark.parametrize("P", wi.W32_PRIMES)
def test_the_two_word_lengths_compute_the_same_integers(P):
    """2^20 moduniform elements: the same integers at both word lengths (the model of tests/util.py on a sample too), and
    redc(modmul(nres(a), nres(b))) through Field(P, 32) equals the same through Field(P, 64) -- values, not limbs"""
    import torch
    from modarith_amd.field import Field
    from tests.util import uniform_model
    n = 1 << 20
    F32, F64 = Field(P, wl=32), Field(P)
    p = F32.params.p

    def words(F, t):
        """the VALUES of a batch of plain elements as byte records [n, Nbytes], compared on the device: modexp(nres(t)) -- modexp takes
        the internal form, and the Montgomery factor differs between the word lengths"""
        return F.modexp(F.nres(t))

    a32, b32 = F32.uniform(n, seed=7, array=3), F32.uniform(n, seed=7, array=4)
    a64, b64 = F64.uniform(n, seed=7, array=3), F64.uniform(n, seed=7, array=4)
    assert a32.dtype == torch.int32 and a32.dim() == 3 and a64.dtype == torch.int64
    assert torch.equal(words(F32, a32), words(F64, a64)) and torch.equal(words(F32, b32), words(F64, b64))
    sample = list(range(0, n, 65537)) + [n - 1]
    flat = F32.to_flat(a32)[:, sample].contiguous()
    assert Field(P, wl=32, tile=None).to_ints(flat) == [uniform_model(p, F32.params.n, 7, 3, j) for j in sample]
    c32 = F32.redc(F32.modmul(F32.nres(a32), F32.nres(b32)))
    c64 = F64.redc(F64.modmul(F64.nres(a64), F64.nres(b64)))
    assert torch.equal(words(F32, c32), words(F64, c64))
    va = Field(P, wl=32, tile=None).to_ints(F32.to_flat(a32)[:, sample].contiguous())
    vb = Field(P, wl=32, tile=None).to_ints(F32.to_flat(b32)[:, sample].contiguous())
    vc = Field(P, wl=32, tile=None).to_ints(F32.to_flat(c32)[:, sample].contiguous())
    assert vc == [x * y % p for x, y in zip(va, vb)]
    # plus_p: the same value + p, top limb unmasked
    q32 = F32.uniform(4096, seed=7, array=3, plus_p=True)
    assert Field(P, wl=32, tile=None).to_ints(F32.to_flat(q32)[:, :64].contiguous()) == [uniform_model(p, F32.params.n, 7, 3, j) + p for j in range(64)]
