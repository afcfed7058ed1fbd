"""The integer model of tests/curve_model.py, which judges the scratch-less fixed-base kernels (tests/test_gpu_fixed_base_fallbacks.py),
pinned without a GPU: every `mul` record of the four curve fixtures, q*G = (0, 1), and the table form of e*G against the plain
double-and-add."""
import random

import pytest

from tests import curve_model
from tests.conftest import load_golden

FIXTURES = {"ED25519": ("edwards_ED25519.json", 40), "ED448": ("edwards_ED448.json", 20),
            "NIST256": ("weierstrass_NIST256.json", 32), "SECP256K1": ("weierstrass_SECP256K1.json", 28)}


@pytest.fixture(scope="module", params=sorted(FIXTURES))
def mg(request):
    return curve_model.model(request.param), load_golden(FIXTURES[request.param][0]), FIXTURES[request.param][1]


def test_model_takes_its_constants_from_the_fixture(mg):
    m, g, _ = mg
    assert [v.to_bytes(m.nbytes, "big").hex() for v in m.G] == g["gen"] and m.q == int(g["order"], 16)
    x, y = m.G
    if m.name in curve_model.EDWARDS:
        assert (m.a * x * x + y * y - 1 - m.d * x * x * y * y) % m.p == 0
    else:
        assert (y * y - x * x * x - m.a * x - m.b) % m.p == 0


def test_model_reproduces_every_mul_record(mg):
    m, g, count = mg
    assert len(g["mul"]) == count
    for r in g["mul"]:
        P = tuple(int(v, 16) for v in r["P"])
        if r.get("inf"):
            assert m.affine_bytes(int(r["e"], 16), P) == m.export(None), r
        assert [b.hex() for b in m.affine_bytes(int(r["e"], 16), P)] == r["eP"], r


def test_order_times_generator_is_the_neutral_element(mg):
    m, _, _ = mg
    zero, one = (0).to_bytes(m.nbytes, "big"), (1).to_bytes(m.nbytes, "big")
    assert m.mul(m.q, m.G) is None and m.affine_bytes(m.q, m.G) == (zero, one)
    assert m.affine_bytes(0, m.G) == (zero, one) and m.affine_bytes(5, None) == (zero, one)
    minus_g = (-m.G[0] % m.p, m.G[1]) if m.name in curve_model.EDWARDS else (m.G[0], -m.G[1] % m.p)
    assert m.mul(m.q - 1, m.G) == minus_g
    assert m.mul(m.q + 1, m.G) == m.G


def test_table_form_equals_double_and_add(mg):
    """base_bytes (byte-wide table, projective accumulation) against the plain model: scalars with an infinite result (q and the
    largest multiple of q in a record are where the partial sum meets the negative of the last table entry), the neighbours of q,
    single bytes at both ends of the record, and seeded random records"""
    m, _, _ = mg
    top = 1 << (8 * m.nbytes)
    rng = random.Random(20)
    es = [0, 1, 2, 255, 256, 257, m.q - 1, m.q, m.q + 1, top // m.q * m.q, top - 1, top >> 1, (top >> 1) - 1, 255 << (8 * (m.nbytes - 1)),
          m.q + 256, 2 * m.q % top]
    es += [rng.getrandbits(8 * m.nbytes) for _ in range(12)]
    assert m.base_bytes(es) == [m.affine_bytes(e, m.G) for e in es]
