"""The signature flows with the hashes on the device (examples/batch_signatures_device.py) against the host-hash flows of
examples/batch_signatures.py, byte for byte and verdict for verdict, and against the RFC 8032 Ed448 vectors.

Ed448Device keeps the step order of ed448.c; every hash is a launch of modarith_amd.hash over the records where they lie (dom4
shared, R as half of the signature row, ragged messages through their lengths).  The yardstick is batch_signatures.Ed448 with
hashlib: same keys, same signatures, same verdicts -- also on the tampered lanes of
tests/test_gpu_signatures.py::test_eddsa_ed448_batch_against_the_integer_model, rebuilt here."""
import hashlib
import os
import random
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "examples"))

RFC8032_ED448 = [   # (secret key, public key, message, signature): RFC 8032 section 7.4, "Blank" and "1 octet"
    ("6c82a562cb808d10d632be89c8513ebf6c929f34ddfa8c9f63c9960ef6e348a3528c8a3fcc2f044e39a3fc5b94492f8f032e7549a20098f95b",
     "5fd7449b59b461fd2ce787ec616ad46a1da1342485a70e1f8a0ea75d80e96778edf124769b46c7061bd6783df1e50f6cd1fa1abeafe8256180",
     "",
     "533a37f6bbe457251f023c0d88f976ae2dfb504a843e34d2074fd823d41a591f2b233f034f628281f2fd7a22ddd47d7828c59bd0a21bfd3980"
     "ff0d2028d4b18a9df63e006c5d1c2d345b925d8dc00b4104852db99ac5c7cdda8530a113a0f4dbb61149f05a7363268c71d95808ff2e652600"),
    ("c4eab05d357007c632f3dbb48489924d552b08fe0c353a0d4a1f00acda2c463afbea67c5e8d2877c5e3bc397a659949ef8021e954e0a12274e",
     "43ba28f430cdff456ae531545f7ecd0ac834a55d9358c0372bfa0c6c6798c0866aea01eb00742802b8438ea4cb82169c235160627b4c3a9480",
     "03",
     "26b8f91727bd62897af15e41eb43c377efb9c610d48f2335cb0bd0087810f4352541b143c4b981b7e18f62de8ccdf633fc1bf037ab7cd77980"
     "5e0dbcc0aae1cbcee1afb2e027df36bc04dcecbf154336c19f0af7e0a6472905e799f1953d2a0ff3348ab21aa4adafd1d234441cf807c03a00"),
]
P448 = 2**448 - 2**224 - 1
Q448 = 2**446 - 0x8335dc163bb124b65129c96fde933d8d723a70aadc873d6d54a7bb0d


@pytest.fixture(scope="module")
def flows():
    import torch
    assert torch.cuda.is_available()
    import batch_signatures as host
    import batch_signatures_device as dev
    return host, dev


def dev_rows(rows):
    import torch
    return torch.tensor([list(r) for r in rows], dtype=torch.uint8, device="cuda")


def host_rows(t):
    return [bytes(r) for r in t.cpu().tolist()]


def test_ed448_device_flow_on_the_rfc8032_vectors(flows):
    _, dev = flows
    E = dev.Ed448Device()
    for sk, pk, m, sg in RFC8032_ED448:
        sk, pk, m, sg = bytes.fromhex(sk), bytes.fromhex(pk), bytes.fromhex(m), bytes.fromhex(sg)
        dm, dl = dev.messages([m] * 3)
        prv = dev_rows([sk] * 3)
        pub = E.key_pair(prv)
        assert host_rows(pub) == [pk] * 3
        assert host_rows(E.sign(prv, None, dm, dl)) == [sg] * 3                  # pub == NULL: derived inside (ed448.c:207-209)
        sig = E.sign(prv, pub, dm, dl)
        assert host_rows(sig) == [sg] * 3
        assert E.verify(pub, dm, dl, sig).tolist() == [1] * 3


def test_ed448_device_flow_matches_the_host_hash_flow_on_ragged_and_tampered_records(flows):
    host, dev = flows
    H, D = host.Ed448(), dev.Ed448Device()
    rng = random.Random(8032)
    n = 24
    prv = [rng.randbytes(57) for _ in range(n)]
    msgs = [rng.randbytes(rng.randrange(0, 120)) for _ in range(n)]
    dprv = dev_rows(prv)
    dm, dl = dev.messages(msgs)
    pub = H.key_pair(prv)
    dpub = D.key_pair(dprv)
    assert host_rows(dpub) == pub
    sig = H.sign(prv, pub, msgs)
    dsig = D.sign(dprv, dpub, dm, dl)
    assert host_rows(dsig) == sig
    assert D.verify(dpub, dm, dl, dsig).tolist() == H.verify(pub, msgs, sig) == [1] * n

    # the tampered lanes of test_eddsa_ed448_batch_against_the_integer_model, valid lanes in between
    bad_sig, bad_msg, bad_pub = list(sig), list(msgs), list(pub)
    S = lambda i: int.from_bytes(sig[i][57:113], "little")                  # noqa: E731
    d448 = -39081 % P448

    def decodes(y):                                                          # does y have an x on the curve: x^2 = (y^2 - 1) / (d y^2 - 1)
        u, v = (y * y - 1) % P448, (d448 * y * y - 1) % P448
        return pow(u * pow(v, -1, P448) % P448, (P448 - 1) // 2, P448) in (0, 1)
    bad_msg[1] = msgs[1] + b"!"
    bad_sig[3] = sig[3][:57] + ((S(3) + 1) % Q448).to_bytes(56, "little") + b"\0"
    bad_sig[5] = sig[5][:57] + (S(5) + Q448).to_bytes(56, "little") + b"\0"  # S + q: same residue, out of range
    bad_sig[7] = sig[6][:57] + sig[7][57:]                                   # R of another signature
    bad_pub[9] = pub[10]
    bad_sig[11] = (1).to_bytes(56, "little") + b"\0" + sig[11][57:]          # R = the neutral element (y = 1)
    bad_pub[13] = (1).to_bytes(56, "little") + b"\0"                         # A = the neutral element
    ynon = next(y for y in range(2, 100) if not decodes(y))
    bad_sig[15] = ynon.to_bytes(56, "little") + b"\0" + sig[15][57:]         # R: y with no x on the curve
    bad_pub[17] = ynon.to_bytes(56, "little") + b"\0"
    bad_sig[19] = (P448 - 1).to_bytes(56, "little") + b"\0" + sig[19][57:]   # R = (0, -1): order 2, killed by the cofactor
    bad_sig[21] = sig[21][:56] + bytes([sig[21][56] ^ 0x80]) + sig[21][57:]  # the other x
    want = H.verify(bad_pub, bad_msg, bad_sig)
    assert sum(want) == n - 11 and [j for j, v in enumerate(want) if not v] == [1, 3, 5, 7, 9, 11, 13, 15, 17, 19, 21]
    bm, bl = dev.messages(bad_msg)
    got = D.verify(dev_rows(bad_pub), bm, bl, dev_rows(bad_sig))
    assert got.is_cuda and got.tolist() == want


def test_nist256_device_verify_agrees_with_the_host_flow_on_hashlib_digests(flows):
    host, dev = flows
    H, D = host.Nist256(), dev.Nist256Device()
    rng = random.Random(186)
    n = 16
    q = 0xffffffff00000000ffffffffffffffffbce6faada7179e84f3b9cac2fc632551
    prv = [rng.randrange(1, q).to_bytes(32, "big") for _ in range(n)]
    ran = [rng.getrandbits(320).to_bytes(40, "little") for _ in range(n)]
    msgs = [rng.randbytes(rng.randrange(0, 200)) for _ in range(n)]
    thm = [hashlib.sha256(m).digest() for m in msgs]
    dm, dl = dev.messages(msgs)
    for compress in (True, False):
        pub = H.key_pair(compress, prv)
        assert host_rows(D.key_pair(compress, dev_rows(prv))) == pub
    sig = H.sign(prv, ran, thm)
    assert host_rows(D.sign(dev_rows(prv), dev_rows(ran), dm, dl)) == sig
    bad_sig, bad_msg = list(sig), list(msgs)
    bad_msg[1] = msgs[1] + b"!"
    bad_sig[3] = b"\0" * 32 + sig[3][32:]                                    # r = 0
    bad_sig[5] = sig[5][:32] + (q + 5).to_bytes(32, "big")                   # s > q
    bad_sig[7] = sig[7][:32] + ((int.from_bytes(sig[7][32:], "big") + 1) % q).to_bytes(32, "big")
    bm, bl = dev.messages(bad_msg)
    for pub in (H.key_pair(True, prv), H.key_pair(False, prv)):
        assert D.verify(dev_rows(pub), dm, dl, dev_rows(sig)).tolist() == H.verify(pub, thm, sig) == [1] * n
        want = H.verify(pub, [hashlib.sha256(m).digest() for m in bad_msg], bad_sig)
        assert sum(want) == n - 4
        assert D.verify(dev_rows(pub), bm, bl, dev_rows(bad_sig)).tolist() == want


def test_example_program_prints_the_rfc8032_transcript():
    """python examples/batch_signatures_device.py: the RFC 8032 public key and signature and both 'Signature is valid' lines"""
    import subprocess
    p = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "batch_signatures_device.py")], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-2000:]
    out = p.stdout
    assert out.count("Signature is valid") == 2 and "NOT valid" not in out
    assert RFC8032_ED448[1][1] in out and RFC8032_ED448[1][3] in out
