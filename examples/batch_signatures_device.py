"""examples/batch_signatures_device.py -- the flows of examples/batch_signatures.py with the hashes on the device as well.

ed448.c hashes what it has just computed: ED448_SIGN hashes the private key, multiplies, then hashes dom4 || R || A || M, where R came
out of the multiplication; ED448_VERIFY hashes what arrives with the signature.  With hashlib in a Python loop (batch_signatures.py) a
signing batch crosses to the host and back twice.  Here every hash is one launch of modarith_amd.hash over the records where they
lie -- the SHA3_process loops of ed448.c:219-225, 236-244, 289-298 become the `parts` of one call, no concatenation pass -- and the
clamp, the byte reversals and the slicing of reduce() are torch ops on device tensors.  There is no Python loop over records and no
.cpu() before the verdicts.

Inputs and outputs are device tensors: prv uint8 [n, 57], pub [n, 57], sig [n, 114], messages uint8 [n, Lmax] with int32 [n] lengths.
Each function keeps the reference function's name, argument meaning and step order, as in batch_signatures.py (the yardstick:
tests/test_gpu_hash_signatures.py compares the two byte for byte and verdict for verdict).

    python examples/batch_signatures_device.py   # the two main() programs of the reference on a batch (needs a GPU)
"""
from __future__ import annotations

import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from modarith_amd import hash as mh  # noqa: E402
from modarith_amd.edwards import Curve  # noqa: E402
from modarith_amd.field import Field  # noqa: E402


def _be(le: torch.Tensor, width: int) -> torch.Tensor:
    """little-endian byte columns -> big-endian records of `width` bytes (zero-extended): what modimp and the curve layer take"""
    n, k = le.shape
    out = torch.zeros((n, width), dtype=torch.uint8, device=le.device)
    out[:, width - k:] = le.flip(1)
    return out


def messages(msgs, device="cuda"):
    """a list of byte strings -> (uint8 [n, Lmax] on the device, int32 [n] lengths): how a caller who holds host messages uploads them"""
    lmax = max(1, max(len(m) for m in msgs))
    buf = bytearray(len(msgs) * lmax)
    for j, m in enumerate(msgs):
        buf[j * lmax:j * lmax + len(m)] = m
    rows = torch.frombuffer(buf, dtype=torch.uint8).view(len(msgs), lmax).to(device)
    return rows, torch.tensor([len(m) for m in msgs], dtype=torch.int32, device=device)


# ------------------------------------------------------------------------------------------------ ECDSA, nist256.c
class Nist256Device:
    BYTES = 32

    def __init__(self):
        self.C = Curve("NIST256")
        self.G = Field("NIST256Q", tile=None)

    def reduce(self, h):
        """nist256.c:122-146: 40 little-endian bytes -> integer mod q as 2^248 x + y"""
        G, B = self.G, self.BYTES
        c = G.mod2r(8 * (B - 1), h.shape[0])
        y, _ = G.modimp(_be(h[:, :31], B))
        x, _ = G.modimp(_be(h[:, 31:40], B))
        G.modmul(x, c, x)
        return G.modadd(x, y)

    def key_pair(self, compress: bool, prv):
        """NIST256_KEY_PAIR (nist256.c:150-161) -> uint8 [n, 33] or [n, 65]"""
        x, y, sign = self.C.mulgen_get(prv.contiguous(), want_y=not compress)
        if compress:
            return torch.cat([(sign + 2).to(torch.uint8).unsqueeze(1), x], dim=1)
        return torch.cat([torch.full((x.shape[0], 1), 4, dtype=torch.uint8, device=x.device), x, y], dim=1)

    def sign(self, prv, ran, m, mlen):
        """NIST256_SIGN (nist256.c:196-222) of HASH256(m): ran 40 random bytes per message -> uint8 [n, 64]"""
        G = self.G
        e, _ = G.modimp(mh.sha256([m], lens=[mlen]))
        s, _ = G.modimp(prv.contiguous())
        k = self.reduce(ran)
        x, _, _ = self.C.mulgen_get(G.modexp(k), want_y=False)
        kinv = G.modinv(k)
        r, _ = G.modimp(x)
        G.modmul(s, r, s)
        G.modadd(s, e, s)
        G.modmul(s, kinv, s)
        return torch.cat([G.modexp(r), G.modexp(s)], dim=1)

    def verify(self, pub, m, mlen, sig):
        """NIST256_VERIFY (nist256.c:226-260) of HASH256(m) -> int32 [n] of 0 / 1 on the device.  pub: uint8 [n, 65] (0x04) or [n, 33]"""
        G, B = self.G, self.BYTES
        e, _ = G.modimp(mh.sha256([m], lens=[mlen]))
        r, r_ok = G.modimp(sig[:, :B].contiguous())
        s, s_ok = G.modimp(sig[:, B:].contiguous())
        ok = (r_ok != 0) & (s_ok != 0) & (G.modis0(r) == 0) & (G.modis0(s) == 0)
        sinv = G.modinv(s)
        v = G.modexp(G.modmul(r, sinv))
        u = G.modexp(G.modmul(sinv, e))
        if pub.shape[1] == 1 + 2 * B:
            Q = self.C.set(None, pub[:, 1:1 + B].contiguous(), pub[:, 1 + B:].contiguous())
        else:
            Q = self.C.set((pub[:, 0] & 1).to(torch.int32), pub[:, 1:].contiguous(), None)
        x, y, _ = self.C.mulgen2_get(u, v, Q)
        inf = (x == 0).all(dim=1) & (y[:, :-1] == 0).all(dim=1) & (y[:, -1] == 1)
        e2, _ = G.modimp(x)
        return (ok & ~inf & (G.modcmp(r, e2) != 0)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ EdDSA, ed448.c
class Ed448Device:
    BYTES = 56
    dom4 = b"SigEd448" + b"\0\0"

    def __init__(self):
        self.C = Curve("ED448")
        self.G = Field("ED448Q", tile=None)
        self._dom = None

    def _dom4(self, n):
        """dom4 as a part: one row on the device, uploaded once, shared by the batch (stride 0)"""
        if self._dom is None:
            self._dom = torch.tensor(list(self.dom4), dtype=torch.uint8, device="cuda").unsqueeze(0)
        return self._dom.expand(n, len(self.dom4))

    def H(self, parts, lens, olen):
        """ed448.c:107-117: SHAKE256 of the parts of every record, olen bytes"""
        return mh.shake256(parts, olen, lens=lens)

    def reduce(self, h):
        """ed448.c:121-153: 114 little-endian bytes -> integer mod q as 2^440 (2^440 x + y) + z"""
        G, B = self.G, self.BYTES
        c = G.mod2r(440, h.shape[0])
        z, _ = G.modimp(_be(h[:, :55], B))
        y, _ = G.modimp(_be(h[:, 55:110], B))
        x, _ = G.modimp(_be(h[:, 110:114], B))
        G.modmul(x, c, x)
        G.modadd(x, y, x)
        G.modmul(x, c, x)
        return G.modadd(x, z)

    def _clamp_be(self, h):
        """the first 56 bytes of a hash as the secret scalar (ed448.c:176-178), big endian"""
        s = h[:, :self.BYTES].clone()
        s[:, 0] &= 0xFC
        s[:, 55] |= 0x80
        return s.flip(1).contiguous()

    @staticmethod
    def _encode(y, sign):
        """ecnXXXget's y (big endian) and the sign of x -> the 57-byte point record"""
        return torch.cat([y.flip(1), (sign << 7).to(torch.uint8).unsqueeze(1)], dim=1)

    def key_pair(self, prv):
        """ED448_KEY_PAIR (ed448.c:167-186): prv uint8 [n, 57] -> pub uint8 [n, 57]"""
        s = self._clamp_be(self.H([prv], None, self.BYTES))
        _, y, sign = self.C.mulgen_get(s, want_x=False)
        return self._encode(y, sign)

    def sign(self, prv, pub, m, mlen):
        """ED448_SIGN (ed448.c:191-257) -> sig uint8 [n, 114]"""
        G, B = self.G, self.BYTES
        n = prv.shape[0]
        if pub is None:
            pub = self.key_pair(prv)
        h = self.H([prv], None, 2 * B + 2)
        s, _ = G.modimp(self._clamp_be(h))
        dom = self._dom4(n)
        r = self.reduce(self.H([dom, h[:, B + 1:], m], [None, None, mlen], 2 * B + 2))           # the prefix where the hash left it
        _, y, sign = self.C.mulgen_get(G.modexp(r), want_x=False)
        R = self._encode(y, sign)
        d = self.reduce(self.H([dom, R, pub, m], [None, None, None, mlen], 2 * B + 2))
        G.modmul(d, s, d)
        G.modadd(d, r, d)
        return torch.cat([R, G.modexp(d).flip(1), torch.zeros((n, 1), dtype=torch.uint8, device=R.device)], dim=1)

    def verify(self, pub, m, mlen, sig):
        """ED448_VERIFY (ed448.c:261-311) -> int32 [n] of 0 / 1 on the device"""
        G, C, B = self.G, self.C, self.BYTES
        n = sig.shape[0]
        R = C.set((sig[:, B] >> 7).to(torch.int32), None, sig[:, :B].flip(1).contiguous())
        ok = C.isinf(R) == 0
        Q = C.set(((pub[:, B] >> 7) & 1).to(torch.int32), None, pub[:, :B].flip(1).contiguous())
        ok = ok & (C.isinf(Q) == 0)
        buff = sig[:, B + 1:2 * B + 1].flip(1).contiguous()
        u = self.reduce(self.H([self._dom4(n), sig[:, :B + 1], pub, m], [None, None, None, mlen], 2 * B + 2))   # R: half of the signature row
        G.modneg(u, u)
        h = G.modexp(u)
        _, in_range = G.modimp(buff)
        ok = ok & (in_range != 0)
        Gp = C.cof(C.gen(n))
        C.cof(R)
        C.cof(Q)
        Q = C.mul2(buff, Gp, h, Q)
        return (ok & (C.cmp(R, Q) != 0)).to(torch.int32)


def _row(b: bytes, n: int) -> torch.Tensor:
    return torch.tensor(list(b), dtype=torch.uint8, device="cuda").unsqueeze(0).repeat(n, 1)


def main():
    n = 8
    # nist256.c:264-296, the message hashed on the device in front of it
    sk = bytes.fromhex("519b423d715f8b581f4fa8ee59f4771a5b44c8130b4e3eacca54a56dda72b464")
    ran = bytes.fromhex("94a1bbb14b906a61a280f245f9e93c7f3b4a6247824f5d33b9670787642a68deb9670787642a68de")
    m, mlen = messages([b"sample"] * n)
    N = Nist256Device()
    print("Run ECDSA P-256 over SHA-256 of the message (%d lanes)" % n)
    pub = N.key_pair(True, _row(sk, n))
    print("public key=", bytes(pub[0].tolist()).hex())
    sig = N.sign(_row(sk, n), _row(ran, n), m, mlen)
    print("signature= ", bytes(sig[0].tolist()).hex())
    print("Signature is valid" if bool(N.verify(pub, m, mlen, sig).all()) else "Signature is NOT valid")
    # ed448.c:315-341
    sk = bytes.fromhex("c4eab05d357007c632f3dbb48489924d552b08fe0c353a0d4a1f00acda2c463afbea67c5e8d2877c5e3bc397a659949ef8021e954e0a12274e")
    E = Ed448Device()
    m, mlen = messages([b"\x03"] * n)
    print("Run RFC8032 test vector (%d lanes)" % n)
    pub = E.key_pair(_row(sk, n))
    print("public key= ", bytes(pub[0].tolist()).hex())
    sig = E.sign(_row(sk, n), pub, m, mlen)
    print("signature=  ", bytes(sig[0].tolist()).hex())
    print("Signature is valid" if bool(E.verify(pub, m, mlen, sig).all()) else "Signature is NOT valid")


if __name__ == "__main__":
    main()
