"""The per-lane hash functions of modarith_amd/csrc/hash.h on the CPU, against hashlib and literal FIPS vectors (no GPU).

tools/hash_host.hip compiles the very record functions the kernels of csrc/capi_hash.hip wrap (the part cursor, the padding rules,
SHA-256 / SHA-512 compression, Keccak-f and the squeeze) with --offload-host-only.  Every padding edge of every block size, every
SHAKE output length around the rate and every split of a message into parts runs through it; the same program built with
AddressSanitizer and UBSan runs the sweep once more (each part and each digest sits in an exact-size heap block there).
"""
import hashlib
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

SHA2 = {"sha256": (hashlib.sha256, (0, 1, 55, 56, 57, 63, 64, 65, 119, 120, 128)),
        "sha384": (hashlib.sha384, (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 256)),
        "sha512": (hashlib.sha512, (0, 1, 111, 112, 113, 127, 128, 129, 239, 240, 256))}
KECCAK = {"sha3-224": (hashlib.sha3_224, 144), "sha3-256": (hashlib.sha3_256, 136), "sha3-384": (hashlib.sha3_384, 104),
          "sha3-512": (hashlib.sha3_512, 72), "shake128": (hashlib.shake_128, 168), "shake256": (hashlib.shake_256, 136)}
BLOCK = {"sha256": 64, "sha384": 128, "sha512": 128, **{k: r for k, (_, r) in KECCAK.items()}}


def keccak_lengths(r):
    return (0, 1, r - 2, r - 1, r, r + 1, 2 * r - 1, 2 * r)


def message(n, seed=0):
    return hashlib.shake_128(b"hash_host %d" % seed).digest(n) if n else b""


def truth(algo, msg, olen):
    if algo in SHA2:
        return SHA2[algo][0](msg).digest()
    fn = KECCAK[algo][0]
    return fn(msg).digest(olen) if algo.startswith("shake") else fn(msg).digest()


def splits(msg, block):
    """the same message cut into 1, 2, 4 and 8 parts: cuts at byte offsets 0, 1, 3, 7 and across a block edge, empty parts included"""
    n = len(msg)
    cut = lambda at: [msg[a:b] for a, b in zip([0] + at, at + [n])]
    c = lambda v: max(0, min(n, v))
    yield cut([])
    for at in (0, 1, 3, 7, block - 1, block + 1):
        yield cut([c(at)])
    yield cut([c(0), c(1), c(3)])
    yield cut([c(3), c(7), c(block + 3)])
    yield cut([c(block - 3), c(block - 3), c(block + 5)])
    yield cut([c(0), c(1), c(3), c(7), c(7), c(block - 1), c(block + 1)])
    yield cut([c(1), c(block), c(block), c(block + 1), c(2 * block - 1), c(2 * block), c(n)])


def requests():
    """(algorithm, olen, parts, expected digest)"""
    out = []
    for algo, (_, lengths) in SHA2.items():
        for n in lengths:
            out.append((algo, 0, [message(n, n)], truth(algo, message(n, n), 0)))
    for algo, (_, r) in KECCAK.items():
        for n in keccak_lengths(r):
            out.append((algo, 32, [message(n, n)], truth(algo, message(n, n), 32)))
        if algo.startswith("shake"):
            for olen in (1, 32, 114, r - 1, r, r + 1, 2 * r + 5):
                for n in (0, 67, r - 1):
                    out.append((algo, olen, [message(n, olen)], truth(algo, message(n, olen), olen)))
    for algo in list(SHA2) + list(KECCAK):
        b = BLOCK[algo]
        for n in (0, 7, b - 1, b + 9, 2 * b + 3):
            msg = message(n, 1000 + n)
            want = truth(algo, msg, 57)
            for parts in splits(msg, b):
                assert len(parts) in (1, 2, 4, 8) and b"".join(parts) == msg
                out.append((algo, 57, parts, want))
    return out


def text_of(reqs):
    return "".join("%s %d %s\n" % (algo, olen, " ".join(p.hex() or "-" for p in parts)) for algo, olen, parts, _ in reqs)


def compile_host(tmp, name, extra=()):
    cc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    exe = os.path.join(tmp, name)
    cmd = [cc, "-O1", "-std=c++17", "-w", "--offload-host-only", *extra, "-I", os.path.join(ROOT, "modarith_amd", "csrc"),
           os.path.join(ROOT, "tools", "hash_host.hip"), "-o", exe]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-4000:]
    return exe


def run(exe, text, env=None):
    p = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, (p.returncode, p.stdout[-500:], p.stderr[-3000:])
    return p.stdout.split()


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return compile_host(str(tmp_path_factory.mktemp("hash_host")), "hash_host")


def test_literal_vectors(host):
    """FIPS 180-4 "abc" (SHA-256 / 384 / 512), and the empty message of SHA3-256 and SHAKE256 (FIPS 202 example values)"""
    abc = b"abc".hex()
    got = run(host, "sha256 0 %s\nsha384 0 %s\nsha512 0 %s\nsha3-256 0 -\nshake256 32 -\n" % (abc, abc, abc))
    assert got == [
        "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad",
        "cb00753f45a35e8bb5a03d699ac65007272c32ab0eded1631a8b605a43ff5bed8086072ba1e7cc2358baeca134c825a7",
        "ddaf35a193617abacc417349ae20413112e6fa4e89a97ea20a9eeee64b55d39a2192992a274fc1a836ba3c23a3feebbd454d4423643ce80e2a9ac94fa54ca49f",
        "a7ffc6f8bf1ed76651c14756a061d662f580ff4de43b49fa82d80a4b80f8434a",
        "46b9dd2b0ba88d13233b3feb743eeb243fcd52ea62b81b82b50c27646ed5762f"]


def test_padding_edges_output_lengths_and_part_splits_against_hashlib(host):
    reqs = requests()
    assert len(reqs) > 600
    got = run(host, text_of(reqs))
    assert len(got) == len(reqs)
    bad = [(a, o, [len(p) for p in parts]) for (a, o, parts, want), g in zip(reqs, got) if g != want.hex()]
    assert not bad, "%d of %d differ, first: %r" % (len(bad), len(reqs), bad[:3])


def test_length_entries_are_clamped_to_the_part(host):
    """a lens[] entry above the part's length hashes the part's own bytes; below it, that many"""
    a, b = message(57, 1), message(80, 2)
    text = ("shake256 114 %s:1000 %s:33\n" % (a.hex(), b.hex())) + ("sha512 0 %s:57 %s:0 %s:4294967295\n" % (a.hex(), b.hex(), b.hex()))
    got = run(host, text)
    assert got == [hashlib.shake_256(a + b[:33]).hexdigest(114), hashlib.sha512(a + b).hexdigest()]


def test_sweep_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """the same stand-alone program with -fsanitize=address,undefined: one run of the whole sweep, nothing preloaded"""
    exe = compile_host(str(tmp_path), "hash_host_san", ("-g", "-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
    reqs = requests()
    got = run(exe, text_of(reqs))
    assert got == [want.hex() for _, _, _, want in reqs]
