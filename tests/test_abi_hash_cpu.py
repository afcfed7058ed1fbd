"""CPU-side checks of include/modarith_amd_hash.h: every name it declares is exported and bound, the argument refusals come back
as a status without a device, and include/modarith_amd.h declares what it declared before (no GPU, no compute calls)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = 1                          # hipErrorInvalidValue


@pytest.fixture(scope="module")
def lib():
    from modarith_amd import _lib, build
    build.build(verbose=False)
    return _lib.load()


def _declared():
    text = open(os.path.join(ROOT, "include", "modarith_amd_hash.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"^int\s+(\w+)\s*\(", text, flags=re.M)))


def test_every_declared_hash_entry_is_exported_and_bound(lib):
    from modarith_amd import _lib
    names = _declared()
    assert names == sorted(["HASH256_batch", "HASH384_batch", "HASH512_batch", "SHA3_hash_batch", "SHA3_shake_batch"])
    assert set(_lib.HASH_FUNCS) == set(names)
    for n in names:
        f = getattr(lib, n)
        assert f.restype is ctypes.c_int and f.argtypes, n
    assert ctypes.sizeof(_lib.HashPart) == 32 and _lib.HashPart.len.offset == 24      # the C layout of ma_hash_part on LP64


def test_main_header_and_abi_version_are_unchanged(lib):
    """the hash entry points live in a header of their own: modarith_amd.h names none of them, and the ABI version stays 2"""
    main = open(os.path.join(ROOT, "include", "modarith_amd.h")).read()
    assert "HASH" not in main and "SHA3" not in main and "ma_hash_part" not in main
    assert '#include "modarith_amd.h"' in open(os.path.join(ROOT, "include", "modarith_amd_hash.h")).read()
    assert lib.modarith_amd_abi_version() == 2
    from modarith_amd import _lib
    for table in (_lib.BATCH_FUNCS, _lib.SCALAR_FUNCS, _lib.UTIL_FUNCS, _lib.FUSED_FUNCS, _lib.ED_BATCH_FUNCS, _lib.ED_SCALAR_FUNCS):
        assert not any("HASH" in n or "SHA3" in n for n in table)


def test_argument_refusals_need_no_device(lib):
    from modarith_amd._lib import HashPart
    buf = ctypes.create_string_buffer(256)                  # never dereferenced: every call below is refused before a launch
    addr = ctypes.addressof(buf)
    good = (HashPart * 8)(*[HashPart(addr, 16, None, 16) for _ in range(8)])
    err = lambda: lib.modarith_amd_last_error().decode()

    def sha2(f, parts=good, nparts=1, digest=addr, dstride=64, n=4):
        return f(parts, nparts, digest, dstride, n, None)
    for f, dlen in ((lib.HASH256_batch, 32), (lib.HASH384_batch, 48), (lib.HASH512_batch, 64)):
        assert sha2(f, n=0) == 0                            # an empty batch launches nothing
        assert sha2(f, nparts=0) == INVALID and "nparts" in err()
        assert sha2(f, nparts=9) == INVALID
        assert sha2(f, nparts=-1) == INVALID
        assert sha2(f, parts=None) == INVALID and "null" in err()
        assert sha2(f, digest=None) == INVALID
        assert sha2(f, dstride=dlen - 1) == INVALID and "dstride" in err()
        bad = (HashPart * 2)(HashPart(addr, 16, None, 16), HashPart(None, 16, None, 16))
        assert sha2(f, parts=bad, nparts=2) == INVALID and "null" in err()
    sha3 = lambda t, nparts=1, digest=addr, dstride=64, n=4: lib.SHA3_hash_batch(t, good, nparts, digest, dstride, n, None)
    for t in (0, 16, 20, 33, 65, -32):
        assert sha3(t) == INVALID and "t must be" in err()
    for t in (28, 32, 48, 64):
        assert sha3(t, n=0) == 0
        assert sha3(t, nparts=9) == INVALID
        assert sha3(t, dstride=t - 1) == INVALID
        assert sha3(t, digest=None) == INVALID
    shake = lambda t, olen=114, nparts=1, digest=addr, dstride=128, n=4: lib.SHA3_shake_batch(t, good, nparts, digest, dstride, olen, n, None)
    for t in (0, 28, 48, 64, 128, 256):
        assert shake(t) == INVALID and "t must be" in err()
    for t in (16, 32):
        assert shake(t, n=0) == 0
        assert shake(t, olen=0) == INVALID and "olen" in err()
        assert shake(t, dstride=113) == INVALID
        assert shake(t, nparts=0) == INVALID
        assert shake(t, digest=None) == INVALID
    assert lib.modarith_amd_last_launch() not in (b"hash sha256", b"hash shake256")       # nothing was launched
