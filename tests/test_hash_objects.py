"""The hash kernels of csrc/capi_hash.hip in the built object: state and schedule stay in registers (no GPU).

csrc/hash.h indexes the Keccak state, the SHA-2 working variables and the rolling schedule by compile-time constants only, and the
parts of a record by a select over static indices; a regression to a dynamically indexed array shows here as a scratch frame.  From
the metadata of the gfx950 code object (tools/kernel_resources.py): no spilled register, no accumulation register, no private segment.
docs/hash_layer.md records the register counts."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402

EXPECTED = {"k_sha2<ma::hash::Sha256, 32>", "k_sha2<ma::hash::Sha512, 48>", "k_sha2<ma::hash::Sha512, 64>",
            "k_keccak<144, 6>", "k_keccak<136, 6>", "k_keccak<104, 6>", "k_keccak<72, 6>", "k_keccak<168, 31>", "k_keccak<136, 31>"}


@pytest.fixture(scope="module")
def kernels():
    from modarith_amd import build
    build.build(verbose=False)
    obj = os.path.join(build.OBJ, "capi_hash.o")
    if not os.path.exists(obj):                       # a library that travelled without its objects: this one unit again (~30 s)
        os.makedirs(build.OBJ, exist_ok=True)
        build._compile(("capi_hash", "capi_hash", []))
    ks = kernel_resources.kernels_of(obj)
    assert ks, "no gfx950 code object in " + obj
    return {k["name"].split("(")[0].replace("ma::hash::k_", "k_", 1): k for k in ks}


def test_every_hash_kernel_is_there(kernels):
    assert set(kernels) == EXPECTED, sorted(kernels)


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_state_and_schedule_stay_in_registers(kernels, name):
    k = kernels[name]
    assert k["vgpr_spill_count"] == 0 and k["sgpr_spill_count"] == 0, k
    assert k["agpr_count"] == 0, k
    assert k["private_segment_fixed_size"] == 0, k
    assert k["group_segment_fixed_size"] == 0, k
    assert k["vgpr_count"] <= 168, k                  # three waves per SIMD at least (512 registers per lane)
