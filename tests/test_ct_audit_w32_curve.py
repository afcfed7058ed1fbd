"""The classifier of tools/ct_audit.py over the constant-time scalar multiplication of the curve layer at word length 32
(ma32::k_ed_mul<...> in the three capi_<CURVE>_w32_ecn_mul objects): what tests/test_ct_audit.py asserts for the 64-bit k_ed_mul --
no branch on lane data, no exec mask narrowed by lane data, nothing unclassified.  (k_ed_mul2x, the reference's own variable-time
walk, is not a constant-time kernel and is not audited, as its 64-bit counterpart is not.)"""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_audit  # noqa: E402

KERNEL = {"ED25519": "ma32::k_ed_mul<ma32::Edwards<ma32::C_ED25519_W32", "NIST256": "ma32::k_ed_mul<ma32::Weierstrass<ma32::C_NIST256_W32",
          "ED448": "ma32::k_ed_mul<ma32::Edwards<ma32::C_ED448_W32"}


@pytest.mark.parametrize("C", sorted(KERNEL))
def test_w32_scalar_multiplication_has_no_data_dependent_branch(C):
    obj = os.path.join(ROOT, "modarith_amd", "build", "capi_%s_w32_ecn_mul.o" % C)
    if not os.path.exists(obj):
        pytest.skip("no built objects (run __graft_entry__.build())")
    funcs = ct_audit.disassemble(obj)
    syms = list(funcs)
    names = dict(zip(syms, ct_audit.demangle(syms)))
    seen = []
    for sym, ins in funcs.items():
        name = re.sub(r"^void ", "", names.get(sym, sym))
        if "k_ed_mul<" not in name or not ins:
            continue
        a = ct_audit.audit_function(ins)
        seen.append(name)
        assert name.startswith(KERNEL[C]) and ", 0>(" in name, name                       # one launch, no vote (GUARD = 0)
        assert a["scc_lane_data"] == 0 and a["vcc_lane_data"] == 0 and a["exec_lane_data"] == 0 and a["unknown"] == 0, (name, a["detail"])
    assert len(seen) == 1, seen
