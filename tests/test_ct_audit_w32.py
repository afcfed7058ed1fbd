"""The classifier of tools/ct_audit.py over the 32-bit modcsw / modcmv kernels (ma32::k_cond: csrc/kernels.h at MA_WL = 32, in the three
capi_<PRIME>_w32 objects): what tests/test_ct_audit.py asserts for the 64-bit k_cond -- no branch on lane data, no exec mask narrowed
by lane data, nothing unclassified; the only exec-mask / lane-index branches are those of the grid-stride loop (`t < n`)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_audit  # noqa: E402

W32 = ("X25519", "NIST256", "X448")


@pytest.mark.parametrize("P", W32)
def test_w32_cond_kernels_have_no_data_dependent_branch(P):
    obj = os.path.join(ROOT, "modarith_amd", "build", "capi_%s_w32.o" % P)
    if not os.path.exists(obj):
        pytest.skip("no built objects (run __graft_entry__.build())")
    funcs = ct_audit.disassemble(obj)
    syms = list(funcs)
    names = dict(zip(syms, ct_audit.demangle(syms)))
    seen = []
    for sym, ins in funcs.items():
        name = re.sub(r"\(.*", "", re.sub(r"^void ", "", names.get(sym, sym)))
        if "k_cond<" not in name or not ins:
            continue
        a = ct_audit.audit_function(ins)
        seen.append(name)
        assert a["scc_lane_data"] == 0 and a["vcc_lane_data"] == 0 and a["exec_lane_data"] == 0 and a["unknown"] == 0, (name, a["detail"])
        assert a["exec"] + a["lane_index"] <= 2, (name, a["detail"])          # the grid-stride loop: its entry guard and its back edge
        assert a["calls"] == 0, name
    assert sorted(seen) == ["ma32::k_cond<ma32::P_%s_W32, false>" % P, "ma32::k_cond<ma32::P_%s_W32, true>" % P]
