"""The scalar-multiplication kernel of generated curves at word length 32, cross-compiled for gfx950 (no GPU): part 1 of the plug-in unit
(ecn_<c>_w32_mul_batch, ma32::k_ed_mul) of SECP256K1 and NUMS256E (9 limbs), NIST384 (14) and NIST521, ED500 (18).

  * registers (tools/kernel_resources.py): no spilled register, no scratch and no accumulation registers at 9 and 14 limbs; at 18 limbs
    exactly what tools/w32_curve_gen_resources.json records with its reviewed reason -- and whatever scratch is left there lies outside
    the window loop (the loop that runs once per 4-bit window: the last outermost loop of the kernel);
  * constant time (tools/ct_audit.py): no branch on lane data, no exec mask narrowed by lane data, nothing unclassified, as
    tests/test_ct_audit_w32_curve.py asserts for the three built-in curves (the tracer's budget holds at 18 limbs too:
    docs/curve_layer.md "Word length 32, any curve")."""
import bisect
import concurrent.futures as cf
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from modarith_amd import generate as gen
from modarith_amd.build import FLAGS, HIPCC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import ct_audit  # noqa: E402
import kernel_resources  # noqa: E402

CURVES = {"SECP256K1": ("Weierstrass", 9), "NUMS256E": ("Edwards", 9), "NIST384": ("Weierstrass", 14), "NIST521": ("Weierstrass", 18), "ED500": ("Edwards", 18)}
RECORD = json.load(open(os.path.join(ROOT, "tools", "w32_curve_gen_resources.json")))

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (cross-compiles for gfx950)")


@pytest.fixture(scope="module")
def objects(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("w32_curve_objects"))
    csrc = os.path.join(ROOT, "modarith_amd", "csrc")
    inc = ["-I", os.path.join(csrc, "generated"), "-I", csrc, "-I", os.path.join(ROOT, "include"), "-I", d, "-I", gen.PLUGIN_DIR]

    def compile_mul(c):
        gen.generate_named_curve(c, wl=32, plugin_dir=d, emit_only=True)
        o = os.path.join(d, "capi_curve_%s_w32_ecn_mul.o" % c)
        p = subprocess.run([HIPCC] + list(FLAGS) + inc + ["-DMA_CURVE_PART=1", "-c", os.path.join(d, "capi_curve_%s_w32.hip" % c), "-o", o],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=1500)
        assert p.returncode == 0, p.stdout[-3000:]
        return o
    with cf.ThreadPoolExecutor(max_workers=min(5, os.cpu_count() or 1)) as ex:
        return dict(zip(CURVES, ex.map(compile_mul, CURVES)))


def the_kernel(obj, C):
    ks = [k for k in kernel_resources.kernels_of(obj) if "k_ed_mul<" in k["name"]]
    assert len(ks) == 1 and re.sub(r"^void ", "", ks[0]["name"]).startswith("ma32::k_ed_mul<ma32::%s<ma32::C_%s_W32" % (CURVES[C][0], C)) and ", 0>(" in ks[0]["name"], ks
    return ks[0]


@pytest.mark.parametrize("C", sorted(CURVES))
def test_registers_and_scratch(objects, C):
    k = the_kernel(objects[C], C)
    got = {key: k[key] for key in ("vgpr_count", "agpr_count", "vgpr_spill_count", "private_segment_fixed_size")}
    if CURVES[C][1] < 18:
        assert got["vgpr_spill_count"] == 0 and got["private_segment_fixed_size"] == 0 and got["agpr_count"] == 0 and got["vgpr_count"] <= 256, (C, got)
        return
    rec = RECORD["k_ed_mul"][C]
    assert rec["why"] and got == {key: rec[key] for key in got}, (C, got, rec)
    # whatever scratch is left is touched outside the window loop
    funcs = ct_audit.disassemble(objects[C])
    ins = next(v for s, v in funcs.items() if "k_ed_mul" in s and v)
    addr, text = [a for a, _ in ins], [t for _, t in ins]
    scratch = [i for i, t in enumerate(text) if t.startswith("scratch_")]
    loops = []
    for i, t in enumerate(text):
        if t.startswith(("s_cbranch", "s_branch")):
            off = int(t.split()[-1])
            j = bisect.bisect_left(addr, addr[i] + 4 + 4 * (off - 65536 if off >= 32768 else off))
            if j < i:
                loops.append((j, i))
    outer = [l for l in loops if not any(m != l and m[0] <= l[0] and l[1] <= m[1] for m in loops)]
    window = max(outer, key=lambda l: l[1])
    assert window[1] - window[0] > 5000 and window[1] > len(text) - 2000, (window, len(text))          # four doublings, a table scan and an addition
    inside = [i for i in scratch if window[0] <= i <= window[1]]
    assert len(inside) == rec["scratch_accesses_in_window_loop"] == 0, (C, inside[:8])
    assert (len(scratch) > 0) == (got["private_segment_fixed_size"] > 0)


@pytest.mark.parametrize("C", sorted(CURVES))
def test_scalar_multiplication_has_no_data_dependent_branch(objects, C):
    funcs = ct_audit.disassemble(objects[C])
    syms = list(funcs)
    names = dict(zip(syms, ct_audit.demangle(syms)))
    seen = []
    for sym, ins in funcs.items():
        name = re.sub(r"^void ", "", names.get(sym, sym))
        if "k_ed_mul<" not in name or not ins:
            continue
        a = ct_audit.audit_function(ins)
        seen.append(name)
        assert a["scc_lane_data"] == 0 and a["vcc_lane_data"] == 0 and a["exec_lane_data"] == 0 and a["unknown"] == 0, (name, a["detail"])
    assert len(seen) == 1, seen
