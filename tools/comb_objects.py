#!/usr/bin/env python3
"""The kernels of a list of units, for "is it the same code" between two built trees.

  python tools/comb_objects.py --tree TREE --out figures.json           # TREE: a checkout on which build() has run
  python tools/comb_objects.py --pair PARENT.json NEW.json --out profiles/comb_one_walk.json

--units A,B,...: the objects to read, by default the units that see the fixed-base comb (csrc/comb.h): the G units, which instantiate
the walk, and the F / F2 units, which only include ed26.h, ed28.h, wn26.h, wj26.h or glv26.h.  A name is an object of
modarith_amd/build/ (capi_X25519, capi_ED25519_part2); one with a slash is relative to modarith_amd/ (plugins/capi_ladder_M383, a
generated ladder).  --pair compares the units its two files hold.

Per kernel: the resource figures of tools/kernel_resources.py, the instruction count, a hash of the instruction text as
tools/chain_objects.py takes it (and one that leaves out the pc-relative distances to the object's constant tables), and the loop-weighted instruction and multiply-add counts of tools/isa_mix.py; per tree `nm -D` of the
library.  No GPU needed.
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_mix
import kernel_resources

CURVES = ("ED25519", "ED448", "NIST256", "SECP256K1")


def less_pc_relative(ins):
    """the instruction text with the literal blanked in `s_getpc_b64 s[N:N+1]; s_add_u32 sN, sN, 0x...` -- that pair and no other add: the
    distance from the program counter to a constant table of the same object, which moves when ANOTHER kernel of the object changes size"""
    out = list(ins)
    for k in range(1, len(out)):
        m = re.match(r"s_getpc_b64 s\[(\d+):\d+\]$", ins[k - 1])
        if m:
            out[k] = re.sub(r"^(s_add_u32 s%s, s%s, )0x[0-9a-f]+$" % (m.group(1), m.group(1)), r"\1", ins[k])
    return out
UNITS = ["capi_%s%s" % (c, s) for s in ("G", "F", "F2") for c in CURVES]


def latch_trips(code):
    """{loop head: trips} for the loops whose counter isa_mix does not trace back to its start value, but whose latch is
    `s_cmp_lg_u32 sN, IMM; s_cbranch_scc1 head` -- the shape of `#pragma unroll 1 for (i = 0; i < IMM; i++)`, the window loops: whether
    the start value is found depends on what is scheduled in front of the loop, and an uncounted window loop would make two kernels
    with the same loop look different"""
    loops, out = isa_mix.loops_of(code), {}
    for h, e in loops:
        inner = [(h2, e2) for h2, e2 in loops if (h2, e2) != (h, e) and h <= h2 and e2 <= e]
        if isa_mix.trip_count(code, h, e, inner) is None:
            i = [j for j, (a, _) in enumerate(code) if a == e][0]
            m = re.match(r"s_cmp_lg_u32 s\d+, (\d+)$", code[i - 1][1])
            if m and code[i][1].startswith("s_cbranch_scc1"):
                out["%05x" % h] = int(m.group(1))
    return out


def figures(tree, units=UNITS):
    out = {}
    for u in units:
        obj = os.path.join(tree, "modarith_amd", *(u.split("/") if "/" in u else ("build", u))) + ".o"
        code = {nm: c for (_, nm), c in isa_mix.kernels(obj, "*").items()}
        ks = {}
        for k in kernel_resources.kernels_of(obj):
            c = code[k["name"]]
            a = isa_mix.analyse(c, latch_trips(c))
            ks[k["name"]] = dict({x: k[x] for x in kernel_resources.KEYS}, instructions=sum(a["static"].values()),
                                 weighted_valu=a["valu"], weighted_multiply_adds=a["multiplier"],
                                 isa_sha256=hashlib.sha256("\n".join(ins for _, ins in c).encode()).hexdigest(),
                                 isa_sha256_less_pc_relative=hashlib.sha256("\n".join(less_pc_relative([ins for _, ins in c])).encode()).hexdigest())
        out[u] = ks
    nm = subprocess.run(["nm", "-D", os.path.join(tree, "modarith_amd", "libmodarith_amd.so")], capture_output=True, text=True, check=True).stdout.split("\n")
    out["nm_D"] = sorted(" ".join(l.split()[-2:]) for l in nm if l.strip() and "__hip_cuid_" not in l)
    return out


def pair(parent, new):
    units, differs = {}, []
    assert set(parent) == set(new), sorted(set(parent) ^ set(new))
    names = sorted(u for u in parent if u != "nm_D")
    for u in names:
        kp, kn = parent[u], new[u]
        assert set(kp) == set(kn), (u, sorted(set(kp) ^ set(kn)))
        units[u] = {}
        for nm in sorted(kp):
            if kp[nm] == kn[nm]:
                units[u][nm] = dict(kp[nm], same_as_parent=True)
            else:
                units[u][nm] = {"same_as_parent": False, "parent": kp[nm], "new": kn[nm]}
                fig = [x for x in kp[nm] if not x.startswith("isa_sha256")]
                differs.append({"unit": u, "kernel": nm, "parent_to_new": {x: [kp[nm][x], kn[nm][x]] for x in fig if kp[nm][x] != kn[nm][x]},
                                "no_figure_higher": all(kn[nm][x] <= kp[nm][x] for x in fig),
                                "same_but_for_pc_relative_literals": kp[nm]["isa_sha256_less_pc_relative"] == kn[nm]["isa_sha256_less_pc_relative"]})
    return {"units": units, "kernels": sum(len(v) for v in units.values()), "kernels_whose_instruction_text_differs": differs,
            "units_without_any_difference": [u for u in names if all(k["same_as_parent"] for k in units[u].values())],
            "nm_D_equal_but_for_hip_cuid": parent["nm_D"] == new["nm_D"], "nm_D_symbols": len(new["nm_D"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=kernel_resources.ROOT)
    ap.add_argument("--units", default=",".join(UNITS), help="comma-separated objects (see above); default: the G / F / F2 units")
    ap.add_argument("--pair", nargs=2, default=None, metavar=("PARENT", "NEW"))
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    load = lambda p: json.load(open(p))
    out = pair(*map(load, args.pair)) if args.pair else figures(os.path.abspath(args.tree), args.units.split(","))
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
