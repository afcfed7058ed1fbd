#!/usr/bin/env python3
"""Rate of the chain kernels of this checkout against another build's plug-ins, in ONE process on the same buffers (GPU box).

  python tools/chain_ab_rate.py --parent DIR [--out FILE]

DIR holds the other build's plug-ins -- libmodarith_amd_chain_bench_prod_X25519.so and libmodarith_amd_chain_rate_prod_<P>_w32.so for the
three 32-bit primes, built from that checkout (its fuse.bench_chain / tools/w32_chain_rate.chain with build(plugin_dir=...)) -- in two
copies, DIR/a and DIR/b: the second copy is the A/A control.  This checkout's own plug-ins must be built.  Where the other build's
plug-ins cannot find libmodarith_amd.so by their run path, put this checkout's modarith_amd/ on LD_LIBRARY_PATH.
Timed: bench_prod / X25519 through _batch (2^24 elements on tiles of 4096) and _aos (2^22), rate_prod at word length 32 in the default
shape (2^24 on tiles of 4096); device events around single launches, parent / parent copy / new alternating, warm-up first, 25 launches
each, medians; every kernel's output is compared with the call-by-call sequence before it is timed.  Bound: new <= parent * (1 + m),
m = twice the relative difference of the two parent copies' medians in the same run (docs/measurement.md: placement moves these kernels by
more than code does).  Exit status 1 where a case misses it.  "rate" of profiles/chain_one_include.json and of profiles/chain_one_entry.json is this tool's output."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402
from modarith_amd import _lib  # noqa: E402
from modarith_amd import generate as gen  # noqa: E402
from modarith_amd.field import Field  # noqa: E402
from modarith_amd.fuse import FusedChain, bench_chain  # noqa: E402
import w32_chain_rate  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chain_one_include_rate.json"))
args = ap.parse_args()
LAUNCHES = 25
PAR = os.path.abspath(args.parent)
assert torch.cuda.is_available()
_lib.load()


def trio(chain):
    name = os.path.basename(chain.lib_path())
    new = chain.lib_path()
    assert os.path.exists(new), new
    return {"parent": FusedChain(chain, os.path.join(PAR, "a", name), False), "parent_copy": FusedChain(chain, os.path.join(PAR, "b", name), False),
            "new": FusedChain(chain, new, False)}


def measure(runs, check):
    for k, run in runs.items():
        check(k, run)
    for _ in range(2):
        for run in runs.values():
            for _ in range(5):
                run()
    torch.cuda.synchronize()
    ev = {k: [] for k in runs}
    for _ in range(LAUNCHES):
        for k, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            ev[k].append((e0, e1))
    torch.cuda.synchronize()
    ms = {k: statistics.median(a.elapsed_time(b) for a, b in v) for k, v in ev.items()}
    m = 2 * abs(ms["parent"] - ms["parent_copy"]) / min(ms["parent"], ms["parent_copy"])
    res = {"median_ms": ms, "m": m, "bound_ms": ms["parent"] * (1 + m), "within_bound": ms["new"] <= ms["parent"] * (1 + m)}
    print(json.dumps(res), flush=True)
    return res


out = {"launches_each": LAUNCHES, "device": torch.cuda.get_device_name(0), "timing": "device events around single launches, alternating parent / parent copy / new, warm-up first, medians",
       "bound": "new <= parent * (1 + m), m = twice the relative difference of the two parent copies' medians in the same run", "cases": {}}

# 64 bits: bench_prod / X25519, _batch at 2^24 on tiles of 4096 and _aos at 2^22
F = Field("X25519", tile=4096)
n = 1 << 24
x, y, z = F.nres(F.uniform(n, seed=31, array=0)), F.nres(F.uniform(n, seed=31, array=1)), F.empty(n)
fs = trio(bench_chain("X25519"))
want = F.modsqr(F.modmul(F.modadd(x, y), F.modsub(x, y)))


def chk(k, run):
    z.zero_()
    run()
    assert torch.equal(z, want), k


print("bench_prod/X25519 _batch", flush=True)
out["cases"]["bench_prod/X25519/_batch 2^24 tiles of 4096"] = measure({k: (lambda f: lambda: f(x, y, out=[z]))(f) for k, f in fs.items()}, chk)
del x, y, z, want
torch.cuda.empty_cache()
Ff = Field("X25519", tile=None)
n2 = 1 << 22
xf, yf = Ff.nres(Ff.uniform(n2, seed=32, array=0)), Ff.nres(Ff.uniform(n2, seed=32, array=1))
wanta = Ff.to_aos(Ff.modsqr(Ff.modmul(Ff.modadd(xf, yf), Ff.modsub(xf, yf))))
xa, ya = Ff.to_aos(xf), Ff.to_aos(yf)
za = torch.empty_like(xa)


def chka(k, run):
    za.zero_()
    run()
    assert torch.equal(za, wanta), k


print("bench_prod/X25519 _aos", flush=True)
out["cases"]["bench_prod/X25519/_aos 2^22"] = measure({k: (lambda f: lambda: f.aos(xa, ya, out=[za]))(f) for k, f in fs.items()}, chka)
del xf, yf, xa, ya, za, wanta
torch.cuda.empty_cache()

# 32 bits: rate_prod in the default shape
for P in w32_chain_rate.PRIMES:
    F = Field(P, wl=32, tile=4096)
    x, y, z = F.nres(F.uniform(n, seed=31, array=0)), F.nres(F.uniform(n, seed=31, array=1)), F.empty(n)
    fs = trio(w32_chain_rate.chain(P))
    want = F.modsqr(F.modmul(F.modadd(x, y), F.modsub(x, y)))
    print("rate_prod/%s/w32" % P, flush=True)
    out["cases"]["rate_prod/%s/w32 2^24 tiles of 4096" % P] = measure({k: (lambda f: lambda: f(x, y, out=[z]))(f) for k, f in fs.items()}, chk)
    del x, y, z, want
    torch.cuda.empty_cache()

out["all_within_bound"] = all(c["within_bound"] for c in out["cases"].values())
with open(args.out, "w") as f:
    json.dump(out, f, indent=1)
print("all within bound:", out["all_within_bound"], "-> wrote", args.out)
sys.exit(0 if out["all_within_bound"] else 1)
