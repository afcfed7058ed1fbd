"""modarith_amd/plugin.py: the one build path of every plug-in -- reuse, clean failure, two threads on one target, missing
prerequisites, install order, search order.  No hipcc and no main library: the compiler is a script that writes a few bytes to its
-o path and logs its command line, the main library a stub file."""
import json
import os
import subprocess
import sys
import threading

import pytest

from modarith_amd import generate as gen
from modarith_amd import plugin
from modarith_amd.fuse import Chain

_CC = """#!%s -SE
import os, sys, time
a = sys.argv[1:]
with open(os.environ["FAKE_CC_LOG"], "a") as f:
    f.write(" ".join(a) + "\\n")
time.sleep(float(os.environ.get("FAKE_CC_SLEEP", "0")))
open(a[a.index("-o") + 1], "w").write("made by: " + " ".join(a))
sys.exit(1 if os.environ.get("FAKE_CC_FAIL", "-") in a else 0)
"""


class Box:
    def __init__(self, tmp_path):
        self.d = str(tmp_path / "plugins")
        self.logfile = str(tmp_path / "cc.log")
        os.makedirs(self.d)

    def log(self):
        return open(self.logfile).read().splitlines() if os.path.exists(self.logfile) else []

    def target(self, units=1):
        """(lib, meta, units) of a plug-in "t" of that many units in the directory"""
        at = lambda f: os.path.join(self.d, f)
        us = []
        for k in range(1, units + 1):
            open(at("t%d.hip" % k), "w").write("// unit %d\n" % k)
            us.append((at("t%d.hip" % k), at("t%d.o" % k), ["-DMA_CURVE_PART=%d" % k]))
        return at("libt.so"), at("t.json"), us

    def build(self, key="k1", units=1, **kw):
        lib, meta, us = self.target(units)
        return plugin.build_plugin(self.d, lib, meta, {"what": "t"}, key, us, "field", **kw)

    def files(self):
        return {f: open(os.path.join(self.d, f), "rb").read() for f in sorted(os.listdir(self.d))}


@pytest.fixture
def box(tmp_path, monkeypatch):
    cc = tmp_path / "fake_hipcc"
    cc.write_text(_CC % sys.executable)
    cc.chmod(0o755)
    (tmp_path / "libmodarith_amd.so").write_text("stub")
    b = Box(tmp_path)
    monkeypatch.setattr(plugin, "HIPCC", str(cc))
    monkeypatch.setattr(plugin, "LIB", str(tmp_path / "libmodarith_amd.so"))
    monkeypatch.setattr(gen, "PLUGIN_DIR", str(tmp_path / "default"))
    monkeypatch.setenv("FAKE_CC_LOG", b.logfile)
    return b


def no_tmp(d):
    return not [f for f in os.listdir(d) if f.endswith(".tmp")]


def test_reuse(box):
    assert box.build() is True
    lib, meta, _ = box.target()
    assert json.load(open(meta)) == {"what": "t", "hash": "k1"} and os.path.exists(lib)
    n = len(box.log())
    assert n == 2                                               # one compile, one link
    assert box.build() is False and len(box.log()) == n
    assert plugin.is_current(lib, meta, "k1") and not plugin.is_current(lib, meta, "k1", force=True)
    assert box.build(force=True) is True and len(box.log()) == 2 * n
    open(meta, "w").write("{ not json")
    assert box.build() is True and len(box.log()) == 3 * n
    assert box.build(key="k2") is True and len(box.log()) == 4 * n           # another hash
    assert json.load(open(meta))["hash"] == "k2" and no_tmp(box.d)


@pytest.mark.parametrize("earlier", [False, True])
def test_failure_is_clean(box, monkeypatch, earlier):
    if earlier:
        assert box.build(units=3) is True
    lib, meta, us = box.target(3)
    before = box.files()
    monkeypatch.setenv("FAKE_CC_FAIL", "-DMA_CURVE_PART=2")
    with pytest.raises(subprocess.CalledProcessError):
        box.build(key="k2", units=3)
    assert no_tmp(box.d)
    assert box.files() == before                                # nothing new, and a good earlier build byte for byte what it was
    assert all(os.path.exists(f) == earlier for f in [lib, meta] + [o for _, o, _ in us])
    assert sum("-DMA_CURVE_PART=" in l for l in box.log()) == (6 if earlier else 3)      # (the failed call did compile)


def test_two_threads_one_target(box, monkeypatch):
    monkeypatch.setenv("FAKE_CC_SLEEP", "0.3")                  # the two calls overlap in their compiles
    res = []

    def run():
        try:
            res.append(box.build(units=3))
        except BaseException as e:
            res.append(e)

    ts = [threading.Thread(target=run) for _ in range(2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert res == [True, True]
    lib, meta, us = box.target(3)
    assert json.load(open(meta)) == {"what": "t", "hash": "k1"}
    assert open(lib).read().startswith("made by: ") and all(open(o).read().startswith("made by: ") for _, o, _ in us)
    assert no_tmp(box.d)
    assert sum("-DMA_CURVE_PART=" in l for l in box.log()) == 6                # both did build


NIST224 = next(c for c in gen.EXAMPLE_CURVES if c["name"] == "NIST224")
M383 = next(c for c in gen.EXAMPLE_LADDERS if c["name"] == "M383")


def _chain(d):
    ch = Chain("X25519", "t")
    ch.output(ch.modsqr(ch.input()))
    return ch.build(plugin_dir=d)


CALLERS = {"field": (lambda d: gen.generate("2**130-5", plugin_dir=d), gen.GenerateError, "generating a field"),
           "field32": (lambda d: gen.generate_w32("2**130-5", plugin_dir=d), gen.GenerateError, "generating a field"),
           "curve": (lambda d: gen.generate_curve(plugin_dir=d, **NIST224), gen.GenerateError, "generating a curve"),
           "curve32": (lambda d: gen.generate_named_curve("SECP256K1", wl=32, plugin_dir=d), gen.GenerateError, "generating a curve"),
           "ladder": (lambda d: gen.generate_ladder(plugin_dir=d, **M383), gen.GenerateError, "generating a ladder"),
           "chain": (_chain, RuntimeError, "fusing a chain")}


@pytest.mark.parametrize("caller", sorted(CALLERS))
@pytest.mark.parametrize("missing", ["HIPCC", "LIB"])
def test_missing_prerequisites(box, monkeypatch, caller, missing):
    call, exc, doing = CALLERS[caller]
    gone = os.path.join(box.d, "not_there")
    monkeypatch.setattr(plugin, missing, gone)
    with pytest.raises(exc) as e:
        call(box.d)
    assert type(e.value) is exc
    want = ("%s not found: %s needs the ROCm compiler (there is no CPU path)" % (gone, doing) if missing == "HIPCC" else
            "%s is missing: build it first (python -m modarith_amd.build); plug-ins link against it" % gone)
    assert str(e.value) == want
    assert box.log() == [] and no_tmp(box.d)
    assert not [f for f in os.listdir(box.d) if f.endswith((".so", ".o"))]


def test_install_order(box, monkeypatch):
    moved, real = [], os.replace
    lib, meta, us = box.target(3)

    def replace(src, dst):
        assert not os.path.exists(meta)                         # the metadata is the last file to appear
        moved.append(dst)
        real(src, dst)

    monkeypatch.setattr(plugin.os, "replace", replace)
    assert box.build(units=3) is True
    assert moved == [o for _, o, _ in us] + [lib, meta] and os.path.exists(meta)


def test_search_order(box):
    here = os.path.dirname(os.path.abspath(plugin.__file__))
    dirs = plugin.include_dirs(box.d)
    assert dirs == [os.path.join(here, "csrc", "generated"), os.path.join(here, "csrc"), os.path.join(os.path.dirname(here), "include"),
                    box.d, gen.PLUGIN_DIR]
    g = gen.generate_named_curve("SECP256K1", wl=32, plugin_dir=box.d)          # three parts, and its field beside them
    assert g.built and no_tmp(box.d)
    compiles = [l.split() for l in box.log() if " -c " in l]
    inc = " ".join("-I " + i for i in dirs)
    assert len(compiles) == 4 and all(inc in " ".join(c) for c in compiles)
    for part, nm in ((1, "mul"), (2, "mul2"), (3, "rest")):
        c, = [c for c in compiles if "-DMA_CURVE_PART=%d" % part in c]
        obj = os.path.join(box.d, "capi_curve_SECP256K1_w32_ecn_%s.o" % nm)
        assert c[c.index("-c") + 1] == os.path.join(box.d, "capi_curve_SECP256K1_w32.hip")
        assert c[c.index("-o") + 1].startswith(obj + ".") and os.path.exists(obj)
    c, = [c for c in compiles if not any(a.startswith("-DMA_CURVE_PART=") for a in c)]
    assert c[c.index("-c") + 1] == os.path.join(box.d, "capi_SECP256K1_w32.hip")
    assert json.load(open(os.path.join(box.d, "curve_SECP256K1_w32.json")))["hash"] and os.path.exists(gen.plugin_path("SECP256K1", box.d, 32))
