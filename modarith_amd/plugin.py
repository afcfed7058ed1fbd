"""The one build path of every plug-in: generated fields, curves and ladders (modarith_amd.generate) and fused chains (modarith_amd.fuse).

A caller emits its texts, computes the key they and the kernel sources hash to, and calls build_plugin().  A plug-in whose metadata
carries that key is current and is reused.  Otherwise the units are compiled and linked against libmodarith_amd.so and the metadata is
written, all under names private to the call; then objects, library and metadata are moved into place, the metadata last: whoever
finds the metadata finds a complete plug-in, and a failed or interrupted build leaves the directory as it was.
"""
from __future__ import annotations

import concurrent.futures as cf
import functools
import itertools
import json
import os
import subprocess

from .build import ARCH, FLAGS, HERE, HIPCC, LIB

_calls = itertools.count()
_VERB = {"chain": "fusing"}                 # (every other noun is "generating a ...")


def tmp_suffix() -> str:
    """private to one call, not to one process: threads of one process that build the same target never share a file"""
    return ".%d.%d.tmp" % (os.getpid(), next(_calls))


def include_dirs(d: str) -> list:
    """where every plug-in unit looks for its headers; the target directory before the default one, as the field lookup prefers it"""
    from .generate import PLUGIN_DIR
    return [os.path.join(HERE, "csrc", "generated"), os.path.join(HERE, "csrc"), os.path.join(os.path.dirname(HERE), "include"), d, PLUGIN_DIR]


def is_current(lib: str, meta: str, key: str, force: bool = False) -> bool:
    if force or not (os.path.exists(lib) and os.path.exists(meta)):
        return False
    try:
        return json.load(open(meta)).get("hash") == key
    except (ValueError, OSError):
        return False


def build_plugin(d: str, lib: str, meta: str, record: dict, key: str, units, noun: str, force: bool = False, verbose: bool = False,
                 jobs=(), error=RuntimeError) -> bool:
    """units: (source path, final object path, extra flags) each; jobs: callables run beside the compiles (the field of a 32-bit
    curve); error: what a missing compiler or main library raises.  Returns False when the plug-in was current, True when built."""
    if is_current(lib, meta, key, force):
        return False
    if not os.path.exists(HIPCC):
        raise error("%s not found: %s a %s needs the ROCm compiler (there is no CPU path)" % (HIPCC, _VERB.get(noun, "generating"), noun))
    if not os.path.exists(LIB):
        raise error("%s is missing: build it first (python -m modarith_amd.build); plug-ins link against it" % LIB)
    if verbose:
        print("[modarith_amd] hipcc %s%s%s" % (os.path.basename(units[0][0]), " (three parts)" if len(units) == 3 else "",
                                             "" if noun == "chain" else " -> " + os.path.basename(lib)), flush=True)
    tmp = tmp_suffix()
    inc = [a for i in include_dirs(d) for a in ("-I", i)]
    timeout = int(os.environ.get("MA_BUILD_TIMEOUT", "1500"))
    objs = [obj for _, obj, _ in units]

    def compile_unit(src, obj, extra):
        subprocess.run([HIPCC] + list(FLAGS) + inc + list(extra) + ["-c", src, "-o", obj + tmp], check=True, timeout=timeout)

    work = [functools.partial(compile_unit, *u) for u in units] + list(jobs)
    try:
        if len(work) == 1:
            work[0]()
        else:
            with cf.ThreadPoolExecutor(max_workers=4) as ex:
                for j in [ex.submit(w) for w in work]:
                    j.result()
        subprocess.check_call([HIPCC, "--offload-arch=" + ARCH, "-shared", "-fPIC", "-o", lib + tmp] + [o + tmp for o in objs]
                              + ["-L", HERE, "-l:libmodarith_amd.so", "-Wl,-rpath,$ORIGIN/" + os.path.relpath(HERE, d), "-Wl,-rpath," + HERE])
        with open(meta + tmp, "w") as f:
            json.dump(dict(record, hash=key), f, indent=1)
        for f in objs + [lib, meta]:
            os.replace(f + tmp, f)
    finally:
        for f in objs + [lib, meta]:
            if os.path.exists(f + tmp):
                os.remove(f + tmp)
    return True
