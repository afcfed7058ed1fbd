"""Generator mode: a field for ANY prime the reference generators accept, built at run time.

  python -m modarith_amd.generate 64 2**251-9               # the reference's own command-line shape
  python -m modarith_amd.generate 64 BP256=0xa9fb57db...5377 --monty
  python -m modarith_amd.generate 64 2**251-9 --time        # ... and run the time.c protocol on the GPU, as the generators do last
  python -m modarith_amd.generate curve NIST224 weierstrass NIST224 -3 0xb405...ffb4 0xffff...2a3d 0xb70e...1d21 0xbd37...7e34
  python -m modarith_amd.generate w32 BP256=0xa9fb57db...5377      # the same field on uint32_t limbs (`monty.py 32 ...`): generate_w32()
  python -m modarith_amd.generate curve32 NIST384                  # a curve of the table on uint32_t points (`curve.py 32 NIST384`): generate_curve(wl=32)
  python -m modarith_amd.generate --list

This is the counterpart of `python pseudo.py 64 <prime>` / `python monty.py 64 <prime>` (pseudo.py:1461-1473,
1552-1566; monty.py:2111-2135): where the reference writes a specialised field.c for the prime, this driver derives
the same constants (modarith_amd.params), emits them as a `struct P_<TAG>` (modarith_amd.emit.header_text), and has
hipcc instantiate the hand-written kernels of csrc/field.h + csrc/kernels.h for it -- one translation unit, about
ten seconds -- into a plug-in `modarith_amd/plugins/libmodarith_amd_<TAG>.so` that exports the same C-ABI as a
built-in prime: `<fn>_<TAG>_ct` (host pointers, the reference's signatures) and `<fn>_<TAG>_batch` (device
pointers), declared by `MODARITH_AMD_DECLARE(<TAG>)` of include/modarith_amd.h.  The plug-in links against
libmodarith_amd.so (launch geometry, error text, staging buffers); `Field("<TAG>")` loads it.

Naming follows the generators' decoration rule (pseudo.py:1940-1944, monty.py:2510-2520): a named prime keeps its
name; an unnamed pseudo-Mersenne 2^n - m is tagged `<n><m>` ("25519"); any other unnamed modulus must be given a
name (`NAME=<expression>` or `name=`), as monty.py insists ("Modulus must have a name").  generate() builds 64-bit words
(u64 limbs, SURVEY 8 sizes) and refuses 16 / 32 with the reason; the 32-bit word form -- the limbs of the reference's `pseudo.py 32` /
`monty.py 32` and of its CUDA generators -- is generate_w32() / the verb `w32`: the same resolution, tags and refusals at word
length 32, a plug-in `libmodarith_amd_<TAG>_w32.so` over csrc/capi_w32.inc that exports what MODARITH_AMD_DECLARE_W32(<TAG>) of
include/modarith_amd_w32.h declares, next to (and independent of) the 64-bit plug-in of the same tag; `Field("<TAG>", wl=32)` loads it.

How a plug-in is installed and reused -- fields, curves and ladders here, and the fused chains of modarith_amd/fuse.py, all through
build_plugin() of modarith_amd/plugin.py: the generator writes its emitted texts (only those that differ from what is there) and hashes
them with the compile flags and every kernel source (key_of).  A plug-in whose metadata records that hash is current and is returned
with built = False, its directory untouched.  Otherwise the units are compiled and linked against libmodarith_amd.so and the metadata
is written, all under names private to the call, and then moved into place -- objects, library, metadata last -- so that another
thread or process generating or loading the same plug-in never sees a half-written file, and a failed compile leaves nothing behind.
A field is looked for among the built-in primes, then in the directory being generated into, then in the default one (find_field).

There is no CPU path here either: the plug-in contains GPU kernels only, and a missing hipcc is an error.
"""
from __future__ import annotations

import hashlib
import json
import os
import re
import sys
from dataclasses import dataclass
from typing import List, Optional

from . import emit
from .params import NAMED, RADIX_32, FieldParams, derive_monty, derive_pseudo
from .plugin import build_plugin, tmp_suffix

HERE = os.path.dirname(os.path.abspath(__file__))
PLUGIN_DIR = os.environ.get("MA_PLUGIN_DIR", os.path.join(HERE, "plugins"))
_TAG_RE = re.compile(r"^[A-Za-z0-9][A-Za-z0-9_]*$")


# unnamed moduli the test-suite generates (tests/golden/field_<TAG>.json hold what the reference generators emit for them):
# (argument as on the reference's command line, family) -- an unnamed pseudo-Mersenne, a three-limb one, a general 256-bit
# prime (brainpoolP256r1) in full Montgomery form, and monty.py's PM shortcut for an unnamed 2^n - m
EXAMPLES = (("2**251-9", "pseudo"), ("2**130-5", "pseudo"),
            ("BP256=0xa9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377", "monty"), ("M2519=2**251-9", "monty"))


# the 32-bit examples (tests/golden/field_w32gen_<TAG>.json.xz: what `pseudo.py 32` / `monty.py 32` emit for them), one per class: an
# unnamed pseudo-Mersenne (9 x 28), the smallest (5 x 26), full Montgomery with ndash != 1 and a Barrett modmli, negative prime limbs
# (14 x 28), a radix override, 18 limbs (the reduced launch width), a group order, and monty.py's form of 2^251 - 9
EXAMPLES_W32 = (("2**251-9", "pseudo"), ("2**130-5", "pseudo"),
                ("BP256=0xa9fb57dba1eea9bc3e660a909d838d726e3bf623d52620282013481d1f6e5377", "monty"), ("NIST384", None), ("GM240", None),
                ("PM512", None), ("Q25519=00" + str(NAMED["ED25519Q"][0]), "monty"), ("M2519=2**251-9", "monty"))


class GenerateError(ValueError):
    pass


@dataclass
class Generated:
    tag: str                    # the <TAG> of the exported symbols
    lib: str                    # path of the plug-in shared object
    params: FieldParams
    built: bool                 # False when an up-to-date plug-in was reused


def _evaluate(expr: str) -> int:
    """the modulus of a command-line argument: an expression that starts with a digit (pseudo.py:1554-1556), or
    "00" + decimal for a group order (monty.py:2116-2118)"""
    if not expr or not expr[0].isdigit():
        raise GenerateError("%r: an unnamed modulus is a python expression that starts with a digit, e.g. 2**255-19" % (expr,))
    if expr.startswith("00"):
        return int(expr)
    if not re.fullmatch(r"[0-9a-fA-FxX*+\-() ]+", expr):
        raise GenerateError("%r: only integers, + - * ** and parentheses are evaluated" % (expr,))
    return int(eval(expr, {"__builtins__": {}}))


def resolve(prime: str, family: Optional[str] = None, name: Optional[str] = None, radix: Optional[int] = None, wl: int = 64) -> FieldParams:
    """prime (a name of modarith_amd.params.NAMED, an expression, or NAME=expression) -> FieldParams with .name = TAG, at word length wl"""
    if "=" in prime and name is None:
        name, prime = prime.split("=", 1)
    if prime in NAMED:
        p, fam = NAMED[prime]
        name = name or prime
        if wl == 32:
            if radix is None:
                radix = RADIX_32.get(prime)
            if family is None and fam == "pseudo":
                fam = None                # (a named pseudo-Mersenne that does not fit this word length falls back, as params.derive does)
        family = family or fam
    else:
        p = _evaluate(prime)
    n = p.bit_length()
    fp = None
    if family in (None, "pseudo"):
        try:
            fp = derive_pseudo(name or "_", p, radix, wl)
        except ValueError as e:
            if family == "pseudo":
                raise GenerateError("%s (pseudo.py:1563-1592)" % e) from None
    if fp is None:
        try:
            fp = derive_monty(name or "_", p, radix, wl)
        except ValueError as e:
            raise GenerateError("%s (monty.py:2131-2230)" % e) from None
    if name is None:
        if fp.family == "pseudo" or fp.pm:
            name = "%d%d" % (n, (1 << n) - p)                   # the generators' own tag for an unnamed 2^n - m
        else:
            raise GenerateError("Modulus must have a name - unable to make one for you (monty.py:2517-2519): pass NAME=<expression>")
    if not _TAG_RE.match(name):
        raise GenerateError("%r cannot be part of a C identifier" % (name,))
    if name.lower().endswith("_w32"):
        # libmodarith_amd_<TAG>_w32.so / <TAG>_w32.json / <fn>_<TAG>_w32_batch are the names of the 32-bit plug-in of <TAG>
        raise GenerateError("%r: a tag cannot end in _w32, the suffix of the 32-bit word form's files and symbols" % (name,))
    fp.name = name
    return fp


def key_of(*texts: str) -> str:
    """what a plug-in was made from: the flags, its emitted texts and every kernel source (path-independent, so a plug-in built in one
    checkout is recognised as current in a copy of it)"""
    from .build import FLAGS, _stamp
    return hashlib.sha256("\n".join([" ".join(FLAGS)] + list(texts) + [_stamp()]).encode()).hexdigest()


def plugin_path(tag: str, plugin_dir: Optional[str] = None, wl: int = 64) -> str:
    return os.path.join(plugin_dir or PLUGIN_DIR, "libmodarith_amd_%s%s.so" % (tag, "" if wl == 64 else "_w32"))


def _meta_path(tag: str, plugin_dir: Optional[str] = None, wl: int = 64) -> str:
    return os.path.join(plugin_dir or PLUGIN_DIR, "%s%s.json" % (tag, "" if wl == 64 else "_w32"))


def find_field(field: str, d: Optional[str] = None, wl: int = 64, built: bool = False):
    """the field a curve, ladder, chain or Field names -> (FieldParams, directory of its plug-in, or None for a built-in prime); None
    when there is no such field.  Built-in primes first, then the directory d, then the default one.  A generated field is there when
    its metadata is (generate_w32's emit_only writes no more); built=True asks for its shared object instead."""
    from . import _lib
    from .params import derive
    if field in (_lib.PRIMES if wl == 64 else _lib.W32_PRIMES):
        return derive(field, wl=wl), None
    for where in (d or PLUGIN_DIR, PLUGIN_DIR):
        if os.path.exists((plugin_path if built else _meta_path)(field, where, wl)):
            return params_of_plugin(field, where, wl), where
    return None


def _generate_field(prime, wl, family, name, radix, plugin_dir, force, verbose, emit_only=False) -> Generated:
    """generate() and generate_w32(): the word lengths differ in the built-in list, the limb cap, the file stem and the unit text"""
    from . import _lib
    w32 = wl == 32
    builtin, cap = (_lib.W32_PRIMES, emit.MAX_GENERATED_LIMBS_W32) if w32 else (_lib.PRIMES, emit.MAX_GENERATED_LIMBS)
    fp = resolve(prime, family, name, radix, wl=wl)
    tag = fp.name
    if tag in builtin and NAMED.get(tag, (None,))[0] == fp.p and (family is None or NAMED[tag][1] == fp.family) and radix is None:
        return Generated(tag, _lib.LIB_PATH, fp, False)         # a built-in prime: nothing to generate
    if tag in builtin:
        raise GenerateError("%s names a built-in field with other constants; choose another name" % tag)
    if fp.nlimbs > cap and w32:
        raise GenerateError("%d limbs of %d bits: the 32-bit kernels keep every operand in registers and are built for at most %d limbs "
                            "(no streaming kernel beyond that has been shown free of scratch)" % (fp.nlimbs, fp.radix, cap))
    if fp.nlimbs > cap:
        raise GenerateError("%d limbs: the kernels keep every operand in registers and are built for at most %d limbs" % (fp.nlimbs, cap))
    d = plugin_dir or PLUGIN_DIR
    os.makedirs(d, exist_ok=True)
    at = lambda f: os.path.join(d, f % (tag + "_w32" if w32 else tag))
    unit, lib, meta = at("capi_%s.hip"), plugin_path(tag, d, wl), at("%s.json")
    hdr_text = emit.header_text(fp, generated=w32)
    unit_text = emit.capi_unit_text_w32(tag, fp.nlimbs) if w32 else emit.capi_unit_text(tag)
    key = key_of(hdr_text, unit_text)           # (the 64-bit unit as emit gives it: its include is redirected below, for a unit in d)
    emit._write(at("params_%s.h"), hdr_text)
    # the paste-marker shim of this field, next to its plug-in: what a consumer includes where the reference says "paste field.c here"
    emit._write(at("field_%s.h"), emit.field_shim_text(fp, tag))
    emit._write(unit, unit_text.replace('"../capi_prime.inc"', '"capi_prime.inc"'))
    record = {"tag": tag, "prime": prime, "p": hex(fp.p), "family": fp.family, "radix": fp.radix, "nlimbs": fp.nlimbs}
    if w32:
        record.update(wl=32, ept_max=emit.w32_ept_max(fp.nlimbs))
    if emit_only:
        if not os.path.exists(meta):
            tmp = meta + tmp_suffix()
            with open(tmp, "w") as f:
                json.dump(record, f, indent=1)
            os.replace(tmp, meta)
        return Generated(tag, lib, fp, False)
    built = build_plugin(d, lib, meta, record, key, [(unit, at("capi_%s.o"), [])], "field", force, verbose, error=GenerateError)
    return Generated(tag, lib, fp, built)


def generate(prime: str, wl: int = 64, family: Optional[str] = None, name: Optional[str] = None, radix: Optional[int] = None,
             plugin_dir: Optional[str] = None, force: bool = False, verbose: bool = False) -> Generated:
    """derive the constants of `prime`, emit them (params_<TAG>.h, field_<TAG>.h, capi_<TAG>.hip), compile the kernels for it; returns
    the plug-in to load."""
    if wl != 64:
        raise GenerateError("generate() builds 64-bit words only (u64 limbs, 128-bit column sums); the 32-bit form is generate_w32() / "
                            "`python -m modarith_amd.generate w32 <prime>` (include/modarith_amd_w32.h), the 16-bit form does not exist")
    return _generate_field(prime, 64, family, name, radix, plugin_dir, force, verbose)


def generate_w32(prime: str, family: Optional[str] = None, name: Optional[str] = None, radix: Optional[int] = None,
                 plugin_dir: Optional[str] = None, force: bool = False, verbose: bool = False, emit_only: bool = False) -> Generated:
    """generate() at word length 32: `python pseudo.py 32 <prime>` / `python monty.py 32 <prime>`.  Emits, next to each other in the
    plug-in directory, params_<TAG>_w32.h (emit.header_text: struct ma32::P_<TAG>_W32, with the driver's verdict on the shared
    inversion), capi_<TAG>_w32.hip (three lines over csrc/capi_w32.inc and the launch width the limb count allows), field_<TAG>_w32.h
    (the paste-marker shim), libmodarith_amd_<TAG>_w32.so and the metadata <TAG>_w32.json ("wl": 32).  The 64-bit plug-in of the same
    tag is neither needed nor touched.  X25519, NIST256 and X448 are built in.
    emit_only: write the texts (and, where there is none, the metadata without a hash, so that a curve can be emitted over the tag) and
    return without calling the compiler."""
    return _generate_field(prime, 32, family, name, radix, plugin_dir, force, verbose, emit_only)


# ---------------------------------------------------------------------------------------------------------------------
# curves of one's own: the counterpart of curve.py's table ("More curves can be added here", curve.py:73-203)
@dataclass
class GeneratedCurve:
    name: str                   # upper-case name; symbols ecn_<lower>_*
    kind: str                   # "edwards" | "weierstrass"
    field: str                  # tag of the field (built-in or generated)
    lib: str
    nlimbs: int
    nbytes: int
    built: bool


def curve_plugin_path(name: str, plugin_dir: Optional[str] = None, wl: int = 64) -> str:
    return os.path.join(plugin_dir or PLUGIN_DIR, "libmodarith_amd_curve_%s%s.so" % (name.lower(), "" if wl == 64 else "_w32"))


def _curve_definition(kind, up, field, a, b, order, gx, gy, cof, fp):
    """the checks curve.py leaves to its user (the form edwards.c / weierstrass.c handles, the generator on the curve) -> the
    curves.EdwardsCurve or curves.WeierstrassCurve of the definition, at the word length of fp"""
    from . import curves
    if kind == "edwards":
        if a not in (1, -1):
            raise GenerateError("edwards.c handles a = 1 and a = -1")
        on_curve = a * gx * gx + gy * gy - 1 - b * gx * gx * gy * gy
    else:
        if a not in (-3, 0):
            raise GenerateError("weierstrass.c handles a = -3 and a = 0")
        on_curve = gy * gy - gx ** 3 - a * gx - b
    if gy and on_curve % fp.p:
        raise GenerateError("the generator is not on the curve")
    if kind == "edwards":
        return curves.EdwardsCurve(up, field, a, b, cof, order, gx, gy, fp)
    return curves.WeierstrassCurve(up, field, a, b, order, gx, gy, fp)


def _curve_record(c, kind, a, b, cof, fp) -> dict:
    return {"curve": c.name, "kind": kind, "field": c.field, "a": a, "b": hex(b) if b >= 0 else "-" + hex(-b), "order": hex(c.order), "cof": cof,
            "gx": hex(c.gx), "gy": hex(c.gy), "nlimbs": fp.nlimbs, "nbytes": fp.nbytes}


def generate_curve(name: str, kind: str, field: str, a: int, b: int, order: int, gx: int, gy: int, cof: int = 0,
                   plugin_dir: Optional[str] = None, force: bool = False, verbose: bool = False, wl: int = 64, emit_only: bool = False,
                   mul_wps: Optional[int] = None) -> GeneratedCurve:
    """The curve layer (curve.h: ecn_<name>_mul / mul2 / add / dbl / set / get ..., scalar and batched) for a curve that is not in
    curve.py's table.  kind "edwards": a x^2 + y^2 = 1 + b x^2 y^2 with a = +-1 (edwards.c; cof = log2 of the cofactor);
    kind "weierstrass": y^2 = x^3 + a x + b with a = -3 or 0 and prime order (weierstrass.c).  `field`: a built-in prime name or the
    tag of a generated field (generate() first).  One hipcc unit (the scalar-multiplication kernels take about a minute to
    compile); the plug-in exports what MODARITH_AMD_DECLARE_EDWARDS(<lower-case name>, Nlimbs) declares.
    wl=32: the same curve on uint32_t points (`curve.py 32 <CURVE>`), see _generate_curve_w32; emit_only and mul_wps belong to it."""
    if wl not in (64, 32):
        raise GenerateError("word length must be 64 or 32")
    if wl == 64 and (emit_only or mul_wps is not None):
        raise GenerateError("emit_only and mul_wps belong to the 32-bit word form (wl=32)")
    if kind not in ("edwards", "weierstrass"):
        raise GenerateError("kind must be 'edwards' or 'weierstrass'")
    if wl == 32:
        return _generate_curve_w32(name, kind, field, a, b, order, gx, gy, cof, plugin_dir, force, verbose, emit_only, mul_wps)
    from . import _lib
    if not _TAG_RE.match(name) or not name[0].isalpha():
        raise GenerateError("%r cannot be part of a C identifier" % (name,))
    up, low = name.upper(), name.lower()
    if low in _lib.CURVES:
        raise GenerateError("%s is a built-in curve" % up)
    d = plugin_dir or PLUGIN_DIR
    found = find_field(field, d)
    if found is None:
        raise GenerateError("field %r is neither built in nor generated: run generate() for it first" % (field,))
    fp = found[0]
    c = _curve_definition(kind, up, field, a, b, order, gx, gy, cof, fp)
    if kind == "edwards":
        hdr_text, cls, inc = emit.curve_header_text_of(c), "ma::Edwards<ma::C_%s>" % up, "edwards.h"
    else:
        hdr_text, cls, inc = emit.wcurve_header_text_of(c), "ma::Weierstrass<ma::C_%s>" % up, "weierstrass.h"
    unit_text = ("// GENERATED by modarith_amd/generate.py -- do not edit.  C-ABI of the curve layer for %s (%s over %s); body: csrc/capi_curve.inc\n"
                 '#include "modarith_amd.h"\nextern "C" {\nMODARITH_AMD_DECLARE_EDWARDS(%s, %d)\n}\n#include "curve_%s.h"\n#include "%s"\n'
                 "#define MA_CURVE_CLASS %s\n#define MA_CNAME %s\n#include \"capi_curve.inc\"\n" % (up, kind, field, low, fp.nlimbs, up, inc, cls, low))
    os.makedirs(d, exist_ok=True)
    unit, lib, meta = os.path.join(d, "capi_curve_%s.hip" % up), curve_plugin_path(up, d), os.path.join(d, "curve_%s.json" % up)
    emit._write(os.path.join(d, "curve_%s.h" % up), hdr_text)
    emit._write(unit, unit_text)
    built = build_plugin(d, lib, meta, _curve_record(c, kind, a, b, cof, fp), key_of(hdr_text, unit_text, emit.header_text(fp)),
                         [(unit, os.path.join(d, "capi_curve_%s.o" % up), [])], "curve", force, verbose, error=GenerateError)
    return GeneratedCurve(up, kind, field, lib, fp.nlimbs, fp.nbytes, built)


def _w32_curve_field(field: str, d: str):
    """the field of a 32-bit curve -> (FieldParams, header to include, generate_w32 argument or None): a built-in 32-bit prime, the
    tag of a generate_w32 plug-in (next to the curve or in the default directory), or a named prime, which is then generated"""
    from . import _lib
    found = find_field(field, d, 32)
    if found is not None:
        fp, where = found
        if where is None:
            return fp, "w32_%s.h" % field, None
        meta = json.load(open(_meta_path(field, where, 32)))
        # (the prime as it was given: a second process generating the same curve reaches the same up-to-date field plug-in)
        return fp, "params_%s_w32.h" % field, (meta.get("prime", field), meta["family"], meta["radix"], where)
    if field in NAMED:
        return resolve(field, wl=32), "params_%s_w32.h" % field, (field, None, None, d)
    raise GenerateError("field %r is neither built in at word length 32 (%s), nor generated there, nor a named prime: run generate_w32() for it first"
                        % (field, ", ".join(_lib.W32_PRIMES)))


def _generate_curve_w32(name, kind, field, a, b, order, gx, gy, cof, plugin_dir, force, verbose, emit_only, mul_wps) -> GeneratedCurve:
    """generate_curve() at word length 32: `python curve.py 32 <CURVE>`.  The field is a built-in 32-bit prime, the tag of a generate_w32
    plug-in, or a named prime (generated first, in the same call).  Emits, next to each other in the plug-in directory,
    w32_curve_<CURVE>.h (emit.w32_curve_header_text_of: struct ma32::C_<CURVE>_W32), capi_curve_<CURVE>_w32.hip (the lines of
    csrc/capi_ED25519_w32_ecn.hip, MA_MUL_WPS chosen by emit.w32_curve_mul_wps), libmodarith_amd_curve_<c>_w32.so and
    curve_<CURVE>_w32.json ("wl": 32).  The unit is compiled as its three MA_CURVE_PART objects, concurrently (the two
    scalar-multiplication kernels take about half a minute each), and linked into one library that exports what
    MODARITH_AMD_DECLARE_W32_CURVE(<c>, Nlimbs) declares; `Curve("<CURVE>", wl=32)` loads it.  A name is refused only where it is built in
    at THIS word length (ED25519, NIST256, ED448).  emit_only: write the texts and return without calling the compiler."""
    if not _TAG_RE.match(name) or not name[0].isalpha() or name.lower().endswith("_w32"):
        raise GenerateError("%r cannot name a curve (a C identifier that does not end in _w32, the suffix of this word length's files)" % (name,))
    up = name.upper()
    if up in emit.W32_CURVES:
        raise GenerateError("%s is a built-in curve at word length 32" % up)
    d = plugin_dir or PLUGIN_DIR
    fp, field_inc, field_gen = _w32_curve_field(field, d)
    if fp.nlimbs > emit.MAX_GENERATED_LIMBS_W32:
        raise GenerateError("%d limbs: the 32-bit kernels are built for at most %d limbs" % (fp.nlimbs, emit.MAX_GENERATED_LIMBS_W32))
    c = _curve_definition(kind, up, field, a, b, order, gx, gy, cof, fp)
    wps = mul_wps or emit.w32_curve_mul_wps(fp.nlimbs, fp.montgomery, kind)
    if wps not in (1, 2, 3, 4):
        raise GenerateError("MA_MUL_WPS is 1 to 4 resident waves per SIMD")
    hdr_text = emit.w32_curve_header_text_of(c, include=field_inc)
    unit_text = emit.w32_curve_unit_text(up, kind, field, fp.nlimbs, fp.montgomery, wps)
    field_text = emit.header_text(fp, generated=field_gen is not None)
    os.makedirs(d, exist_ok=True)
    stem = "%s_w32" % up
    unit, lib, meta = os.path.join(d, "capi_curve_%s.hip" % stem), curve_plugin_path(up, d, 32), os.path.join(d, "curve_%s.json" % stem)
    out = GeneratedCurve(up, kind, field, lib, fp.nlimbs, fp.nbytes, False)
    emit._write(os.path.join(d, "w32_curve_%s.h" % up), hdr_text)
    emit._write(unit, unit_text)
    if field_gen is not None and field_gen[3] == d:
        emit._write(os.path.join(d, "params_%s_w32.h" % field), field_text)      # (what generate_w32 writes: the curve parts compile beside it)
    if emit_only:
        return out
    jobs = []
    if field_gen is not None and not os.path.exists(plugin_path(field, field_gen[3], 32)):
        # the field's plug-in is not there yet: it is generated beside the curve's parts, and the curve is built whatever its metadata says
        jobs = [lambda: generate_w32(field_gen[0], family=field_gen[1], name=field, radix=field_gen[2], plugin_dir=field_gen[3], verbose=verbose)]
    record = dict(_curve_record(c, kind, a, b, cof, fp), wl=32, radix=fp.radix, family=fp.family, mul_wps=wps)
    units = [(unit, os.path.join(d, "capi_curve_%s_ecn_%s.o" % (stem, nm)), ["-DMA_CURVE_PART=%d" % part]) for part, nm in ((1, "mul"), (2, "mul2"), (3, "rest"))]
    out.built = build_plugin(d, lib, meta, record, key_of(hdr_text, unit_text, field_text), units, "curve", force or bool(jobs), verbose, jobs, GenerateError)
    return out


def named_curve(name: str) -> dict:
    """the constants of a curve of curve.py's table (modarith_amd.curves) as generate_curve's arguments"""
    from . import curves
    up = name.upper()
    if up in curves.CURVES:
        c = curves.CURVES[up]
        return dict(name=up, kind="edwards", field=c.field, a=c.a, b=c.d, order=c.order, gx=c.gx, gy=c.gy, cof=c.cof)
    if up in curves.W_CURVES:
        c = curves.W_CURVES[up]
        return dict(name=up, kind="weierstrass", field=c.field, a=c.a, b=c.b, order=c.order, gx=c.gx, gy=c.gy)
    raise GenerateError("%s is not in the curve table (%s)" % (up, ", ".join(list(curves.CURVES) + list(curves.W_CURVES))))


def generate_named_curve(name: str, wl: int = 32, **kw) -> GeneratedCurve:
    """generate_curve() for a curve of curve.py's table: generate_named_curve("NIST384", wl=32) is `python curve.py 32 NIST384`.  (At word
    length 64 all eleven are built in, and at 32 ED25519, NIST256 and ED448 are: those are refused as generate_curve refuses them.)"""
    return generate_curve(wl=wl, **named_curve(name), **kw)


# ---------------------------------------------------------------------------------------------------------------------
# Montgomery ladders of one's own: rfc7748.c describes its curve in an #ifdef block (A24, COF, GENERATOR, TWIST_SECURE; rfc7748.c:118-132)
# and is otherwise generic over the pasted field; this is that block for a curve other than X25519 / X448
def ladder_plugin_path(name: str, plugin_dir: Optional[str] = None) -> str:
    return os.path.join(plugin_dir or PLUGIN_DIR, "libmodarith_amd_ladder_%s.so" % name)


def generate_ladder(name: str, field: str, a24: int, cof: int, twist_secure: bool = True, plugin_dir: Optional[str] = None,
                    force: bool = False, verbose: bool = False) -> str:
    """`rfc7748_<name>(bk, bu, bv)` and `rfc7748_<name>_batch(bk, bu, bv, n, stream)` for the Montgomery curve
    v^2 = u^3 + A u^2 + u with (A - 2) / 4 = a24 over a built-in or generated field, cofactor 2^cof (2 or 3): the reference's
    rfc7748() call for call on the bit-exact field (csrc/ladder.h k_rfc7748: clamp, 5 M + 4 S + a24 per bit, generic=False sums,
    modpro + modinv, little-endian Nbytes records).  Only the TWIST_SECURE branch of rfc7748.c:224-227 is built; records move as
    64-bit words, so Nbytes must be a multiple of 8.  Returns the plug-in's path."""
    from . import _lib
    if not _TAG_RE.match(name) or name in _lib.LADDERS:
        raise GenerateError("%r: not a usable name (X25519 and X448 are built in)" % (name,))
    if not twist_secure:
        raise GenerateError("only the TWIST_SECURE form of rfc7748() is built (rfc7748.c:224-227); the point-validation branch is not")
    if cof not in (2, 3):
        raise GenerateError("COF is 2 or 3 (rfc7748.c:122)")
    if not 0 < a24 < (1 << 28):
        raise GenerateError("A24 must be a small positive integer: it is the `int` of modmli (rfc7748.c:209)")
    d = plugin_dir or PLUGIN_DIR
    found = find_field(field, d)
    if found is None:
        raise GenerateError("field %r is neither built in nor generated: run generate() for it first" % (field,))
    fp = found[0]
    if fp.nbytes % 8:
        raise GenerateError("%d-byte records: the ladder kernel moves records as 64-bit words" % fp.nbytes)
    sym = "rfc7748_%s" % name
    unit_text = "\n".join([
        "// GENERATED by modarith_amd/generate.py -- do not edit.  rfc7748() for the Montgomery curve %s: A24 = %d, COF = %d, over %s" % (name, a24, cof, field),
        '#include "params_%s.h"' % field, '#include "modarith_amd.h"', '#include "capi_common.h"', '#include "kernels.h"', '#include "ladder.h"', "",
        "namespace {", "using namespace ma;", "using P = ma::P_%s;" % field, "constexpr int NB = P::NBYTES;", "}", "",
        'extern "C" int %s_batch(const char* bk, const char* bu, char* bv, size_t n, void* st) {' % sym,
        "    if (n == 0) return 0;",
        "    if ((reinterpret_cast<uintptr_t>(bk) | reinterpret_cast<uintptr_t>(bu) | reinterpret_cast<uintptr_t>(bv)) & 7u) {",
        '        set_error("%s: byte records must be 8-byte aligned");' % sym,
        "        return (int)hipErrorInvalidValue;",
        "    }",
        "    const int block = ladder_block();",
        "    k_rfc7748<P, %d, %d><<<grid_for(n, block), block, 0, (hipStream_t)st>>>(" % (a24, cof),
        "        reinterpret_cast<const spint*>(bk), reinterpret_cast<const spint*>(bu), reinterpret_cast<spint*>(bv), n);",
        '    return check_launch("%s");' % sym,
        "}",
        "// the reference's own signature (rfc7748.c:156), host pointers: one record through the staging buffer",
        'extern "C" void %s(const char* bk, const char* bu, char* bv) {' % sym,
        "    StageBase s;                   // failures are recorded (modarith_amd_status()), never fatal; bv is zero-filled then",
        "    char *dk = (char*)s.take(NB), *du = (char*)s.take(NB), *dv = (char*)s.take(NB);",
        "    s.h2d(dk, bk, NB);",
        "    s.h2d(du, bu, NB);",
        '    if (!s.bad) s.check(%s_batch(dk, du, dv, 1, nullptr), "%s");' % (sym, sym),
        "    s.d2h(bv, dv, NB);",
        "}", ""])
    os.makedirs(d, exist_ok=True)
    unit, lib = os.path.join(d, "capi_ladder_%s.hip" % name), ladder_plugin_path(name, d)
    emit._write(unit, unit_text)
    build_plugin(d, lib, os.path.join(d, "ladder_%s.json" % name), {"ladder": name, "field": field, "a24": a24, "cof": cof, "nbytes": fp.nbytes, "nbits": fp.n},
                 key_of(unit_text, emit.header_text(fp)), [(unit, os.path.join(d, "capi_ladder_%s.o" % name), [])], "ladder", force, verbose, error=GenerateError)
    return lib


# ladders the test-suite generates: M-383 (Aranha-Barreto-Pereira-Ricardini: v^2 = u^3 + 2065150 u^2 + u over 2^383 - 187, the
# built-in PM383 field; base point u = 12) and a ladder over the GENERATED field 2^251 - 9 (A = 49382: a test curve -- the ladder
# is algebra on (A - 2) / 4 and is checked against plain integer arithmetic, whatever the curve's group looks like)
EXAMPLE_LADDERS = (dict(name="M383", field="PM383", a24=516287, cof=3), dict(name="T2519", field="2519", a24=12345, cof=3))


def _scan(plugin_dir: Optional[str], prefix: str, lib_of):
    """the metadata <prefix><X>.json of every plug-in of the directory whose shared object lib_of(<X>, directory) is present"""
    d = plugin_dir or PLUGIN_DIR
    for f in sorted(os.listdir(d)) if os.path.isdir(d) else []:
        if f.startswith(prefix) and f.endswith(".json") and os.path.exists(lib_of(f[len(prefix):-5], d)):
            try:
                yield json.load(open(os.path.join(d, f)))
            except ValueError:
                continue


def installed_curves(plugin_dir: Optional[str] = None, wl: int = 64) -> List[dict]:
    """metadata of every curve plug-in of word length wl whose shared object is present (curve_<CURVE>.json; 32: curve_<CURVE>_w32.json)"""
    return [m for m in _scan(plugin_dir, "curve_", curve_plugin_path) if m.get("wl", 64) == wl]


# curves the test-suite generates: Curve1174 (Bernstein-Hamburg-Krasnova-Lange: x^2 + y^2 = 1 - 1174 x^2 y^2 over 2^251 - 9, the generated
# field 2519) and NIST P-224 (a = -3 over the built-in NIST224 field) -- neither is in curve.py's table; the reference's own
# edwards.c / weierstrass.c, given the same definitions the way curve.py asks its user to insert them, produced
# tests/golden/curveref_CURVE1174.json / curveref_NIST224.json
EXAMPLE_CURVES = (
    dict(name="CURVE1174", kind="edwards", field="2519", a=1, b=-1174, cof=2,
         order=2**249 - 11332719920821432534773113288178349711,
         gx=1582619097725911541954547006453739763381091388846394833492296309729998839514,
         gy=3037538013604154504764115728651437646519513534305223422754827055689195992590),
    dict(name="NIST224", kind="weierstrass", field="NIST224", a=-3, b=0xb4050a850c04b3abf54132565044b0b7d7bfd8ba270b39432355ffb4,
         order=0xffffffffffffffffffffffffffff16a2e0b8f03e13dd29455c5c2a3d,
         gx=0xb70e0cbd6bb4bf7f321390b94a03c1d356c21122343280d6115c1d21, gy=0xbd376388b5f723fb4c22dfe6cd4375a05a07476444d5819985007e34),
)


def installed(plugin_dir: Optional[str] = None, wl: int = 64) -> List[dict]:
    """metadata of every field plug-in of word length wl whose shared object is present (64: the default; 32: generate_w32's, whose
    <TAG>_w32.json sits next to libmodarith_amd_<TAG>_w32.so).  The directory also holds the plug-ins of curves, ladders and fused
    chains (modarith_amd/fuse.py): theirs have no "tag"."""
    return [m for m in _scan(plugin_dir, "", plugin_path) if "tag" in m and m.get("wl", 64) == wl]


def params_of_plugin(tag: str, plugin_dir: Optional[str] = None, wl: int = 64) -> FieldParams:
    """FieldParams of an installed plug-in, re-derived from its recorded modulus / family / radix"""
    meta = json.load(open(_meta_path(tag, plugin_dir, wl)))
    return (derive_pseudo if meta["family"] == "pseudo" else derive_monty)(tag, int(meta["p"], 16), meta["radix"], wl)


def report(fp: FieldParams) -> str:
    """the lines the reference generators print about their choice (pseudo.py:1600-1612, monty.py:2200-2230), for the CLI"""
    L = ["Chosen radix is %d bits, using %d limbs with excess of %d bits" % (fp.radix, fp.nlimbs, fp.xcess)]
    if fp.family == "pseudo":
        L.append("pseudo-Mersenne 2^%d - %d: fold constant mm = %#x%s%s%s%s" % (fp.n, fp.m, fp.mm, ", overflow form" if fp.overflow else "",
                                                                             ", tighter reduction" if fp.fred else "", ", EPM" if fp.epm else "",
                                                                             ", carry_on" if fp.carry_on else ""))
    else:
        L.append("Montgomery form, R = 2^%d%s, ndash = %#x%s%s" % (fp.radix * (fp.nlimbs + (1 if fp.E else 0)), " (virtual limb)" if fp.E else "", fp.ndash,
                                                                  ", trinomial" if fp.trin else "", ", exploitable pseudo-Mersenne (PM)" if fp.pm else ""))
        L.append("prime limbs: " + " ".join(("%d" % v) if abs(v) < 10 else ("%#x" % v) for v in fp.ppw))
    L.append("split products: %s; inversion chain: 2-adicity %d" % ("cut at bit %d" % emit.split_point(fp) if emit.split_point(fp) else "exact 128-bit products only", fp.pm1d2))
    return "\n".join(L)


def time_report(tag: str, outer: int = 100000, lanes: int = 1 << 16) -> List[str]:
    """What the generators do last: build time.c and run it (pseudo.py:1861-1925, monty.py:2440-2500) -- seed-42 operands,
    `outer` x 1000 dependent modmul, the same number of modsqr, `outer` / 2 x 2... modinv, the 24-bit check word of each.  Here the
    chains run on the GPU, one per lane (csrc/kernels.h k_time): the words are the reference's for outer = 100000 (its own depth);
    the times are per dependent operation in one wave (latency-bound) and the rate with `lanes` chains in flight."""
    import random
    import time

    import torch
    from .field import Field
    F = Field(tag)
    fp = F.params
    random.seed(42)                                              # pseudo.py:1862-1866
    ra, rb, rs, ri = (random.randint(0, fp.p - 1) for _ in range(4))
    mk = lambda v: [(v >> (fp.radix * i)) & ((1 << fp.radix) - 1) for i in range(fp.nlimbs)]      # makebig: every limb masked
    out = []
    for leg, x, y, nops in (("modmul", ra, rb, outer * 1000), ("modsqr", rs, None, outer * 1000), ("modinv", ri, None, max(1, outer // 2) * 2)):
        o = outer if leg != "modinv" else max(1, outer // 2)
        res = {}
        for what, L in (("wave", 64), ("chip", lanes)):
            xa = F.from_limbs([mk(x)]).expand(-1, L).contiguous()
            ya = F.from_limbs([mk(y)]).expand(-1, L).contiguous() if y is not None else None
            F.time_protocol(leg, xa, ya, 1)
            torch.cuda.synchronize(F.device)
            t0 = time.perf_counter()
            z = F.time_protocol(leg, xa, ya, o)
            torch.cuda.synchronize(F.device)
            res[what] = time.perf_counter() - t0
            word = int(z[0, 0].item()) & 0xFFFFFF
        out.append("%s check 0x%06x Nanosecs= %d (one wave, per dependent call; %d calls)   %.3g %s/s with %d chains in flight"
                   % (leg, word, round(res["wave"] / nops * 1e9), nops, lanes * nops / res["chip"], leg, lanes))
    return out


def time_report_w32(tag: str, n: int = 1 << 20, launches: int = 10) -> List[str]:
    """--time at word length 32.  The time.c chains (k_time) are not built at this word length (W32_ABSENT: time_protocol), so this
    reports what the batched entry points do instead: elements per second of modmul, modsqr and modinv on n uniform elements, each the
    median of `launches` single launches timed by device events after three warm-up launches (docs/measurement.md)."""
    import statistics

    import torch
    from .field import Field
    F = Field(tag, wl=32)
    x, y, z = F.nres(F.uniform(n, array=1)), F.nres(F.uniform(n, array=2)), F.empty(n)
    out = []
    for leg, call in (("modmul", lambda: F.modmul(x, y, out=z)), ("modsqr", lambda: F.modsqr(x, out=z)), ("modinv", lambda: F.modinv(x, out=z))):
        for _ in range(3):
            call()
        torch.cuda.synchronize(F.device)
        ev = []
        for _ in range(launches):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            ev.append((e0, e1))
        torch.cuda.synchronize(F.device)
        ms = statistics.median(e0.elapsed_time(e1) for e0, e1 in ev)
        out.append("%s %.3g elements/s (%d elements, batched entry point, 32-bit words; median of %d launches by device events, %.3f ms)"
                   % (leg, n / (ms * 1e-3), n, launches, ms))
    return out


def main(argv: List[str]) -> int:
    args = [a for a in argv if not a.startswith("--")]
    if "--list" in argv:
        for m in installed():
            print("%-12s %-6s %2d x %2d bits  %s" % (m["tag"], m["family"], m["nlimbs"], m["radix"], m["prime"]))
        for m in installed(wl=32):
            print("%-12s %-6s %2d x %2d bits  %s   (32-bit words)" % (m["tag"], m["family"], m["nlimbs"], m["radix"], m["prime"]))
        for m in installed_curves():
            print("%-12s %-11s over %-8s a = %d, b = %s" % (m["curve"], m["kind"], m["field"], m["a"], m["b"]))
        for m in installed_curves(wl=32):
            print("%-12s %-11s over %-8s a = %d, b = %s   (32-bit words, %d limbs)" % (m["curve"], m["kind"], m["field"], m["a"], m["b"], m["nlimbs"]))
        for m in _scan(None, "ladder_", ladder_plugin_path):
            print("%-12s ladder      over %-8s A24 = %d, COF = %d" % (m["ladder"], m["field"], m["a24"], m["cof"]))
        return 0
    if args and args[0] == "ladder":
        # python -m modarith_amd.generate ladder <name> <field> <A24> <COF>
        if len(args) != 5:
            print("Valid syntax - python -m modarith_amd.generate ladder <name> <field> <A24> <COF>")
            return 2
        try:
            lib = generate_ladder(args[1], args[2], int(args[3], 0), int(args[4], 0), force="--force" in argv, verbose=True)
        except (GenerateError, ValueError) as e:
            print(e)
            return 2
        print("%s: void rfc7748_%s(const char *bk, const char *bu, char *bv); int rfc7748_%s_batch(bk, bu, bv, n, stream); rfc7748(%r, ...)" % (lib, args[1], args[1], args[1]))
        return 0
    if args and args[0] == "curve32":
        # python -m modarith_amd.generate curve32 <NAME>: a curve of curve.py's table on uint32_t points, the reference's `curve.py 32 <NAME>`
        if len(args) != 2:
            print("Valid syntax - python -m modarith_amd.generate curve32 <curve of the table> [--force]")
            return 2
        try:
            g = generate_named_curve(args[1], wl=32, force="--force" in argv, verbose=True)
        except (GenerateError, ValueError) as e:
            print(e)
            return 2
        print("%s %s: C-ABI ecn_%s_w32_* (MODARITH_AMD_DECLARE_W32_CURVE(%s, %d)); Curve(%r, wl=32)" % ("built" if g.built else "up to date:", g.lib, g.name.lower(), g.name.lower(), g.nlimbs, g.name))
        return 0
    if args and args[0] == "curve":
        # python -m modarith_amd.generate curve <NAME> edwards|weierstrass <field> <a> <b> <order> <gx> <gy> [cof]   (integers: any python literal)
        if len(args) not in (9, 10):
            print("Valid syntax - python -m modarith_amd.generate curve <name> edwards|weierstrass <field> <a> <b> <order> <gx> <gy> [log2 cofactor]")
            return 2
        try:
            nums = [int(v, 0) for v in args[4:]]
            g = generate_curve(args[1], args[2], args[3], nums[0], nums[1], nums[2], nums[3], nums[4], nums[5] if len(nums) > 5 else 0,
                               force="--force" in argv, verbose=True)
        except (GenerateError, ValueError) as e:
            print(e)
            return 2
        print("%s %s: C-ABI ecn_%s_* (MODARITH_AMD_DECLARE_EDWARDS(%s, %d)); Curve(%r)" % ("built" if g.built else "up to date:", g.lib, g.name.lower(), g.name.lower(), g.nlimbs, g.name))
        return 0
    if len(args) != 2:
        print("Syntax error")
        print("Valid syntax - python -m modarith_amd.generate <word length> <prime> OR <prime name> OR <name>=<prime> [--pseudo|--monty] [--force] [--time[=outer]]")
        print("               python -m modarith_amd.generate w32 <prime> ... (the 32-bit word form)")
        print("For example - python -m modarith_amd.generate 64 2**255-19")
        return 2
    fam = "pseudo" if "--pseudo" in argv else "monty" if "--monty" in argv else None
    if args[0] == "w32":
        # python -m modarith_amd.generate w32 <prime> [--monty|--pseudo] [--time]: the reference's `pseudo.py 32 <prime>` / `monty.py 32 <prime>`
        try:
            g = generate_w32(args[1], family=fam, force="--force" in argv, verbose=True)
        except GenerateError as e:
            print(e)
            return 2
        print(report(g.params))
        from .params import w32_inv_closure
        c = w32_inv_closure(g.params)
        print("launch width: at most %d elements per lane; shared inversion: %s" % (emit.w32_ept_max(g.params.nlimbs),
              "closure shown (columns below 2^%.2f)" % c["column_bits"] if c["closed"] else "closure not shown (%s), one inversion per element" % c["why"]))
        if any(a == "--time" or a.startswith("--time=") for a in argv):
            for line in time_report_w32(g.tag):
                print(line)
        print("%s %s: C-ABI <fn>_%s_w32_ct / <fn>_%s_w32_batch (MODARITH_AMD_DECLARE_W32(%s)); Field(%r, wl=32)" % ("built" if g.built else "up to date:", g.lib, g.tag, g.tag, g.tag, g.tag))
        return 0
    try:
        g = generate(args[1], int(args[0]), family=fam, force="--force" in argv, verbose=True)
    except GenerateError as e:
        print(e)
        return 2
    print(report(g.params))
    for a in argv:
        if a == "--time" or a.startswith("--time="):
            for line in time_report(g.tag, int(a.split("=", 1)[1]) if "=" in a else 100000):
                print(line)
    print("%s %s: C-ABI <fn>_%s_ct / <fn>_%s_batch (MODARITH_AMD_DECLARE(%s)); Field(%r)" % ("built" if g.built else "up to date:", g.lib, g.tag, g.tag, g.tag, g.tag))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
