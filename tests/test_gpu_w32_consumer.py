"""The paste-marker consumer over the 32-bit scalar ABI: examples/paste_marker_consumer.c built against include/field_X25519_w32.h
(-DFIELD_HEADER) must print the macro block of the 32-bit field.c, the RFC 7748 section 6.1 vector and the value of the reference's
chained-call loop after 10 steps (tests/golden/ladder_X25519.json ref_main_chain): these bytes do not depend on the word length, so
this is an end-to-end check of about 4 700 field calls per scalar multiplication through <fn>_X25519_w32_ct."""
import os
import subprocess

import pytest

from tests.conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_consumer_over_the_32_bit_shim_reproduces_the_reference(tmp_path):
    steps = 10
    g = load_golden("ladder_X25519.json")
    exe = str(tmp_path / "consumer_w32")
    cmd = ["gcc", "-O2", os.path.join(ROOT, "examples", "paste_marker_consumer.c"), '-DFIELD_HEADER="field_X25519_w32.h"', "-I" + os.path.join(ROOT, "include"),
           "-L" + os.path.join(ROOT, "modarith_amd"), "-l:libmodarith_amd.so", "-Wl,-rpath," + os.path.join(ROOT, "modarith_amd"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    p = subprocess.run([exe, str(steps)], capture_output=True, text=True, timeout=1500)
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
    out = dict(l.split(" ", 1) for l in p.stdout.strip().splitlines())
    assert out["field"] == "Wordlength 32 Nlimbs 9 Radix 29 Nbits 255 Nbytes 32 sizeof(spint) 4"
    assert out["vector"] == g["kat"][0]["out"]                                      # RFC 7748 6.1
    assert out["key"] == g["ref_main_chain"]["bk"] and out["steps"] == str(steps)
    assert out["chain"] == g["ref_main_chain"]["checkpoints"][str(steps)]
