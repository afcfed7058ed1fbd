"""The shared inversion (csrc/shared_inv.h) and its four item policies on the host, no GPU: tools/shared_inv_host.hip runs every lane of
small batches through the shared form and compares every output word with the unshared one (each item's own F::invert), with zero
denominators at the first, a middle, the last valid and all items of a column."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not os.path.exists(HIPCC) and shutil.which("hipcc") is None, reason="needs hipcc (host compile of the HIP headers)")


@needs_hipcc
@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "asan_ubsan"])
def test_shared_inversion_equals_the_unshared_form_on_host(tmp_path, sanitize):
    """fe26 / fe28 (k_fe_finish, k_fe_batch_div), fm26 / fk26 (k_wn_export) and fm26 (k_wn_table_affine, Jacobian and homogeneous):
    a zero item leaves as its caller's answer for zero -- 0; (0, 0); (0, 1); the entry's X, Y kept, flag set -- and every other item of
    its column exactly as if it were inverted alone.  Once as the kernels' own -O2 code, once under the address and undefined-behaviour
    sanitizers (every array is sized to its batch: an item that does not exist must not be touched)."""
    exe = str(tmp_path / "shared_inv_host")
    cc = HIPCC if os.path.exists(HIPCC) else "hipcc"
    flags = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else ["-O2"]
    subprocess.run([cc] + flags + ["-std=c++17", "-w", "--offload-host-only", os.path.join(ROOT, "tools", "shared_inv_host.hip"), "-o", exe],
                   check=True, timeout=900)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    lines = [l for l in p.stdout.splitlines() if "cases" in l]
    assert len(lines) == 6 and all(l.endswith(" 0 differ") for l in lines), p.stdout
