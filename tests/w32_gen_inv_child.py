"""The per-element side of tests/test_gpu_w32_gen.py test_shared_inversion_against_one_inversion_per_element.

The library reads MA_INV_SIMUL once per process, so "one inversion per element at every batch size" needs a process of its own:
  MA_INV_SIMUL=0 python -m tests.w32_gen_inv_child <TAG> <out.npy>
builds the batch below for the generated 32-bit field <TAG>, inverts it, saves the words and prints the launch name
(modarith_amd_last_launch).  The test builds the same batch in its own process and compares word for word.  TEST INFRASTRUCTURE ONLY."""
import sys

from tests import w32_gen_inputs as gi

N_INV = 32768 + 129


def inv_batch(torch, F, fp):
    """nres(uniform) with zeros, p, 2p and arbitrary-word elements scattered over lanes and rounds"""
    x = F.nres(F.uniform(N_INV, seed=77, array=3))
    N = fp.nlimbs
    sp = [gi.split(fp, 0), gi.split(fp, fp.p), gi.split(fp, 2 * fp.p), [gi.M32] * N, [1 << 31] * N, [(1 << (fp.radix + 2)) - 1] * N,
          [gi.M32 if i % 2 else 0 for i in range(N)], [(1 << fp.radix) - 1] * (N - 1) + [(1 << (fp.n + 1 - fp.radix * (N - 1))) - 1]]
    pos = list(range(11008, 11072))                                         # one whole wave of zero forms ...
    for k in range(160):                                                    # ... and the rest over lanes and rounds, no position twice
        q = (k * 1031 + (k // 5) * 64 + 7) % N_INV
        while q in pos:
            q = (q + 1) % N_INV
        pos.append(q)
    pos = pos[64:] + pos[:64]
    elems = [sp[k % len(sp)] for k in range(160)] + [sp[k % 3] for k in range(64)]
    idx = torch.tensor(pos, dtype=torch.int64, device=x.device)
    vals = torch.tensor([[v if v < (1 << 31) else v - (1 << 32) for v in e] for e in elems], dtype=torch.int32, device=x.device).T.contiguous()
    x[:, idx] = vals
    return x, dict(zip(pos, elems))


if __name__ == "__main__":
    import numpy as np
    import torch
    from modarith_amd import _lib
    from modarith_amd.field import Field
    tag, path = sys.argv[1], sys.argv[2]
    F = Field(tag, wl=32, tile=None)
    x, _ = inv_batch(torch, F, gi.params(tag))
    np.save(path, F.modinv(x).cpu().numpy())
    print(_lib.load().modarith_amd_last_launch().decode())
