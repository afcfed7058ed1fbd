"""modarith_amd.hash -- batched SHA-2, SHA-3 and SHAKE on the device (include/modarith_amd_hash.h, csrc/hash.h).

    digest = shake256([dom4, R, A, M], 114, lens=[None, None, None, mlen])      # uint8 [n, 114], one record per lane

A record is the concatenation of its parts.  A part is a torch.uint8 tensor [n, L] on the device (its row stride is taken from the
tensor, so a column slice of a wider array or an expand()ed row is passed as it is, no copy), or a bytes object (uploaded once per
call, shared by the whole batch: stride 0).  `lens` holds, per part, None or a torch.int32 tensor [n] of per-record lengths; a length
above the part's width is clamped to it.  The functions return torch.uint8 [n, digest bytes] on the device (or fill `out`).

There is no CPU path: without the HIP library, loading raises (modarith_amd._lib).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib

__all__ = ["sha256", "sha384", "sha512", "sha3", "shake128", "shake256"]


def _stream(device) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def _marshal(parts, lens):
    """-> (ctypes array of ma_hash_part, n, device, tensors to keep alive until the launch is enqueued)"""
    if isinstance(parts, (torch.Tensor, bytes, bytearray)):
        parts = [parts]
    parts = list(parts)
    if not 1 <= len(parts) <= 8:
        raise ValueError("a record has 1 to 8 parts")
    lens = [None] * len(parts) if lens is None else list(lens)
    if len(lens) != len(parts):
        raise ValueError("lens needs one entry (a tensor or None) per part")
    tensors = [p for p in parts if isinstance(p, torch.Tensor)]
    if not tensors:
        raise ValueError("at least one part must be a device tensor [n, L]: it gives the batch size")
    dev, n = tensors[0].device, tensors[0].shape[0]
    arr = (_lib.HashPart * len(parts))()
    keep = []
    for k, (p, ln) in enumerate(zip(parts, lens)):
        if isinstance(p, (bytes, bytearray)):
            if ln is not None:
                raise ValueError("a shared bytes part takes no per-record lengths")
            t = torch.frombuffer(bytearray(p), dtype=torch.uint8).to(dev) if len(p) else torch.empty(0, dtype=torch.uint8, device=dev)
            keep.append(t)
            arr[k].ptr, arr[k].stride, arr[k].lens, arr[k].len = (t.data_ptr() or None), 0, None, len(p)
            continue
        if p.dtype != torch.uint8 or p.dim() != 2 or p.device != dev or p.device.type != "cuda":
            raise ValueError("part %d: expected a torch.uint8 tensor [n, L] on one cuda device" % k)
        if p.shape[0] != n:
            raise ValueError("part %d has %d rows, part 0 has %d" % (k, p.shape[0], n))
        if p.shape[1] > 1 and p.stride(1) != 1:
            raise ValueError("part %d: the bytes of a row must be contiguous (stride(1) == 1)" % k)
        if p.shape[1] >= 1 << 32:
            raise ValueError("part %d: a record must stay below 2^32 bytes" % k)
        arr[k].ptr, arr[k].stride, arr[k].len = (p.data_ptr() or None), (p.stride(0) if n > 1 else 0), p.shape[1]
        if ln is not None:
            if ln.dtype != torch.int32 or ln.shape != (n,) or ln.device != dev or not ln.is_contiguous():
                raise ValueError("lens[%d]: expected a contiguous torch.int32 tensor [n] on the parts' device" % k)
            arr[k].lens = ln.data_ptr() or None
        else:
            arr[k].lens = None
    return arr, n, dev, keep


def _out(out, n, dlen, dev):
    if out is None:
        return torch.empty((n, dlen), dtype=torch.uint8, device=dev)
    if out.dtype != torch.uint8 or out.dim() != 2 or out.shape != (n, dlen) or out.device != dev or (dlen > 1 and out.stride(1) != 1) or (n > 1 and out.stride(0) < dlen):
        raise ValueError("out: expected torch.uint8 [%d, %d] on the parts' device, rows contiguous and not overlapping" % (n, dlen))
    return out


def _run(name, head, parts, lens, out, dlen, tail=()):
    lib = _lib.load()
    arr, n, dev, keep = _marshal(parts, lens)
    out = _out(out, n, dlen, dev)
    dstride = out.stride(0) if n > 1 else dlen
    with torch.cuda.device(dev):
        _lib.check(getattr(lib, name)(*head, arr, len(arr), out.data_ptr(), dstride, *tail, n, _stream(dev)), name)
    del keep
    return out


def sha256(parts, lens=None, out=None):
    """HASH256 of every record: uint8 [n, 32]"""
    return _run("HASH256_batch", (), parts, lens, out, 32)


def sha384(parts, lens=None, out=None):
    return _run("HASH384_batch", (), parts, lens, out, 48)


def sha512(parts, lens=None, out=None):
    return _run("HASH512_batch", (), parts, lens, out, 64)


def sha3(t, parts, lens=None, out=None):
    """SHA3-224 / 256 / 384 / 512 by digest bytes t = 28 / 32 / 48 / 64 (hash.h SHA3_HASH224 ...)"""
    if t not in (28, 32, 48, 64):
        raise ValueError("sha3: t must be 28, 32, 48 or 64")
    return _run("SHA3_hash_batch", (t,), parts, lens, out, t)


def shake128(parts, olen, lens=None, out=None):
    if olen < 1:
        raise ValueError("olen must be positive")
    return _run("SHA3_shake_batch", (16,), parts, lens, out, olen, tail=(olen,))


def shake256(parts, olen, lens=None, out=None):
    """SHAKE256 of every record, olen bytes each: what ed448.c's H() computes (ed448.c:107-117)"""
    if olen < 1:
        raise ValueError("olen must be positive")
    return _run("SHA3_shake_batch", (32,), parts, lens, out, olen, tail=(olen,))
