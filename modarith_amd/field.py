"""Host-side mirror of the reference's field API, batched: `Field("X25519").modmul(a, b)`.

Same function names, argument order and meaning as the generated field.c
(function list pseudo.py:1413-1445 / monty.py:1885-1918), with `spint x[Nlimbs]` widened to a batch:
a torch int64 tensor of shape [Nlimbs, n] resident in HBM (limb-interleaved SoA; int64 is only the
64-bit container, the limbs are unsigned; int32 for the 32-bit word form, `Field(prime, wl=32)`).  Every method launches hand-written HIP kernels through
the C-ABI of include/modarith_amd.h on torch's current stream; torch is used for device memory and
streams only.  As in the reference, outputs may alias inputs (`out=a`).

Conversions (`from_ints`, `to_ints`) are host-side helpers for tests and glue.
"""
from __future__ import annotations

import os

from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch

from . import _lib
from .params import FieldParams


def _stream(device=None) -> int:
    return torch.cuda.current_stream(device).cuda_stream


def normalise_device(device, current=None) -> torch.device:
    """the device an object is bound to, always WITH an index: None, "cuda", torch.device("cuda") and a bare integer all
    resolve to the calling thread's current device (torch.device("cuda") != torch.device("cuda:0"), so an index-less form
    stored verbatim would reject every tensor, including the ones the object allocates itself).  `current` overrides
    torch.cuda.current_device (CPU-side unit test)."""
    if isinstance(device, int):
        return torch.device("cuda", device)
    dev = torch.device(device) if device is not None else torch.device("cuda")
    if dev.type != "cuda":
        raise ValueError("modarith_amd objects are bound to a GPU (got device %r): there is no CPU path" % (device,))
    if dev.index is None:
        dev = torch.device("cuda", (current or torch.cuda.current_device)())
    return dev


def tile_batch(t: torch.Tensor, tile: int = 4096) -> torch.Tensor:
    """flat batch [N, n] -> tiled batch [n / tile, N, tile]: limb i of element j moves from buf[i*n + j] to
    buf[((j // tile)*N + i)*tile + j % tile] (include/modarith_amd.h "TILED").  A copy made with torch ops; any device."""
    if t.dim() != 2 or tile < 128 or tile & (tile - 1):
        raise ValueError("expected a flat batch [N, n] and a power-of-two tile >= 128")
    N, n = t.shape
    if n % tile:
        raise ValueError("n must be a multiple of the tile size")
    return t.reshape(N, n // tile, tile).permute(1, 0, 2).contiguous()


def flatten_batch(t: torch.Tensor) -> torch.Tensor:
    """tiled batch [ntiles, N, tile] -> flat batch [N, n] (a copy); flat batches pass through"""
    if t.dim() == 2:
        return t
    nt, N, tile = t.shape
    return t.permute(1, 0, 2).reshape(N, nt * tile).contiguous()


class Field:
    """Batched field arithmetic for one of the built primes (X25519, NIST256, X448, ...) or a generated one.

    Shape of the batches this object CREATES -- it depends on n (round 4; ADVICE of round 4: say so here):
      * `Field(prime)` / `Field(prime, tile=4096)`: a batch of n elements is TILED, a 3-D tensor [n / tile, N, tile], when it holds at
        least two whole tiles and n is a multiple of the tile (n >= 2 * tile and n % tile == 0); every other n gives the FLAT 2-D
        tensor [N, n].  So `uniform(8192)` is [2, N, 4096] and `uniform(8191)` is [N, 8191].
      * `Field(prime, tile=None)`: always flat [N, n] -- what a script that indexes `[limb, j]` or labels its numbers "flat" must ask for.
    Every method ACCEPTS both forms; `to_flat` / `to_tiled` convert; `creates_tiled(n)` tells which one n gets.

    Word length: `Field(prime, wl=32)` is the 32-bit word form of X25519, NIST256 and X448 (include/modarith_amd_w32.h: the limbs of
    the reference's `pseudo.py 32` / `monty.py 32`, 9 x 29, 9 x 29 and 16 x 28 bits) on torch.int32 tensors of the same shapes, or of
    a field generated at that word length (`Field.generate(prime, wl=32)`, modarith_amd.generate.generate_w32; up to 18 limbs).  It has
    every method of the 64-bit form except modmuls, the _lazy forms and time_protocol (NotImplementedError); modinv shares one
    inversion between up to 64 elements of a large batch as the 64-bit form does (same words as one inversion per element), and
    modarith_amd.fuse.Chain(prime, name, wl=32) fuses sequences of calls on such batches.  wl=64 is the default."""

    DEFAULT_TILE = 4096            # = modarith_amd_recommended_ld(n) for n >= 2 * 4096 (include/modarith_amd.h "TILED")

    def __init__(self, prime: str, device: Optional[torch.device] = None, tile: Optional[int] = DEFAULT_TILE, wl: int = 64,
                 plugin_dir: Optional[str] = None):
        self.lib = _lib.load()
        self.flib = self.lib                   # the library that holds this prime's entry points
        if wl not in (64, 32):
            raise ValueError("word length must be 64 or 32")
        self.wl = wl
        # the container of a limb (the limbs are unsigned), its numpy view, and what the entry points of this word length are called
        self.dtype, self._np, self._sfx = (torch.int64, np.uint64, "") if wl == 64 else (torch.int32, np.uint32, "_w32")
        # a built-in prime, or a field made by the generator mode (modarith_amd.generate: generate / generate_w32), whose kernels live in
        # a plug-in of their own; plugin_dir: where it was generated, if not the default directory (looked into after it, as for a curve's field)
        from . import generate as _gen
        builtin = _lib.PRIMES if wl == 64 else _lib.W32_PRIMES
        found = _gen.find_field(prime, plugin_dir, wl, built=True)
        if found is None and (prime[:1].isdigit() or "=" in prime):
            try:                                       # an expression ("2**251-9", "NAME=0x...") names the field by its tag
                prime = _gen.resolve(prime, wl=wl).name
                found = _gen.find_field(prime, plugin_dir, wl, built=True) if prime not in builtin else None
            except _gen.GenerateError:
                pass
        if found is None and wl == 32:
            raise ValueError("the 32-bit word form is built for %s and generated for %s (got %r): generate it with Field.generate(..., wl=32) "
                             "or `python -m modarith_amd.generate w32 <prime>`"
                             % (", ".join(builtin), ", ".join(m["tag"] for m in _gen.installed(plugin_dir, wl=32)) or "no other field yet", prime))
        if found is None:
            raise ValueError("prime %r is neither built in (%s) nor generated (%s); generate it with Field.generate(...) or "
                             "`python -m modarith_amd.generate 64 <prime>`"
                             % (prime, ", ".join(builtin), ", ".join(m["tag"] for m in _gen.installed()) or "none"))
        self.params: FieldParams = found[0]
        if found[1] is not None:
            self.flib = _lib.load_plugin(prime, _gen.plugin_path(prime, found[1], wl), wl=wl)
        self.prime = prime
        self.N = self.params.nlimbs
        self.radix = self.params.radix
        self.nbytes = self.params.nbytes
        self.device = normalise_device(device)
        # Layout of the batches this object CREATES (empty / uniform / from_limbs / modimp ...): tile = 2^k >= 128 (default
        # 4096, the recommended stride) = tiled [n / tile, N, tile] for every batch of at least two whole tiles (include/
        # modarith_amd.h "TILED": the fast layout, 0.82 against 0.70 of the HBM peak for flat rows); smaller batches, and sizes
        # that are not a multiple of the tile, are flat [N, n] (see creates_tiled).  tile = None or 0: always flat (the n-lane
        # form of the reference's SIMD layout; what the curve and byte-record APIs take).  Every method ACCEPTS both forms,
        # whatever this is set to; to_flat / to_tiled convert.
        tile = tile or None
        if tile is not None and (tile < 128 or tile & (tile - 1)):
            raise ValueError("tile must be a power of two >= 128")
        self.tile = tile

    @classmethod
    def generate(cls, prime: str, device: Optional[torch.device] = None, tile: Optional[int] = None, **kw) -> "Field":
        """the generator mode in one call: `Field.generate("2**251-9")` is `python pseudo.py 64 2**251-9` followed by loading
        what it built -- constants derived, kernels compiled for the prime (about ten seconds, reused afterwards), field bound.
        Keywords as modarith_amd.generate.generate (family=, name=, radix=, force=).  wl=32: generate_w32, the 32-bit word form
        (`python pseudo.py 32 ...`), bound as Field(tag, wl=32)."""
        from . import generate as _gen
        if kw.pop("wl", 64) == 32:
            return cls(_gen.generate_w32(prime, **kw).tag, device, tile, wl=32)
        return cls(_gen.generate(prime, **kw).tag, device, tile)

    # ------------------------------------------------------------------ buffers
    def recommended_tile(self, n: int) -> Optional[int]:
        """the tile size modarith_amd_recommended_ld_for(n, Nlimbs) names for a batch of n elements of this field (None: flat rows) --
        `Field(P, tile=Field(P).recommended_tile(n))`; the object's own default stays 4096 for every field"""
        t = int(self.lib.modarith_amd_recommended_ld_for(n, self.N))
        return t if t < n else None

    def creates_tiled(self, n: int) -> bool:
        """whether a batch of n elements made by this object is tiled: at least two whole tiles and nothing left over (a
        torch tensor of whole tiles cannot say how many elements of a partial last tile are meant; such sizes stay flat --
        the C ABI itself takes ceil(n / ld) tiles with an explicit n)"""
        return bool(self.tile) and n >= 2 * self.tile and n % self.tile == 0

    def empty(self, n: int) -> torch.Tensor:
        if self.creates_tiled(n):
            return torch.empty((n // self.tile, self.N, self.tile), dtype=self.dtype, device=self.device)
        return torch.empty((self.N, n), dtype=self.dtype, device=self.device)

    def to_tiled(self, t: torch.Tensor, tile: Optional[int] = None) -> torch.Tensor:
        """flat [N, n] -> tiled [n / tile, N, tile] (a copy; torch ops only)"""
        return tile_batch(t, tile or self.tile or 4096)

    def to_flat(self, t: torch.Tensor) -> torch.Tensor:
        """tiled [ntiles, N, tile] -> flat [N, n] (a copy); flat batches pass through"""
        return flatten_batch(t)

    def from_limbs(self, limbs: Sequence[Sequence[int]]) -> torch.Tensor:
        """list of per-element limb lists -> device batch [N, n] (tiled if this object creates tiled batches)."""
        arr = np.array(limbs, dtype=self._np).reshape(len(limbs), self.N).T.copy()
        t = torch.from_numpy(arr.view(np.int64 if self.wl == 64 else np.int32)).to(self.device)
        if self.creates_tiled(t.shape[1]):
            t = self.to_tiled(t)
        return t

    def to_limbs(self, t: torch.Tensor) -> List[List[int]]:
        arr = self.to_flat(t.detach()).cpu().numpy().view(self._np)
        return [[int(v) for v in arr[:, j]] for j in range(arr.shape[1])]

    def from_ints(self, xs: Iterable[int]) -> torch.Tensor:
        """plain integers -> limbs with the top limb unmasked (pseudo.py:1769-1775); NOT nres'd."""
        return self.from_limbs([self.params.to_limbs(int(x)) for x in xs])

    def to_ints(self, t: torch.Tensor) -> List[int]:
        return [self.params.from_limbs(l) for l in self.to_limbs(t)]

    def from_aos(self, aos: torch.Tensor) -> torch.Tensor:
        """element-major device array int64 [n, N] (`spint x[n][Nlimbs]`, how CPU callers of field.c hold
        elements) -> limb-interleaved batch [N, n], converted on the device."""
        if aos.dtype != self.dtype or aos.dim() != 2 or aos.shape[1] != self.N or not aos.is_cuda or not aos.is_contiguous():
            raise ValueError("expected a contiguous %s device tensor of shape [n, %d]" % (self.dtype, self.N))
        n = aos.shape[0]
        out = self.empty(n)
        _lib.check(self._util("aos_to_soa")(aos.data_ptr(), out.data_ptr(), n, self.N, max(self._ld(out), 1), _stream(self.device)), "aos_to_soa")
        return out

    def to_aos(self, soa: torch.Tensor) -> torch.Tensor:
        """limb-interleaved batch [N, n] -> element-major int64 [n, N], on the device."""
        n = self._chk(soa)
        out = torch.empty((n, self.N), dtype=self.dtype, device=soa.device)
        _lib.check(self._util("soa_to_aos")(soa.data_ptr(), out.data_ptr(), n, self.N, self._ld(soa), _stream(self.device)), "soa_to_aos")
        return out

    # ------------------------------------------------------------------ plumbing
    def _util(self, name: str):
        return getattr(self.lib, "modarith_amd%s_%s" % (self._sfx, name))

    def _absent(self, what: str):
        raise NotImplementedError("%s is not offered at word length %d (include/modarith_amd_w32.h); use Field(%r) for it" % (what, self.wl, self.prime))

    def _ld(self, t: torch.Tensor) -> int:
        """the limb stride argument of the C-ABI: the row stride of a flat batch, the tile size of a tiled one"""
        if t.dim() == 3:
            return t.shape[2]
        return t.stride(0) if t.shape[1] else 1

    def _chk(self, *ts: torch.Tensor) -> int:
        t0 = ts[0]
        if t0.dim() == 3:                                   # tiled [ntiles, N, tile]
            nt, N, tile = t0.shape
            if N != self.N or tile < 128 or tile & (tile - 1):
                raise ValueError("tiled batches have shape [ntiles, %d, tile] with tile a power of two >= 128" % self.N)
            for t in ts:
                if t.dtype != self.dtype or t.shape != t0.shape or not t.is_contiguous():
                    raise ValueError("all operands of one call must be contiguous %s tiled batches of one shape" % self.dtype)
                if not t.is_cuda:
                    raise ValueError("batches must live in device memory")
                if t.device != self.device:
                    raise ValueError("batch on %s, field bound to %s (kernels launch on the field's device)" % (t.device, self.device))
            return nt * tile
        n = t0.shape[1]
        for t in ts:
            if t.dtype != self.dtype or t.dim() != 2 or t.shape[0] != self.N or t.shape[1] != n:
                raise ValueError("expected %s tensors of shape [%d, n]" % (self.dtype, self.N))
            if not t.is_cuda:
                raise ValueError("batches must live in device memory")
            if t.device != self.device:
                raise ValueError("batch on %s, field bound to %s (kernels launch on the field's device)" % (t.device, self.device))
            if t.stride(1) != 1:
                raise ValueError("batches must be limb-major with unit element stride")
        ld = ts[0].stride(0) if n > 1 or ts[0].stride(0) >= 1 else n
        for t in ts:
            if t.stride(0) != ld:
                raise ValueError("all operands of one call must share the limb stride")
        if 1 < n and ld < n:
            raise ValueError("a flat batch needs a limb stride >= n")
        return n

    def _call(self, fn: str, *args):
        if self.wl == 32 and fn in _lib.W32_ABSENT:
            self._absent(fn)
        f = getattr(self.flib, "%s_%s%s_batch" % (fn, self.prime, self._sfx))
        with torch.cuda.device(self.device):          # the C-ABI launches on the calling thread's current device
            _lib.check(f(*args), "%s_%s%s_batch" % (fn, self.prime, self._sfx))

    def _out(self, like: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
        # a fresh result takes the operand's limb stride (views of wider batches keep theirs), as one call needs
        return out if out is not None else torch.empty_strided(like.shape, like.stride(), dtype=like.dtype, device=like.device)

    def _bin(self, fn, a, b, out):
        out = self._out(a, out)
        n = self._chk(a, b, out)
        self._call(fn, a.data_ptr(), b.data_ptr(), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def _un(self, fn, a, out):
        out = self._out(a, out)
        n = self._chk(a, out)
        self._call(fn, a.data_ptr(), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def _ints(self, n: int) -> torch.Tensor:
        return torch.empty(n, dtype=torch.int32, device=self.device)

    # ------------------------------------------------------------------ the field.c API, batched
    def modadd(self, a, b, out=None): return self._bin("modadd", a, b, out)
    def modsub(self, a, b, out=None): return self._bin("modsub", a, b, out)
    def modmul(self, a, b, out=None): return self._bin("modmul", a, b, out)
    def modadd_lazy(self, a, b, out=None): return self._bin("modadd_lazy", a, b, out)
    def modsub_lazy(self, a, b, out=None): return self._bin("modsub_lazy", a, b, out)
    def modneg(self, a, out=None): return self._un("modneg", a, out)
    def modneg_lazy(self, a, out=None): return self._un("modneg_lazy", a, out)
    def modsqr(self, a, out=None): return self._un("modsqr", a, out)
    def modcpy(self, a, out=None): return self._un("modcpy", a, out)
    def modpro(self, a, out=None): return self._un("modpro", a, out)
    def nres(self, a, out=None): return self._un("nres", a, out)
    def redc(self, a, out=None): return self._un("redc", a, out)

    def modmuls(self, a, b0: Sequence[int], out=None):
        """shared multiplicand: out[j] = a[j] * b0 (one element, limbs on the host)."""
        if self.wl == 32:
            self._absent("modmuls")
        out = self._out(a, out)
        n = self._chk(a, out)
        host = (_lib.ctypes.c_uint64 * self.N)(*[int(v) for v in b0])
        self._call("modmuls", a.data_ptr(), _lib.ctypes.cast(host, _lib.ctypes.c_void_p), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def modmli(self, a, b: int, out=None):
        out = self._out(a, out)
        n = self._chk(a, out)
        self._call("modmli", a.data_ptr(), int(b), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def modnsqr(self, a, k: int):
        n = self._chk(a)
        self._call("modnsqr", a.data_ptr(), int(k), n, self._ld(a), _stream(self.device))
        return a

    def modinv(self, x, h=None, out=None):
        out = self._out(x, out)
        n = self._chk(x, out) if h is None else self._chk(x, h, out)
        if h is None and out.data_ptr() == x.data_ptr() and n >= (4096 if self.wl == 64 else 32768):     # (32 768: where the 32-bit form starts sharing)
            # in place on a large batch: the simultaneous inversion needs n elements of scratch for its prefix products.  Taken from
            # torch's caching allocator here (visible to it, stream-ordered, reusable) rather than from the library's own pool:
            # the result is computed into a temporary and copied back (the kernel is VALU-bound; the copy is noise)
            tmp = torch.empty_like(x)
            self._call("modinv", x.data_ptr(), None, tmp.data_ptr(), n, self._ld(x), _stream(self.device))
            out.copy_(tmp)
            return out
        self._call("modinv", x.data_ptr(), None if h is None else h.data_ptr(), out.data_ptr(), n, self._ld(x), _stream(self.device))
        return out

    def modsqrt(self, x, h=None, out=None):
        out = self._out(x, out)
        n = self._chk(x, out) if h is None else self._chk(x, h, out)
        self._call("modsqrt", x.data_ptr(), None if h is None else h.data_ptr(), out.data_ptr(), n, self._ld(x), _stream(self.device))
        return out

    def modqr(self, h, x):
        """1 where x is a quadratic residue (or zero); h = optional progenitors modpro(x)."""
        n = self._chk(x) if h is None else self._chk(x, h)
        out = self._ints(n)
        self._call("modqr", None if h is None else h.data_ptr(), x.data_ptr(), out.data_ptr(), n, self._ld(x), _stream(self.device))
        return out

    def modfsb(self, a):
        """in place; returns the per-element flag (1 if the input was < p)."""
        n = self._chk(a)
        flag = self._ints(n)
        self._call("modfsb", a.data_ptr(), flag.data_ptr(), n, self._ld(a), _stream(self.device))
        return flag

    def flatten(self, a):
        n = self._chk(a)
        flag = self._ints(n)
        self._call("flatten", a.data_ptr(), flag.data_ptr(), n, self._ld(a), _stream(self.device))
        return flag

    def prop(self, a):
        """in place (pseudo.py:223-251); returns the per-element mask as int32: -1 where the top limb went negative, else 0."""
        n = self._chk(a)
        flag = self._ints(n)
        self._call("prop", a.data_ptr(), flag.data_ptr(), n, self._ld(a), _stream(self.device))
        return flag

    def modhaf(self, a):
        n = self._chk(a)
        self._call("modhaf", a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def modshl(self, k: int, a):
        n = self._chk(a)
        self._call("modshl", int(k), a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def modshr(self, k: int, a):
        n = self._chk(a)
        out = self._ints(n)
        self._call("modshr", int(k), a.data_ptr(), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def _pred(self, fn, a):
        n = self._chk(a)
        out = self._ints(n)
        self._call(fn, a.data_ptr(), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def modis1(self, a): return self._pred("modis1", a)
    def modis0(self, a): return self._pred("modis0", a)
    def modsign(self, a): return self._pred("modsign", a)

    def modlimbs(self, a):
        """1 per element whose limbs are all below 2^(Radix+2) (the limb budget of the generated functions), else 0"""
        return self._pred("modlimbs", a)

    def modcmp(self, a, b):
        n = self._chk(a, b)
        out = self._ints(n)
        self._call("modcmp", a.data_ptr(), b.data_ptr(), out.data_ptr(), n, self._ld(a), _stream(self.device))
        return out

    def modzer(self, n: int):
        a = self.empty(n)
        self._call("modzer", a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def modone(self, n: int):
        a = self.empty(n)
        self._call("modone", a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def modint(self, x: int, n: int):
        a = self.empty(n)
        self._call("modint", int(x), a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def mod2r(self, r: int, n: int):
        a = self.empty(n)
        self._call("mod2r", int(r), a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def uniform(self, n: int, seed: int = 42, array: int = 0, first: int = 0, plus_p: bool = False, out=None):
        """synthetic batch (SURVEY 8(d) input recipe): canonical limbs of values uniform in [0,p), element j drawn from the
        splitmix64 stream keyed by (seed, array) at position first+j; plus_p: the value + p with the top limb unmasked.
        Plain values (apply nres for Montgomery form)."""
        a = out if out is not None else self.empty(n)
        if out is not None and self._chk(out) != n:
            raise ValueError("out must hold n elements")
        self._call("moduniform", int(seed), int(array), int(first), int(bool(plus_p)), a.data_ptr(), n, self._ld(a), _stream(self.device))
        return a

    def _sel(self, d: torch.Tensor, n: int) -> torch.Tensor:
        if d.dtype != torch.int32 or d.numel() != n or not d.is_cuda or not d.is_contiguous():
            raise ValueError("selector must be a contiguous int32 device tensor with one 0/1 entry per element")
        return d

    def modcmv(self, d, g, f):
        """f[j] = g[j] where d[j] == 1 (constant time); d: int32 [n]."""
        n = self._chk(g, f)
        self._call("modcmv", self._sel(d, n).data_ptr(), g.data_ptr(), f.data_ptr(), n, self._ld(g), _stream(self.device))
        return f

    def modcsw(self, d, g, f):
        """swap g[j], f[j] where d[j] == 1 (constant time)."""
        n = self._chk(g, f)
        self._call("modcsw", self._sel(d, n).data_ptr(), g.data_ptr(), f.data_ptr(), n, self._ld(g), _stream(self.device))
        return g, f

    def time_protocol(self, kind: str, x, y=None, outer: int = 1):
        """The reference's time.c chains (pseudo.py:1177-1386) per lane, in registers: kind "modmul"
        (outer*1000 dependent modmul on x,y), "modsqr" (outer*1000 modsqr), "modinv" (outer*2 modinv).
        x, y: plain limbs (time.c applies nres itself).  Returns redc(z); z[0] & 0xFFFFFF is the check word."""
        if self.wl == 32:
            self._absent("time_protocol")
        k = {"modmul": 0, "modsqr": 1, "modinv": 2}[kind]
        y = x if y is None else y
        z = torch.empty_like(x)
        n = self._chk(x, y, z)
        self._call("time_protocol", k, x.data_ptr(), y.data_ptr(), z.data_ptr(), int(outer), n, self._ld(x), _stream(self.device))
        return z

    def modimp(self, b: torch.Tensor):
        """b: uint8 [n, Nbytes] big-endian records -> (batch, flag)."""
        if b.dtype != torch.uint8 or b.dim() != 2 or b.shape[1] != self.nbytes or not b.is_contiguous() or not b.is_cuda:
            raise ValueError("expected a contiguous uint8 device tensor [n, %d]" % self.nbytes)
        n = b.shape[0]
        a = self.empty(n)
        flag = self._ints(n)
        self._call("modimp", b.data_ptr(), a.data_ptr(), flag.data_ptr(), n, self._ld(a), _stream(self.device))
        return a, flag

    def modexp(self, a):
        n = self._chk(a)
        b = torch.empty((n, self.nbytes), dtype=torch.uint8, device=self.device)
        self._call("modexp", a.data_ptr(), b.data_ptr(), n, self._ld(a), _stream(self.device))
        return b


def rfc7748(curve: str, bk: torch.Tensor, bu: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Batched `rfc7748(bk, bu, bv)` (reference rfc7748.c:156): uint8 [n, Nbytes] RFC little-endian
    records in device memory -> uint8 [n, Nbytes].  `out` may be `bu`."""
    if curve not in _lib.LADDERS:
        return _rfc7748_generated(curve, bk, bu, out)
    lib = _lib.load()
    nb = 32 if curve == "X25519" else 56
    for t in (bk, bu):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != nb or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("expected contiguous uint8 device tensors [n, %d]" % nb)
    if bk.shape[0] != bu.shape[0]:
        raise ValueError("bk and bu must hold the same number of records")
    if bk.device != bu.device:
        raise ValueError("bk and bu must live on the same device")
    if out is None:
        out = torch.empty_like(bu)
    elif (out.dtype != torch.uint8 or out.shape != bu.shape or not out.is_contiguous() or out.device != bu.device):
        raise ValueError("out must be a contiguous uint8 tensor of shape %s on %s" % (tuple(bu.shape), bu.device))
    n = bk.shape[0]
    with torch.cuda.device(bu.device):
        st = torch.cuda.current_stream().cuda_stream
        if n >= 8192 and os.environ.get("MA_LADDER_SPLIT") != "0" and os.environ.get("MA_LADDER_IMPL") != "field":
            # split form (include/modarith_amd.h): ladders, then one inversion per up to 32 records; the scratch comes from
            # torch's caching allocator (stream-ordered, reused across calls, legal under graph capture)
            nbytes = getattr(lib, "rfc7748_%s_batch_workspace_bytes" % curve)(n)
            ws = torch.empty((nbytes + 7) // 8, dtype=torch.int64, device=bu.device)
            f = getattr(lib, "rfc7748_%s_batch_ws" % curve)
            _lib.check(f(bk.data_ptr(), bu.data_ptr(), out.data_ptr(), n, ws.data_ptr(), ws.numel() * 8, st), "rfc7748_%s_batch_ws" % curve)
        else:
            f = getattr(lib, "rfc7748_%s_batch" % curve)
            _lib.check(f(bk.data_ptr(), bu.data_ptr(), out.data_ptr(), n, st), "rfc7748_%s_batch" % curve)
    return out


_ladder_plugins = {}


def _rfc7748_generated(curve: str, bk: torch.Tensor, bu: torch.Tensor, out: Optional[torch.Tensor]) -> torch.Tensor:
    """rfc7748() of a Montgomery curve made by modarith_amd.generate.generate_ladder (the #ifdef block a user of rfc7748.c adds for
    a curve of their own, rfc7748.c:118-132)"""
    import ctypes
    import json
    from . import generate as _gen
    if curve not in _ladder_plugins:
        path = _gen.ladder_plugin_path(curve)
        meta = os.path.join(os.path.dirname(path), "ladder_%s.json" % curve)
        if not (os.path.exists(path) and os.path.exists(meta)):
            raise ValueError("curve must be one of %s or a ladder generated with modarith_amd.generate.generate_ladder" % (_lib.LADDERS,))
        m = json.load(open(meta))
        _lib.load()
        if m["field"] not in _lib.PRIMES:
            _lib.load_plugin(m["field"])
        lib = ctypes.CDLL(path)
        f = getattr(lib, "rfc7748_%s_batch" % curve)
        f.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_size_t, ctypes.c_void_p]
        f.restype = ctypes.c_int
        _ladder_plugins[curve] = (lib, f, m["nbytes"])
    _, f, nb = _ladder_plugins[curve]
    for t in (bk, bu):
        if t.dtype != torch.uint8 or t.dim() != 2 or t.shape[1] != nb or not t.is_contiguous() or not t.is_cuda:
            raise ValueError("expected contiguous uint8 device tensors [n, %d]" % nb)
    if bk.shape[0] != bu.shape[0] or bk.device != bu.device:
        raise ValueError("bk and bu must hold the same number of records on the same device")
    if out is None:
        out = torch.empty_like(bu)
    elif out.dtype != torch.uint8 or out.shape != bu.shape or not out.is_contiguous() or out.device != bu.device:
        raise ValueError("out must be a contiguous uint8 tensor of shape %s on %s" % (tuple(bu.shape), bu.device))
    with torch.cuda.device(bu.device):
        _lib.check(f(bk.data_ptr(), bu.data_ptr(), out.data_ptr(), bk.shape[0], torch.cuda.current_stream().cuda_stream), "rfc7748_%s_batch" % curve)
    return out


def rfc7748_base(curve: str, bk: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Batched `rfc7748(bk, base, bv)` (public-key generation, reference rfc7748.c:297-333): the same bytes as
    rfc7748(curve, bk, bu = base point u = 9 / 5), computed from a fixed-base table on the equivalent Edwards curve."""
    if curve not in _lib.LADDERS:
        raise ValueError("curve must be one of %s" % (_lib.LADDERS,))
    lib = _lib.load()
    nb = 32 if curve == "X25519" else 56
    if bk.dtype != torch.uint8 or bk.dim() != 2 or bk.shape[1] != nb or not bk.is_contiguous() or not bk.is_cuda:
        raise ValueError("expected a contiguous uint8 device tensor [n, %d]" % nb)
    if out is None:
        out = torch.empty_like(bk)
    elif (out.dtype != torch.uint8 or out.shape != bk.shape or not out.is_contiguous() or out.device != bk.device):
        raise ValueError("out must be a contiguous uint8 tensor of shape %s on %s" % (tuple(bk.shape), bk.device))
    f = getattr(lib, "rfc7748_%s_base_batch" % curve)
    with torch.cuda.device(bk.device):
        _lib.check(f(bk.data_ptr(), out.data_ptr(), bk.shape[0], torch.cuda.current_stream().cuda_stream), "rfc7748_%s_base_batch" % curve)
    return out
