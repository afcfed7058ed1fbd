// modarith_amd/csrc/capi_w32.inc -- per-prime body of the C-ABI shim of the 32-bit word form.  Included by capi_<PRIME>_w32.hip
// with MA_P (parameter struct, csrc/generated/w32_<PRIME>.h) and MA_NAME (token) defined.  Every entry point declared by
// MODARITH_AMD_DECLARE_W32(P) in include/modarith_amd_w32.h is defined here: <fn>_<PRIME>_w32_batch (device pointers, limb-
// interleaved uint32_t batches, argument order of the 64-bit _batch forms) and <fn>_<PRIME>_w32_ct (the reference's signatures over
// uint32_t, host pointers, one element through the device).
#include "../../include/modarith_amd_w32.h"
#include "capi_common.h"
#include "kernels32.h"
#include <string.h>
#include <algorithm>

#define MA_CAT4_(a, b, c, d) a##_##b##_##c##_##d
#define MA_CAT4(a, b, c, d) MA_CAT4_(a, b, c, d)
#define BATCH(fn) MA_CAT4(fn, MA_NAME, w32, batch)
#define SCALAR(fn) MA_CAT4(fn, MA_NAME, w32, ct)

namespace {
using namespace ma32;
using ma::check_launch;
using ma::grid_for;
using ma::set_error;
using ma::StageBase;
using P = MA_P;
constexpr int NL = P::N;
constexpr int NB = P::NBYTES;
// Launch shape of the streaming kernels (k_binary, k_unary, k_mli): elements per lane -- four (16 bytes, global_load/store_dwordx4),
// two (8 bytes) or one (4 bytes) -- and workgroup size.  Every width is compiled for every prime, none with scratch or accumulation
// registers (the widest: 95 VGPRs for the 9-limb modmul at four elements per lane, 163 for the 16-limb one).  The default is the
// MEASURED choice (tools/w32_rate.py, profiles/w32_rate.json, docs/kernels_field.md 4.5): on tiles of 4096 at 2^24 elements ONE
// element per lane in workgroups of 256 streamed best for modmul and modsqr of all three primes -- 0.79-0.82 of the HBM peak against
// 0.77-0.80 at two and 0.75-0.79 at four elements per lane -- so the wider accesses are kept as alternatives, not used by default.
// MA_W32_EPT=1|2|4 raises the widest access the library may take and MA_W32_BLOCK=64|128|256|512 sets the workgroup size, for the
// calls that follow (read at every call): testing and measuring knobs, like MA_FORCE_EXACT of the 64-bit form.  Same words on every path.
constexpr int EPT_DEFAULT = 1;
int ept_cap() {                  // (read at every call: tools/w32_rate.py measures the widths side by side in one process)
    const char* e = getenv("MA_W32_EPT");
    const int x = e ? atoi(e) : 0;
    return (x == 1 || x == 2 || x == 4) ? x : EPT_DEFAULT;
}

// workgroup size of the streaming kernels (MA_W32_BLOCK=64|128|256 overrides it for a process, like MA_W32_EPT)
constexpr int STREAM_BLOCK_DEFAULT = 256;
int stream_block() {
    const char* e = getenv("MA_W32_BLOCK");
    const int x = e ? atoi(e) : 0;
    return (x == 64 || x == 128 || x == 256 || x == 512) ? x : STREAM_BLOCK_DEFAULT;
}

bool make_ld(size_t n, size_t ld, Ld* L, const char* what) {
    if (ld >= n) { *L = Ld(ld); return true; }
    if (ld < 128 || (ld & (ld - 1)) != 0) {
        set_error(std::string(what) + ": a limb stride below n selects the tiled layout and must be a power of two >= 128");
        return false;
    }
    *L = Ld(ld, (unsigned)__builtin_ctzll((unsigned long long)ld));
    return true;
}
#define GRID(x) grid_for((x), BLOCK, L.s != 63)       /* launch geometry of a kernel over the batch described by L */
#define SGRID(x) grid_for((x), sb, L.s != 63)         /* ... of a streaming kernel with workgroups of sb = stream_block() threads */
#define MA_LD(what)                                                  \
    Ld L;                                                            \
    if (!make_ld(n, ld, &L, what)) return (int)hipErrorInvalidValue;

// elements per lane for a batch of n elements at limb stride ld whose buffers all sit at the addresses or-ed into `addr`: EPT
// elements need n >= EPT, a stride that is a multiple of EPT and 4 * EPT-byte aligned rows
int pick_ept(size_t n, size_t ld, uintptr_t addr) {
    const int cap = ept_cap();
    if (cap >= 4 && n >= 4 && ld % 4 == 0 && (addr & 15u) == 0) return 4;
    if (cap >= 2 && n >= 2 && ld % 2 == 0 && (addr & 7u) == 0) return 2;
    return 1;
}
uintptr_t U(const void* p) { return reinterpret_cast<uintptr_t>(p); }

// The body of a batch runs EPT elements per lane; what is left over (fewer than EPT elements: they share a tile with their
// predecessors, tiles hold a multiple of four elements) runs one element per lane at its own address with the flat stride.
template <class Op>
int launch_binary(const spint* a, const spint* b, spint* c, size_t n, size_t ld, void* stream, const char* what) {
    if (n == 0) return 0;
    MA_LD(what)
    hipStream_t s = (hipStream_t)stream;
    const int ept = pick_ept(n, ld, U(a) | U(b) | U(c)), sb = std::min(stream_block(), stream_block_max(ept));
    const size_t nt = n / ept, done = nt * ept, o = L.off<NL>(done);
    if (ept == 4) k_binary<P, Op, 4><<<SGRID(nt), sb, 0, s>>>(a, b, c, nt, L, L, L);
    else if (ept == 2) k_binary<P, Op, 2><<<SGRID(nt), sb, 0, s>>>(a, b, c, nt, L, L, L);
    else k_binary<P, Op, 1><<<SGRID(nt), sb, 0, s>>>(a, b, c, nt, L, L, L);
    if (done < n) k_binary<P, Op, 1><<<1, BLOCK, 0, s>>>(a + o, b + o, c + o, n - done, Ld(L.ld), Ld(L.ld), Ld(L.ld));
    return check_launch(what);
}
template <class Op>
int launch_unary(const spint* a, spint* c, size_t n, size_t ld, void* stream, const char* what) {
    if (n == 0) return 0;
    MA_LD(what)
    hipStream_t s = (hipStream_t)stream;
    const int ept = pick_ept(n, ld, U(a) | U(c)), sb = std::min(stream_block(), stream_block_max(ept));
    const size_t nt = n / ept, done = nt * ept, o = L.off<NL>(done);
    if (ept == 4) k_unary<P, Op, 4><<<SGRID(nt), sb, 0, s>>>(a, c, nt, L, L);
    else if (ept == 2) k_unary<P, Op, 2><<<SGRID(nt), sb, 0, s>>>(a, c, nt, L, L);
    else k_unary<P, Op, 1><<<SGRID(nt), sb, 0, s>>>(a, c, nt, L, L);
    if (done < n) k_unary<P, Op, 1><<<1, BLOCK, 0, s>>>(a + o, c + o, n - done, Ld(L.ld), Ld(L.ld));
    return check_launch(what);
}
// long-running per-element kernels (inversion, square root, progenitor): one element per lane
template <class Op>
int launch_unary_heavy(const spint* a, spint* c, size_t n, size_t ld, void* stream, const char* what) {
    if (n == 0) return 0;
    MA_LD(what)
    k_unary_heavy<P, Op><<<GRID(n), BLOCK, 0, (hipStream_t)stream>>>(a, c, n, L, L);
    return check_launch(what);
}

// ---- scalar staging: run a batched call on one element held in host memory
struct Stage : StageBase {
    template <class T>
    T* put(const T* host, size_t count) {
        T* d = reinterpret_cast<T*>(take(count * sizeof(T)));
        if (host) h2d(d, host, count * sizeof(T));
        return d;
    }
    template <class T>
    void get(T* host, const T* dev, size_t count) { d2h(host, dev, count * sizeof(T)); }
};
}  // namespace

extern "C" {

// ------------------------------------------------------------------ batched form
int BATCH(modadd)(const ma_spint32* a, const ma_spint32* b, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_binary<OpAdd<P>>(a, b, c, n, ld, st, "modadd(w32)"); }
int BATCH(modsub)(const ma_spint32* a, const ma_spint32* b, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_binary<OpSub<P>>(a, b, c, n, ld, st, "modsub(w32)"); }
int BATCH(modneg)(const ma_spint32* b, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpNeg<P>>(b, c, n, ld, st, "modneg(w32)"); }
int BATCH(modmul)(const ma_spint32* a, const ma_spint32* b, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_binary<OpMul<P>>(a, b, c, n, ld, st, "modmul(w32)"); }
int BATCH(modsqr)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpSqr<P>>(a, c, n, ld, st, "modsqr(w32)"); }
int BATCH(modcpy)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpCpy<P>>(a, c, n, ld, st, "modcpy(w32)"); }
int BATCH(nres)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpNres<P>>(a, c, n, ld, st, "nres(w32)"); }
int BATCH(redc)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpRedc<P>>(a, c, n, ld, st, "redc(w32)"); }
int BATCH(modpro)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary_heavy<OpPro<P>>(a, c, n, ld, st, "modpro(w32)"); }

// Large batches without a caller-supplied progenitor: simultaneous inversion (kernels32.h k_inv_simul), one modinv per up to 64
// elements, dispatched as the 64-bit form does it (capi_prime.inc): the prefix products go to the output buffer, or -- when the
// output IS the input -- to stream-ordered scratch of the library's own (not during stream capture; without scratch the per-element
// kernel runs).  MA_INV_SIMUL=0 keeps one modinv per element.  Same words either way: outputs in the normalised form
// nres(redc(1/x)), as at 64 bits.  The thresholds are the 64-bit form's.
constexpr size_t INV_SIMUL_LANES = 16384;      // lanes kept busy before elements start sharing an inversion
constexpr size_t INV_SIMUL_MIN = 32768;        // batches from this size on share inversions
int BATCH(modinv)(const ma_spint32* x, const ma_spint32* h, ma_spint32* z, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modinv(w32)")
    if (h == nullptr && n >= INV_SIMUL_MIN && ma::inv_simul()) {
        hipStream_t s = (hipStream_t)st;
        size_t rounds = (n + INV_SIMUL_LANES - 1) / INV_SIMUL_LANES;
        if (rounds > 64) rounds = 64;
        const size_t lanes = (n + rounds - 1) / rounds;
        const unsigned grid = (unsigned)((lanes + BLOCK - 1) / BLOCK);
        if (x != z) {
            k_inv_simul<P><<<grid, BLOCK, 0, s>>>(x, z, z, n, lanes, (int)rounds, L, L, L);
            return check_launch("modinv(w32, simultaneous)");
        }
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (s == nullptr || (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone)) {
            if (spint* ws = static_cast<spint*>(ma::scratch_alloc(n * NL * sizeof(spint), s))) {
                k_inv_simul<P><<<grid, BLOCK, 0, s>>>(x, z, ws, n, lanes, (int)rounds, L, L, Ld(n));
                ma::scratch_free(ws, s);
                return check_launch("modinv(w32, simultaneous, in place)");
            }
        }
        (void)hipGetLastError();
    }
    if (h == nullptr) return launch_unary_heavy<OpInv<P>>(x, z, n, ld, st, "modinv(w32)");
    k_inv_h<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, h, z, n, L, L, L);
    return check_launch("modinv(w32, h)");
}
int BATCH(modsqrt)(const ma_spint32* x, const ma_spint32* h, ma_spint32* r, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    if (h == nullptr) return launch_unary_heavy<OpSqrt<P>>(x, r, n, ld, st, "modsqrt(w32)");
    MA_LD("modsqrt(w32)")
    k_sqrt_h<P, false><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, h, r, nullptr, n, L);
    return check_launch("modsqrt(w32, h)");
}
int BATCH(modqr)(const ma_spint32* h, const ma_spint32* x, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modqr(w32)")
    if (h == nullptr) k_inplace<P, K_MODQR><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(const_cast<ma_spint32*>(x), out, n, L);
    else k_sqrt_h<P, true><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, h, nullptr, out, n, L);
    return check_launch("modqr(w32)");
}

int BATCH(modmli)(const ma_spint32* a, int b, ma_spint32* c, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modmli(w32)")
    hipStream_t s = (hipStream_t)st;
    const int ept = pick_ept(n, ld, U(a) | U(c)), sb = std::min(stream_block(), stream_block_max(ept));
    const size_t nt = n / ept, done = nt * ept, o = L.off<NL>(done);
    if (ept == 4) k_mli<P, 4><<<SGRID(nt), sb, 0, s>>>(a, b, c, nt, L, L);
    else if (ept == 2) k_mli<P, 2><<<SGRID(nt), sb, 0, s>>>(a, b, c, nt, L, L);
    else k_mli<P, 1><<<SGRID(nt), sb, 0, s>>>(a, b, c, nt, L, L);
    if (done < n) k_mli<P, 1><<<1, BLOCK, 0, s>>>(a + o, b, c + o, n - done, Ld(L.ld), Ld(L.ld));
    return check_launch("modmli(w32)");
}
int BATCH(modnsqr)(ma_spint32* a, int k, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modnsqr(w32)")
    k_nsqr<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, k, n, L);
    return check_launch("modnsqr(w32)");
}

#define MA_INPLACE(fn, KIND)                                                                           \
    int BATCH(fn)(ma_spint32 * a, int* out, size_t n, size_t ld, void* st) {                           \
        if (n == 0) return 0;                                                                          \
        MA_LD(#fn "(w32)")                                                                             \
        k_inplace<P, KIND><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, out, n, L);                      \
        return check_launch(#fn "(w32)");                                                              \
    }
MA_INPLACE(modfsb, K_MODFSB)
MA_INPLACE(flatten, K_FLATTEN)
MA_INPLACE(prop, K_PROP)        /* flag[j] = -1 where the top limb went negative (the mask prop returns), else 0 */
int BATCH(modhaf)(ma_spint32* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modhaf(w32)")
    k_inplace<P, K_MODHAF><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, nullptr, n, L);
    return check_launch("modhaf(w32)");
}
#define MA_PRED(fn, KIND)                                                                              \
    int BATCH(fn)(const ma_spint32* a, int* out, size_t n, size_t ld, void* st) {                      \
        if (n == 0) return 0;                                                                          \
        MA_LD(#fn "(w32)")                                                                             \
        k_inplace<P, KIND><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(const_cast<ma_spint32*>(a), out, n, L); \
        return check_launch(#fn "(w32)");                                                              \
    }
MA_PRED(modis1, K_MODIS1)
MA_PRED(modis0, K_MODIS0)
MA_PRED(modsign, K_MODSIGN)
MA_PRED(modlimbs, K_MODLIMBS)
int BATCH(modcmp)(const ma_spint32* a, const ma_spint32* b, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modcmp(w32)")
    k_cmp<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, b, out, n, L, L);
    return check_launch("modcmp(w32)");
}
int BATCH(modshl)(unsigned int k, ma_spint32* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modshl(w32)")
    k_shift<P, true><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(k, a, nullptr, n, L);
    return check_launch("modshl(w32)");
}
int BATCH(modshr)(unsigned int k, ma_spint32* a, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modshr(w32)")
    k_shift<P, false><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(k, a, out, n, L);
    return check_launch("modshr(w32)");
}
int BATCH(modint)(int x, ma_spint32* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modint(w32)")
    k_fill<P, K_INT><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, a, n, L);
    return check_launch("modint(w32)");
}
int BATCH(modzer)(ma_spint32* a, size_t n, size_t ld, void* st) { return BATCH(modint)(0, a, n, ld, st); }
int BATCH(modone)(ma_spint32* a, size_t n, size_t ld, void* st) { return BATCH(modint)(1, a, n, ld, st); }
int BATCH(mod2r)(unsigned int r, ma_spint32* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("mod2r(w32)")
    k_fill<P, K_2R><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>((int)r, a, n, L);
    return check_launch("mod2r(w32)");
}
int BATCH(modcmv)(const int* d, const ma_spint32* g, ma_spint32* f, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modcmv(w32)")
    k_cond<P, false><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(d, const_cast<ma_spint32*>(g), f, n, L, L);
    return check_launch("modcmv(w32)");
}
int BATCH(modcsw)(const int* d, ma_spint32* g, ma_spint32* f, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modcsw(w32)")
    k_cond<P, true><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(d, g, f, n, L, L);
    return check_launch("modcsw(w32)");
}
int BATCH(modimp)(const char* b, ma_spint32* a, int* flag, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modimp(w32)")
    if (reinterpret_cast<uintptr_t>(b) & 7u) { set_error("modimp: byte records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    k_imp<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(reinterpret_cast<const unsigned char*>(b), a, flag, n, L);
    return check_launch("modimp(w32)");
}
int BATCH(modexp)(const ma_spint32* a, char* b, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modexp(w32)")
    if (reinterpret_cast<uintptr_t>(b) & 7u) { set_error("modexp: byte records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    k_exp<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, reinterpret_cast<unsigned char*>(b), n, L);
    return check_launch("modexp(w32)");
}
// synthetic inputs (kernels32.h k_uniform): the integers of moduniform_<P>_batch for the same (seed, array, first), in this form's limbs
int BATCH(moduniform)(unsigned long long seed, unsigned long long array, size_t first, int plus_p, ma_spint32* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("moduniform(w32)")
    const uint64_t s0 = (uint64_t)seed * 0x9E3779B97F4A7C15ull + (uint64_t)array * 0xD1342543DE82EF95ull;
    k_uniform<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(s0, first, plus_p, out, n, L);
    return check_launch("moduniform(w32)");
}

// ------------------------------------------------------------------ scalar form (n = 1 through the device)
#define MA_SC_BIN(fn)                                                                         \
    void SCALAR(fn)(const ma_spint32* a, const ma_spint32* b, ma_spint32* c) {                \
        Stage s;                                                                              \
        spint *da = s.put(a, NL), *db = s.put(b, NL), *dc = s.put<spint>(nullptr, NL);        \
        if (!s.bad) s.check(BATCH(fn)(da, db, dc, 1, 1, nullptr), #fn);                       \
        s.get(c, dc, NL);                                                                     \
    }
#define MA_SC_UN(fn)                                                                          \
    void SCALAR(fn)(const ma_spint32* a, ma_spint32* c) {                                     \
        Stage s;                                                                              \
        spint *da = s.put(a, NL), *dc = s.put<spint>(nullptr, NL);                            \
        if (!s.bad) s.check(BATCH(fn)(da, dc, 1, 1, nullptr), #fn);                           \
        s.get(c, dc, NL);                                                                     \
    }
MA_SC_BIN(modadd)
MA_SC_BIN(modsub)
MA_SC_BIN(modmul)
MA_SC_UN(modneg)
MA_SC_UN(modsqr)
MA_SC_UN(modcpy)
MA_SC_UN(modpro)
MA_SC_UN(nres)
MA_SC_UN(redc)

void SCALAR(modmli)(const ma_spint32* a, int b, ma_spint32* c) {
    Stage s;
    spint *da = s.put(a, NL), *dc = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modmli)(da, b, dc, 1, 1, nullptr), "modmli");
    s.get(c, dc, NL);
}
void SCALAR(modnsqr)(ma_spint32* a, int n) {
    Stage s;
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modnsqr)(da, n, 1, 1, nullptr), "modnsqr");
    s.get(a, da, NL);
}
void SCALAR(modinv)(const ma_spint32* x, const ma_spint32* h, ma_spint32* z) {
    Stage s;
    spint *dx = s.put(x, NL), *dh = h ? s.put(h, NL) : nullptr, *dz = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modinv)(dx, dh, dz, 1, 1, nullptr), "modinv");
    s.get(z, dz, NL);
}
void SCALAR(modsqrt)(const ma_spint32* x, const ma_spint32* h, ma_spint32* r) {
    Stage s;
    spint *dx = s.put(x, NL), *dh = h ? s.put(h, NL) : nullptr, *dr = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modsqrt)(dx, dh, dr, 1, 1, nullptr), "modsqrt");
    s.get(r, dr, NL);
}
int SCALAR(modqr)(const ma_spint32* h, const ma_spint32* x) {
    Stage s;
    spint *dx = s.put(x, NL), *dh = h ? s.put(h, NL) : nullptr;
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modqr)(dh, dx, dr, 1, 1, nullptr), "modqr");
    int r;
    s.get(&r, dr, 1);
    return s.answer(r);
}
#define MA_SC_INPLACE_RET(fn, rtype)                                                          \
    rtype SCALAR(fn)(ma_spint32* a) {                                                         \
        Stage s;                                                                              \
        spint* da = s.put(a, NL);                                                             \
        int* dr = s.put<int>(nullptr, 1);                                                     \
        if (!s.bad) s.check(BATCH(fn)(da, dr, 1, 1, nullptr), #fn);                           \
        int r;                                                                                \
        s.get(&r, dr, 1);                                                                     \
        s.get(a, da, NL);                                                                     \
        return (rtype)r;                                                                      \
    }
MA_SC_INPLACE_RET(modfsb, ma_spint32)
MA_SC_INPLACE_RET(flatten, ma_spint32)
MA_SC_INPLACE_RET(prop, ma_spint32)   /* (ma_spint32)(int)-1 = all ones, as the emitted prop returns */
#define MA_SC_PRED(fn)                                                                        \
    int SCALAR(fn)(const ma_spint32* a) {                                                     \
        Stage s;                                                                              \
        spint* da = s.put(a, NL);                                                             \
        int* dr = s.put<int>(nullptr, 1);                                                     \
        if (!s.bad) s.check(BATCH(fn)(da, dr, 1, 1, nullptr), #fn);                           \
        int r;                                                                                \
        s.get(&r, dr, 1);                                                                     \
        return s.answer(r);                                                                   \
    }
MA_SC_PRED(modis1)
MA_SC_PRED(modis0)
MA_SC_PRED(modsign)
int SCALAR(modcmp)(const ma_spint32* a, const ma_spint32* b) {
    Stage s;
    spint *da = s.put(a, NL), *db = s.put(b, NL);
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modcmp)(da, db, dr, 1, 1, nullptr), "modcmp");
    int r;
    s.get(&r, dr, 1);
    return s.answer(r);
}
void SCALAR(modzer)(ma_spint32* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modzer)(da, 1, 1, nullptr), "modzer");
    s.get(a, da, NL);
}
void SCALAR(modone)(ma_spint32* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modone)(da, 1, 1, nullptr), "modone");
    s.get(a, da, NL);
}
void SCALAR(modint)(int x, ma_spint32* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modint)(x, da, 1, 1, nullptr), "modint");
    s.get(a, da, NL);
}
void SCALAR(mod2r)(unsigned int r, ma_spint32* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(mod2r)(r, da, 1, 1, nullptr), "mod2r");
    s.get(a, da, NL);
}
void SCALAR(modcmv)(int b, const ma_spint32* g, volatile ma_spint32* f) {
    Stage s;
    int bb = b;
    int* dd = s.put(&bb, 1);
    spint *dg = s.put(g, NL), *df = s.put(const_cast<const ma_spint32*>(f), NL);
    if (!s.bad) s.check(BATCH(modcmv)(dd, dg, df, 1, 1, nullptr), "modcmv");
    s.get(const_cast<ma_spint32*>(f), df, NL);
}
void SCALAR(modcsw)(int b, volatile ma_spint32* g, volatile ma_spint32* f) {
    Stage s;
    int bb = b;
    int* dd = s.put(&bb, 1);
    spint *dg = s.put(const_cast<const ma_spint32*>(g), NL), *df = s.put(const_cast<const ma_spint32*>(f), NL);
    if (!s.bad) s.check(BATCH(modcsw)(dd, dg, df, 1, 1, nullptr), "modcsw");
    s.get(const_cast<ma_spint32*>(g), dg, NL);
    s.get(const_cast<ma_spint32*>(f), df, NL);
}
void SCALAR(modshl)(unsigned int n, ma_spint32* a) {
    Stage s;
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modshl)(n, da, 1, 1, nullptr), "modshl");
    s.get(a, da, NL);
}
int SCALAR(modshr)(unsigned int n, ma_spint32* a) {
    Stage s;
    spint* da = s.put(a, NL);
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modshr)(n, da, dr, 1, 1, nullptr), "modshr");
    int r;
    s.get(&r, dr, 1);
    s.get(a, da, NL);
    return r;
}
void SCALAR(modhaf)(ma_spint32* a) {
    Stage s;
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modhaf)(da, 1, 1, nullptr), "modhaf");
    s.get(a, da, NL);
}
void SCALAR(modexp)(const ma_spint32* a, char* b) {
    Stage s;
    char* db = s.put<char>(nullptr, NB);           // (first: the staging buffer is aligned, the byte record wants 8 bytes)
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modexp)(da, db, 1, 1, nullptr), "modexp");
    s.get(b, db, NB);
}
int SCALAR(modimp)(const char* b, ma_spint32* a) {
    Stage s;
    char* db = s.put(b, NB);
    spint* da = s.put<spint>(nullptr, NL);
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modimp)(db, da, dr, 1, 1, nullptr), "modimp");
    int r;
    s.get(&r, dr, 1);
    s.get(a, da, NL);
    return s.answer(r);
}

}  // extern "C"
