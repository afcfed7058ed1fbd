// modarith_amd/csrc/capi_prime.inc -- per-prime body of the C-ABI shim.  Included by capi_<PRIME>.hip
// with MA_P (parameter struct), MA_NAME (token) defined, and optionally MA_LADDER_A24 / MA_LADDER_COF.
// Every entry point declared by MODARITH_AMD_DECLARE(P) in include/modarith_amd.h is defined here or in capi_field.inc, the part
// shared with the 32-bit word form (capi_w32.inc): this file keeps the product-policy dispatch, modmuls, the lazy forms, the time.c
// protocol and the ladders.
#include "../../include/modarith_amd.h"
#include "capi_common.h"
#include "kernels.h"
#include "ladder.h"
#ifdef MA_LADDER_FE26
#include "fe26.h"
#endif
#ifdef MA_LADDER_FE28
#include "fe28.h"
#endif
#include <string.h>
#include <algorithm>

#define MA_CAT3_(a, b, c) a##_##b##_##c
#define MA_CAT3(a, b, c) MA_CAT3_(a, b, c)
#define BATCH(fn) MA_CAT3(fn, MA_NAME, batch)
#define SCALAR(fn) MA_CAT3(fn, MA_NAME, ct)

namespace {
using namespace ma;
using P = MA_P;
constexpr int NL = P::N;
constexpr int NB = P::NBYTES;
#define MA_WHAT(fn) fn
#define MA_WHAT2(fn, how) fn "(" how ")"
// streaming kernels: 16 bytes per lane at the most, workgroups of BLOCK
int ept_cap() { return 2; }
int stream_block() { return BLOCK; }
constexpr bool INV_SIMUL = NL <= 9 && P::RADIX <= 60;   // (wider fields keep one inversion per element: register footprint; radix > 60: no flag bits)
}  // namespace
#include "capi_field.inc"

namespace {
int modinv_each(const spint* x, spint* z, size_t n, size_t ld, void* st) {
    if (force_fast() && P::SPLIT > 0) return launch_unary_heavy<OpInv<P, true>>(x, z, n, ld, st, "modinv(fast)");
    if (force_exact() || P::SPLIT == 0) return launch_unary_heavy<OpInv<P>>(x, z, n, ld, st, "modinv(exact)");
    return launch_unary_heavy<OpAutoUnary<P, OpInv>>(x, z, n, ld, st, "modinv");
}
bool inv_may_share() { return !force_exact(); }
template <int EPT, bool AUTO>
void launch_shared(const spint* a, const Elem<P>& b0, spint* c, size_t nt, Ld L, unsigned grid, hipStream_t s) {
    k_mul_shared<P, EPT, AUTO><<<grid, BLOCK, 0, s>>>(a, b0, c, nt, L, L);
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------ batched form: what chooses a product policy, and what only this word length has
int BATCH(modadd_lazy)(const ma_spint* a, const ma_spint* b, ma_spint* c, size_t n, size_t ld, void* st) { return launch_binary<OpAddLazy<P>>(a, b, c, n, ld, st, "modadd_lazy"); }
int BATCH(modsub_lazy)(const ma_spint* a, const ma_spint* b, ma_spint* c, size_t n, size_t ld, void* st) { return launch_binary<OpSubLazy<P>>(a, b, c, n, ld, st, "modsub_lazy"); }
int BATCH(modneg_lazy)(const ma_spint* b, ma_spint* c, size_t n, size_t ld, void* st) { return launch_unary<OpNegLazy<P>>(b, c, n, ld, st, "modneg_lazy"); }
// Product policy of the element-wise kernels.  Default for modmul / modsqr: per wave, the split products when every
// lane's operands are inside their limb contract, else the exact ones (OpMulAuto: same results for every input; keeps
// the 8-limb kernels HBM-bound).  Testing knobs: MA_FORCE_EXACT=1 -> exact products everywhere; MA_FORCE_FAST=1 ->
// the split products unguarded, also in nres/redc/modinv, so that the whole parity suite can be run against them.
int BATCH(modmul)(const ma_spint* a, const ma_spint* b, ma_spint* c, size_t n, size_t ld, void* st) {
    if (force_fast() && P::SPLIT > 0) return launch_binary<OpMul<P, true>>(a, b, c, n, ld, st, "modmul(fast)");
    if (force_exact() || P::SPLIT == 0) return launch_binary<OpMul<P>>(a, b, c, n, ld, st, "modmul(exact)");
    return launch_binary<OpMulAuto<P>>(a, b, c, n, ld, st, "modmul");
}
int BATCH(modsqr)(const ma_spint* a, ma_spint* c, size_t n, size_t ld, void* st) {
    if (force_fast() && P::SPLIT > 0) return launch_unary<OpSqr<P, true>>(a, c, n, ld, st, "modsqr(fast)");
    if (force_exact() || P::SPLIT == 0) return launch_unary<OpSqr<P>>(a, c, n, ld, st, "modsqr(exact)");
    return launch_unary<OpSqrAuto<P>>(a, c, n, ld, st, "modsqr");
}
int BATCH(nres)(const ma_spint* a, ma_spint* c, size_t n, size_t ld, void* st) {
    if (force_fast() && P::SPLIT > 0) return launch_unary<OpNres<P, true>>(a, c, n, ld, st, "nres(fast)");
    if (force_exact() || P::SPLIT == 0 || !P::MONTGOMERY) return launch_unary<OpNres<P>>(a, c, n, ld, st, "nres(exact)");
    return launch_unary<OpNresAuto<P>>(a, c, n, ld, st, "nres");
}
int BATCH(redc)(const ma_spint* a, ma_spint* c, size_t n, size_t ld, void* st) {
    if (force_fast() && P::SPLIT > 0) return launch_unary<OpRedc<P, true>>(a, c, n, ld, st, "redc(fast)");
    if (force_exact() || P::SPLIT == 0 || !P::MONTGOMERY) return launch_unary<OpRedc<P>>(a, c, n, ld, st, "redc(exact)");
    return launch_unary<OpRedcAuto<P>>(a, c, n, ld, st, "redc");
}
int BATCH(modpro)(const ma_spint* a, ma_spint* c, size_t n, size_t ld, void* st) {
    if (force_exact() || P::SPLIT == 0) return launch_unary_heavy<OpPro<P>>(a, c, n, ld, st, "modpro(exact)");
    return launch_unary_heavy<OpAutoUnary<P, OpPro>>(a, c, n, ld, st, "modpro");
}

int BATCH(modsqrt)(const ma_spint* x, const ma_spint* h, ma_spint* r, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modsqrt")
    if (h == nullptr) {
        if (force_exact() || P::SPLIT == 0) return launch_unary_heavy<OpSqrt<P>>(x, r, n, ld, st, "modsqrt(exact)");
        return launch_unary_heavy<OpAutoUnary<P, OpSqrt>>(x, r, n, ld, st, "modsqrt");
    }
    k_sqrt_h<P, false><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, h, r, nullptr, n, L);
    return check_launch("modsqrt(h)");
}
int BATCH(modqr)(const ma_spint* h, const ma_spint* x, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("modqr")
    if (h == nullptr) k_inplace<P, K_MODQR><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(const_cast<ma_spint*>(x), out, n, L);
    else k_sqrt_h<P, true><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, h, nullptr, out, n, L);
    return check_launch("modqr");
}

// shared multiplicand.  b0 is host memory (the reference passes nres'd constants by pointer: monty.py:1386-1416, edwards.c:92); it is
// checked against the limb contract here, once, and travels in the kernel arguments.  Product policy as for modmul.
int BATCH(modmuls)(const ma_spint* a, const ma_spint* b0_host, ma_spint* c, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    Elem<P> b0;
    bool b_ok = P::SPLIT > 0 && !force_exact();
    for (int i = 0; i < NL; i++) {
        b0.l[i] = b0_host[i];
        if (P::RADIX + 2 < 64 && (b0_host[i] >> ((P::RADIX + 2) & 63)) != 0) b_ok = false;
    }
    MA_LD("modmuls")
    hipStream_t s = (hipStream_t)st;
    if (n >= 2 && ld % 2 == 0 && aligned16(a) && aligned16(c)) {
        size_t nt = n / 2;
        if (b_ok) launch_shared<2, true>(a, b0, c, nt, L, GRID(nt), s);
        else launch_shared<2, false>(a, b0, c, nt, L, GRID(nt), s);
        const size_t o = L.off<NL>(n - 1);
        if (n & 1) launch_shared<1, false>(a + o, b0, c + o, 1, Ld(L.ld), 1, s);
    } else {
        launch_shared<1, false>(a, b0, c, n, L, GRID(n), s);
    }
    return check_launch("modmuls");
}

// time.c protocol on the device: z[j] = redc(chain(x[j], y[j])); kind 0 modmul, 1 modsqr, 2 modinv
int BATCH(time_protocol)(int kind, const ma_spint* x, const ma_spint* y, ma_spint* z, long outer, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD("time_protocol")
    hipStream_t s = (hipStream_t)st;
    if (kind < 0 || kind > 2) { set_error("time_protocol: kind must be 0, 1 or 2"); return (int)hipErrorInvalidValue; }
    // product policy as for the element-wise kernels: per-wave vote by default, MA_FORCE_FAST / MA_FORCE_EXACT pin one
    const int policy = (P::SPLIT == 0 || force_exact()) ? 0 : (force_fast() ? 1 : 2);
#define MA_TIME_LAUNCH(KIND, POL) k_time<P, KIND, POL><<<GRID(n), BLOCK, 0, s>>>(x, y, z, outer, n, L)
    if (policy == 0) { if (kind == 0) MA_TIME_LAUNCH(0, 0); else if (kind == 1) MA_TIME_LAUNCH(1, 0); else MA_TIME_LAUNCH(2, 0); }
    else if (policy == 1) { if (kind == 0) MA_TIME_LAUNCH(0, 1); else if (kind == 1) MA_TIME_LAUNCH(1, 1); else MA_TIME_LAUNCH(2, 1); }
    else { if (kind == 0) MA_TIME_LAUNCH(0, 2); else if (kind == 1) MA_TIME_LAUNCH(1, 2); else MA_TIME_LAUNCH(2, 2); }
#undef MA_TIME_LAUNCH
    return check_launch("time_protocol");
}

// ------------------------------------------------------------------ RFC 7748 ladder
#ifdef MA_LADDER_A24
#define LADDER_BATCH_(name) rfc7748_##name##_batch
#define LADDER_BATCH(name) LADDER_BATCH_(name)
#define LADDER_SCALAR_(name) rfc7748_##name
#define LADDER_SCALAR(name) LADDER_SCALAR_(name)
#if defined(MA_LADDER_FE26) || defined(MA_LADDER_FE28)
// ---- split form with a caller-supplied workspace (csrc/fe_finish.h): per scalar, Nbytes of canonical z2 and the prefix-
// product limbs (10 / 16 x 32 bit).  rounds = how many scalars share one inversion (at most 32; fewer for small batches, so
// that the second kernel still fills the chip).
#ifdef MA_LADDER_FE26
using LadderFe = Fe26;
constexpr int LADDER_NL = 10, LADDER_NW = 4;
#define LADDER_XZ_KERNEL k_x25519_fe26_xz
#else
using LadderFe = Fe28;
constexpr int LADDER_NL = 16, LADDER_NW = 7;
#define LADDER_XZ_KERNEL k_x448_fe28_xz
#endif
#define LADDER_WS_(name) rfc7748_##name##_batch_workspace_bytes
#define LADDER_WS(name) LADDER_WS_(name)
#define LADDER_BATCH_WS_(name) rfc7748_##name##_batch_ws
#define LADDER_BATCH_WS(name) LADDER_BATCH_WS_(name)
constexpr size_t LADDER_SPLIT_MIN = 8192;
size_t LADDER_WS(MA_NAME)(size_t n) { return n * (LADDER_NW * sizeof(uint64_t) + LADDER_NL * sizeof(uint32_t)); }
int LADDER_BATCH_WS(MA_NAME)(const char* bk, const char* bu, char* bv, size_t n, void* workspace, size_t workspace_bytes, void* st) {
    if (n == 0) return 0;
    if (records_misaligned(bk, bu, bv, workspace)) return reject("rfc7748: byte records and workspace must be 8-byte aligned");
    if (workspace == nullptr || workspace_bytes < LADDER_WS(MA_NAME)(n))
        return reject("rfc7748 batch_ws: workspace too small (see rfc7748_<CURVE>_batch_workspace_bytes)");
    hipStream_t s = (hipStream_t)st;
    const int block = ladder_block();
    if (ladder_use_field()) {
        // MA_LADDER_IMPL=field selects the field.c-form ladder for EVERY entry point (A/B and parity runs must measure what they
        // name): the self-contained kernel, one inversion per lane; the workspace stays unused
        k_rfc7748<P, MA_LADDER_A24, MA_LADDER_COF><<<grid_for(n, block), block, 0, s>>>(
            reinterpret_cast<const spint*>(bk), reinterpret_cast<const spint*>(bu), reinterpret_cast<spint*>(bv), n);
        return check_launch("rfc7748(field form)");
    }
    uint64_t* wz = reinterpret_cast<uint64_t*>(workspace);
    uint32_t* wc = reinterpret_cast<uint32_t*>(wz + (size_t)LADDER_NW * n);
    LADDER_XZ_KERNEL<<<grid_for(n, block), block, 0, s>>>(reinterpret_cast<const uint64_t*>(bk), reinterpret_cast<const uint64_t*>(bu),
                                                         reinterpret_cast<uint64_t*>(bv), wz, n);
    const auto [L, rounds] = shared_inv_rounds(n);
    k_fe_finish<LadderFe, LADDER_NL, LADDER_NW><<<(unsigned)((L + 63) / 64), 64, 0, s>>>(reinterpret_cast<uint64_t*>(bv), wz, wc, n, L, rounds);
    return check_launch("rfc7748(split)");
}
// the split form on a stream-ordered workspace of the library's own, when that is possible: not while the stream is being
// captured, not with MA_LADDER_SPLIT=0, not for small batches; false = the caller launches the self-contained kernel
static bool ladder_try_split(const char* bk, const char* bu, char* bv, size_t n, void* st, int* rc) {
    if (n < LADDER_SPLIT_MIN || !ladder_split()) return false;
    hipStream_t s = (hipStream_t)st;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (s != nullptr && hipStreamIsCapturing(s, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
    if (cs != hipStreamCaptureStatusNone) return false;
    const size_t bytes = LADDER_WS(MA_NAME)(n);
    void* ws = scratch_alloc(bytes, s);
    if (!ws) return false;
    *rc = LADDER_BATCH_WS(MA_NAME)(bk, bu, bv, n, ws, bytes, st);
    scratch_free(ws, s);
    return true;
}
#endif
int LADDER_BATCH(MA_NAME)(const char* bk, const char* bu, char* bv, size_t n, void* st) {
    if (n == 0) return 0;
    if (records_misaligned(bk, bu, bv)) return reject("rfc7748: byte records must be 8-byte aligned");
    const int block = ladder_block();
#if defined(MA_LADDER_FE26) || defined(MA_LADDER_FE28)
    // the fused 32-bit-limb ladders (csrc/fe26.h: X25519 on 10 x 25.5 bits; csrc/fe28.h: X448 on 16 x 28 bits);
    // MA_LADDER_IMPL=field selects the field.c-form ladder below.  Large batches take the split form (one inversion per
    // `rounds` scalars), otherwise the self-contained kernel with one inversion per lane.  Same bytes either way.
    if (!ladder_use_field()) {
        int rc = 0;
        if (ladder_try_split(bk, bu, bv, n, st, &rc)) return rc;
#ifdef MA_LADDER_FE26
        k_x25519_fe26<<<grid_for(n, block), block, 0, (hipStream_t)st>>>(
            reinterpret_cast<const uint64_t*>(bk), reinterpret_cast<const uint64_t*>(bu), reinterpret_cast<uint64_t*>(bv), n);
        return check_launch("rfc7748(fe26)");
#else
        k_x448_fe28<<<grid_for(n, block), block, 0, (hipStream_t)st>>>(
            reinterpret_cast<const uint64_t*>(bk), reinterpret_cast<const uint64_t*>(bu), reinterpret_cast<uint64_t*>(bv), n);
        return check_launch("rfc7748(fe28)");
#endif
    }
#endif
    k_rfc7748<P, MA_LADDER_A24, MA_LADDER_COF><<<grid_for(n, block), block, 0, (hipStream_t)st>>>(
        reinterpret_cast<const spint*>(bk), reinterpret_cast<const spint*>(bu), reinterpret_cast<spint*>(bv), n);
    return check_launch("rfc7748(field form)");
}
void LADDER_SCALAR(MA_NAME)(const char* bk, const char* bu, char* bv) {
    Stage s;
    char *dk = s.put(bk, NB), *du = s.put(bu, NB), *dv = s.put<char>(nullptr, NB);
    if (!s.bad) s.check(LADDER_BATCH(MA_NAME)(dk, du, dv, 1, nullptr), "rfc7748");
    s.get(bv, dv, NB);
}
#endif

}  // extern "C"
