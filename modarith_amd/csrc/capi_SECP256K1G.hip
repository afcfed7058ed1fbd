// modarith_amd/csrc/capi_SECP256K1G.hip -- ecn_secp256k1_mulgen_get_batch: generator multiplication fused with the affine export
// (csrc/wn26.h wn26_mulgen_get_one), the call sequence ecnXXXgen + ecnXXXmul + ecnXXXget that opens key generation and
// signing in the reference's ECDSA code (nist256.c:150-161, 214-222).  Fixed-base table: generated/comb_SECP256K1.h.
#include "../../include/modarith_amd.h"
#include "capi_common.h"
#include "generated/curve_SECP256K1.h"
#include "generated/comb_SECP256K1.h"
#include "kernels.h"
#include "wn26.h"
#include "glv26.h"
#include "wn_export.h"

namespace ma {

MA_COMB_TABLE(CombSECP256K1, comb_secp256k1, SECP256K1);       // csrc/comb.h

// e*G, ONE scalar per lane, (X : Y : Z) to the inversion shared by up to 32 records (csrc/wn_export.h; round 5).  Rounds 2-4 shared one
// inversion between the four scalars of a lane, whose four results cost 120 registers (the kernel below: 252-254 registers, two waves
// per SIMD); it stays for callers without scratch (a stream under capture: this entry point has no workspace argument).
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 4)))
void k_secp256k1_mulgen(const unsigned char* e, WnExpWs ex) {
    const size_t t = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (t >= ex.m) return;
    spint ew[4];
    load_be_record<P_SECP256K1>(e, t, ew);
    Wn26<CvSecp256k1>::Pt R;
    wn26_mulgen_acc<CvSecp256k1, CombSECP256K1>(ew, R);
    ex.store<Fk26>(t, R.X, R.Y, R.Z);
}

// MULGEN_G scalars per lane (elements t, t + lanes, ... of a MULGEN_G * lanes stride) share one inversion
#ifndef MULGEN_G
#define MULGEN_G 4
#endif
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 4)))
void k_secp256k1_mulgen_get(const unsigned char* e, unsigned char* xb, unsigned char* yb, int* sign, size_t n) {
    using P = P_SECP256K1;
    const size_t lanes = (size_t)gridDim.x * blockDim.x;
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < n; t += MULGEN_G * lanes) {
        spint xw[MULGEN_G][4], yw[MULGEN_G][4];
        wn26_mulgen_get_many<CvSecp256k1, CombSECP256K1, MULGEN_G>(
            [&](int g, spint* ew) { const size_t tg = t + (size_t)g * lanes; load_be_record<P>(e, tg < n ? tg : t, ew); }, xw, yw);
        static_for<0, MULGEN_G>([&](auto GI) {
            const size_t tg = t + (size_t)GI * lanes;
            if (tg < n) store_affine_be<P>(xb, yb, sign, tg, xw[GI], yw[GI]);
        });
    }
}

// e*G + f*Q and its affine export (verification, nist256.c:251-256): the per-lane table of Q in the workspace as for mul_get,
// the generator part through the constant table above
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3)))
void k_secp256k1_mulgen2_get(const unsigned char* e, const unsigned char* f, const spint* Qb, size_t ld, uint64_t* ws, WnExpWs ex) {
    const size_t n = ex.m;                                  // the records of this chunk; (X : Y : Z) of the result to the shared inversion (wn_export.h)
    using P = P_SECP256K1;
    using DIG = GlvLds;                                      // f split by the endomorphism (csrc/glv26.h)
    __shared__ unsigned char digs[DIG::COUNT * 64];          // the windows of f's halves in LDS; Q's table in the wave's slab; index at use: see the mul_get unit
    const WnTabSlab T{ws + (size_t)blockIdx.x * (64 * (size_t)WN26_TABLE_WORDS), threadIdx.x};
    unsigned char* col = digs + threadIdx.x;
    for (size_t base = (size_t)blockIdx.x * 64; base < n; base += (size_t)gridDim.x * 64) {
        auto t = [&]() { return base + (size_t)(T.origin() - T.base); };
        if (t() >= n) continue;
        DIG dig;
        {
            spint fw[4];
            load_be_record<P>(f, t(), fw);
            dig.fill(fw, col);
        }
        spint X[5], Y[5], Z[5];
        load_xyz<5>(Qb, ld, 0, t, X, Y, Z);
        Wn26<CvSecp256k1>::Pt R;
        secp256k1_glv_mul_acc(dig, X, Y, Z, T, R);
        spint ew[4];
        load_be_record<P>(e, t(), ew);                          // (fetched here: eight registers less across f Q)
        wn26_mulgen_acc<CvSecp256k1, CombSECP256K1, false>(ew, R);
        ex.store<Fk26>(t(), R.X, R.Y, R.Z);
    }
}

}  // namespace ma

using namespace ma;

namespace {
size_t fused2_lanes(size_t n) {
    const size_t lanes = (n + 63) / 64 * 64, cap = (size_t)3 * 1024 * 64;
    return lanes < cap ? lanes : cap;
}
}  // namespace

static size_t slab_bytes(size_t n) { return (fused2_lanes(n) + 36) * WN26_TABLE_WORDS * sizeof(uint64_t); }
extern "C" size_t ecn_secp256k1_mulgen2_get_workspace_bytes(size_t n) { return slab_bytes(n) + WnExpWs::bytes(n); }

extern "C" int ecn_secp256k1_mulgen2_get_batch(const char* e, const char* f, const ma_spint* Q, char* x, char* y, int* sign, size_t n, size_t ld,
                                           void* workspace, size_t workspace_bytes, void* st) {
    if (n == 0) return 0;
    if (records_misaligned(e, f, x, y)) return reject("ecn mulgen2_get: byte records must be 8-byte aligned");
    if (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7u) || workspace_bytes < ecn_secp256k1_mulgen2_get_workspace_bytes(n))
        return reject("ecn mulgen2_get: workspace missing, not 8-byte aligned or too small (see ecn_secp256k1_mulgen2_get_workspace_bytes)");
    hipStream_t s = (hipStream_t)st;
    for (size_t first = 0; first < n; first += WNEXP_CHUNK) {
        const size_t m = n - first < WNEXP_CHUNK ? n - first : WNEXP_CHUNK;
        const WnExpWs ex(reinterpret_cast<char*>(workspace) + slab_bytes(n), m);
        k_secp256k1_mulgen2_get<<<(unsigned)(fused2_lanes(m) / 64), 64, 0, s>>>(reinterpret_cast<const unsigned char*>(e) + first * P_SECP256K1::NBYTES, reinterpret_cast<const unsigned char*>(f) + first * P_SECP256K1::NBYTES, Q + first, ld, reinterpret_cast<uint64_t*>(workspace), ex);
        wn_export<Fk26, P_SECP256K1, 3>(ex, reinterpret_cast<unsigned char*>(x), reinterpret_cast<unsigned char*>(y), sign, first, s);
    }
    return check_launch("ecn mulgen2_get");
}

extern "C" int ecn_secp256k1_mulgen_get_batch(const char* e, char* x, char* y, int* sign, size_t n, void* st) {
    if (n == 0) return 0;
    if (records_misaligned(e, x, y)) return reject("ecn mulgen_get: byte records must be 8-byte aligned");
    hipStream_t s = (hipStream_t)st;
    EdLadScratch ws(nullptr, 0, WnExpWs::bytes(n), 8, s);              // no workspace argument: the library's scratch pool
    if (ws.p) {
        for (size_t first = 0; first < n; first += WNEXP_CHUNK) {
            const size_t m = n - first < WNEXP_CHUNK ? n - first : WNEXP_CHUNK;
            const WnExpWs ex(ws.p, m);
            k_secp256k1_mulgen<<<(unsigned)((m + 63) / 64), 64, 0, s>>>(reinterpret_cast<const unsigned char*>(e) + first * P_SECP256K1::NBYTES, ex);
            wn_export<Fk26, P_SECP256K1, 4>(ex, reinterpret_cast<unsigned char*>(x), reinterpret_cast<unsigned char*>(y), sign, first, s);
        }
        return check_launch("ecn mulgen_get");
    }
    const size_t lanes = ((n + MULGEN_G - 1) / MULGEN_G + 63) / 64 * 64, cap = (size_t)4 * 1024 * 64;       // MULGEN_G scalars per lane; at most 4 waves on each of the 1024 SIMDs
    k_secp256k1_mulgen_get<<<(unsigned)((lanes < cap ? lanes : cap) / 64), 64, 0, (hipStream_t)st>>>(
        reinterpret_cast<const unsigned char*>(e), reinterpret_cast<unsigned char*>(x), reinterpret_cast<unsigned char*>(y), sign, n);
    return check_launch("ecn mulgen_get (self-contained)");
}
