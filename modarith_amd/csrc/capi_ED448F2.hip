// modarith_amd/csrc/capi_ED448F2.hip -- ecn_ed448_mul2_get_batch: double multiplication e*P + f*Q fused with the affine
// export (csrc/ed28s.h: the Straus form), the verification pattern ecnXXXmul2 + ecnXXXget of the reference's signature code
// (ed448.c:290-310).
#include "../../include/modarith_amd.h"
#include "capi_common.h"
#include "generated/params_X448.h"
#include "kernels.h"
#include "ed28.h"
#include "ed28s.h"
#include "ed28l_k.h"

namespace ma {

// one pair per lane, one wave per workgroup: signed 4-bit windows of both scalars in LDS (one byte per window), the two 9-entry tables
// in the wave's slab of the workspace (two 128-byte lines per entry and lane, read by index), the Edwards (X : Y : Z) of the sum to the
// shared inversion of csrc/edlad_k.h.  Records first .. first + ws.m of the caller's arrays.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2)))
void k_ed448_mul2_straus(const unsigned char* e, const spint* Pb, const unsigned char* f, const spint* Qb, size_t first, size_t ld,
                         uint64_t* slab, Ed28lWs ws) {
    using P = P_X448;
    using S = Ed28Straus;
    __shared__ unsigned char digs[2 * 113 * 64];
    unsigned char* ce = digs + threadIdx.x;
    unsigned char* cf = ce + 113 * 64;
    Straus448TabSlab tab{slab + ((size_t)blockIdx.x * 64 + threadIdx.x) * (18 * 32)};
    for (size_t base = (size_t)blockIdx.x * 64; base < ws.m; base += (size_t)gridDim.x * 64) {
        auto t = [&]() {
            unsigned l = threadIdx.x;
            asm volatile("" : "+v"(l));
            return base + l;
        };
        if (t() >= ws.m) continue;
        {
            spint w[7];
            load_be_record<P>(e, first + t(), w);
            W448_4Lds::fill(w, ce);
            load_be_record<P>(f, first + t(), w);
            W448_4Lds::fill(w, cf);
        }
#pragma unroll 1
        for (int which = 0; which < 2; which++) {
            const spint* B = which ? Qb : Pb;
            spint X[8], Y[8], Z[8];
            load_xyz<8>(B, ld, first, t, X, Y, Z);
            S::build(tab, which, X, Y, Z);
        }
        W448_4Lds de{ce}, df{cf};
        S::Ext R;
        S::walk(de, df, tab, R);
        ws.store_xyz(t(), R.X, R.Y, R.Z);
    }
}

}  // namespace ma

using namespace ma;

static size_t straus_waves(size_t n) {
    const size_t w = (n + 63) / 64, cap = (size_t)2 * 1024;          // two waves on each of the 1024 SIMDs
    return w < cap ? w : cap;
}

static size_t mul2_get_net_bytes(size_t n) {
    const size_t m = n < EDLAD_CHUNK ? n : EDLAD_CHUNK;
    return straus_waves(m) * STRAUS448_SLAB_BYTES_PER_WAVE + ed28l_workspace_bytes(n);
}
// (+ 127: the table slab wants 128-byte alignment, EdLadScratch rounds the caller's pointer up)
extern "C" size_t ecn_ed448_mul2_get_workspace_bytes(size_t n) { return mul2_get_net_bytes(n) + 127; }

extern "C" int ecn_ed448_mul2_get_batch(const char* e, const ma_spint* P, const char* f, const ma_spint* Q, char* x, char* y, int* sign,
                                        size_t n, size_t ld, void* workspace, size_t workspace_bytes, void* st) {
    if (n == 0) return 0;
    if (records_misaligned(e, f, x, y)) return reject("ecn mul2_get: byte records must be 8-byte aligned");
    hipStream_t s = (hipStream_t)st;
    EdLadScratch wsp(workspace, workspace_bytes, mul2_get_net_bytes(n), 128, s);
    if (!wsp.p) return reject("ecn mul2_get: no usable workspace -- " + std::string(wsp.why) + " (pass ecn_ed448_mul2_get_workspace_bytes(n) bytes; the library's own scratch pool is not available while the stream is being captured)");
    const unsigned char *eb = reinterpret_cast<const unsigned char*>(e), *fb = reinterpret_cast<const unsigned char*>(f);
    const size_t slab_bytes = straus_waves(n < EDLAD_CHUNK ? n : EDLAD_CHUNK) * STRAUS448_SLAB_BYTES_PER_WAVE;
    for (size_t first = 0; first < n; first += EDLAD_CHUNK) {
        const size_t m = n - first < EDLAD_CHUNK ? n - first : EDLAD_CHUNK;
        Ed28lWs ws(reinterpret_cast<unsigned char*>(wsp.p) + slab_bytes, m);
        k_ed448_mul2_straus<<<(unsigned)straus_waves(m), 64, 0, s>>>(eb, P, fb, Q, first, ld, reinterpret_cast<uint64_t*>(wsp.p), ws);
        edlad_export<LadT448, 3>(ws, reinterpret_cast<unsigned char*>(x), reinterpret_cast<unsigned char*>(y), sign, first, s);
    }
    return check_launch("ecn mul2_get (Straus form)");
}
