// modarith_amd/csrc/capi_w32_common.hip -- the entry points of include/modarith_amd_w32.h that belong to no single prime:
// field_info of the 32-bit word form, AoS <-> SoA of uint32_t limbs, batch sizing.
#include "../../include/modarith_amd_w32.h"
#include "capi_common.h"
#include "kernels32.h"
#include <string.h>

namespace ma32 {
// AoS <-> SoA of 32-bit limbs (element-major records of nlimbs words <-> the batch layout): one element per lane.  A bring-up /
// interchange path: the records of a field.cu-style caller are 36 or 64 bytes, and a wave reads them as one contiguous stretch.
__global__ __launch_bounds__(BLOCK) void k_aos2soa(const spint* aos, spint* soa, size_t n, int nlimbs, Ld L) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        const size_t o = (((t >> L.s) * (size_t)nlimbs) << L.s) + (t & ((((size_t)1) << L.s) - 1));
        for (int i = 0; i < nlimbs; i++) soa[o + (size_t)i * L.ld] = aos[t * (size_t)nlimbs + i];
    }
}
__global__ __launch_bounds__(BLOCK) void k_soa2aos(const spint* soa, spint* aos, size_t n, int nlimbs, Ld L) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        const size_t o = (((t >> L.s) * (size_t)nlimbs) << L.s) + (t & ((((size_t)1) << L.s) - 1));
        for (int i = 0; i < nlimbs; i++) aos[t * (size_t)nlimbs + i] = soa[o + (size_t)i * L.ld];
    }
}

}  // namespace ma32

namespace {
using namespace ma32;
bool conv_ld(size_t n, size_t ld, Ld* L) {
    if (ld >= n) { *L = Ld(ld); return true; }
    if (ld < 128 || (ld & (ld - 1)) != 0) return false;
    *L = Ld(ld, (unsigned)__builtin_ctzll((unsigned long long)ld));
    return true;
}
}  // namespace

extern "C" {

int modarith_amd_w32_field_info(const char* prime, int* nlimbs, int* radix, int* nbits, int* nbytes, int* montgomery) {
    struct Row { const char* name; int nl, rx, nb, by, mo; };
    static const Row rows[] = {
#include "generated/w32_field_table.inc"
    };
    for (const Row& r : rows) {
        if (strcmp(prime, r.name) == 0) {
            if (nlimbs) *nlimbs = r.nl;
            if (radix) *radix = r.rx;
            if (nbits) *nbits = r.nb;
            if (nbytes) *nbytes = r.by;
            if (montgomery) *montgomery = r.mo;
            return 1;
        }
    }
    return 0;
}
size_t modarith_amd_w32_batch_words(size_t n, int nlimbs, size_t ld) {
    if (nlimbs < 1 || ld == 0) return 0;
    if (ld >= n) return (size_t)nlimbs * ld;                       // flat
    return (n + ld - 1) / ld * ld * (size_t)nlimbs;               // whole tiles
}
int modarith_amd_w32_aos_to_soa(const ma_spint32* aos, ma_spint32* soa, size_t n, int nlimbs, size_t ld, void* stream) {
    if (n == 0) return 0;
    Ld L;
    if (nlimbs < 1 || nlimbs > 64 || !conv_ld(n, ld, &L)) { ma::set_error("w32_aos_to_soa: need 1 <= nlimbs <= 64 and ld >= n (flat) or ld a power of two >= 128 (tiles)"); return (int)hipErrorInvalidValue; }
    k_aos2soa<<<ma::grid_for(n), BLOCK, 0, (hipStream_t)stream>>>(aos, soa, n, nlimbs, L);
    return ma::check_launch("w32_aos_to_soa");
}
int modarith_amd_w32_soa_to_aos(const ma_spint32* soa, ma_spint32* aos, size_t n, int nlimbs, size_t ld, void* stream) {
    if (n == 0) return 0;
    Ld L;
    if (nlimbs < 1 || nlimbs > 64 || !conv_ld(n, ld, &L)) { ma::set_error("w32_soa_to_aos: need 1 <= nlimbs <= 64 and ld >= n (flat) or ld a power of two >= 128 (tiles)"); return (int)hipErrorInvalidValue; }
    k_soa2aos<<<ma::grid_for(n), BLOCK, 0, (hipStream_t)stream>>>(soa, aos, n, nlimbs, L);
    return ma::check_launch("w32_soa_to_aos");
}

}  // extern "C"
