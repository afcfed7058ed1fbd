// modarith_amd/csrc/capi_w32.inc -- per-prime body of the C-ABI shim of the 32-bit word form.  Included by capi_<PRIME>_w32.hip
// with MA_P (parameter struct, csrc/generated/w32_<PRIME>.h) and MA_NAME (token) defined.  Every entry point declared by
// MODARITH_AMD_DECLARE_W32(P) in include/modarith_amd_w32.h is defined here: <fn>_<PRIME>_w32_batch (device pointers, limb-
// interleaved uint32_t batches, argument order of the 64-bit _batch forms) and <fn>_<PRIME>_w32_ct (the reference's signatures over
// uint32_t, host pointers, one element through the device) -- here or in capi_field.inc, the part shared with the 64-bit form
// (capi_prime.inc).  This file keeps the two knobs of the streaming kernels and the entry points with ONE product policy where the
// 64-bit form chooses between several.
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
using namespace ma;             // (the host helpers of capi_common.h: this translation unit has no 64-bit kernels)
using P = MA_P;
constexpr int NL = P::N;
constexpr int NB = P::NBYTES;
#define MA_WHAT(fn) fn "(w32)"
#define MA_WHAT2(fn, how) fn "(w32, " how ")"
// Launch shape of the streaming kernels (k_binary, k_unary, k_mli): elements per lane -- four (16 bytes, global_load/store_dwordx4),
// two (8 bytes) or one (4 bytes) -- and workgroup size.  Every width is compiled for every prime, none with scratch or accumulation
// registers (the widest: 95 VGPRs for the 9-limb modmul at four elements per lane, 163 for the 16-limb one).  The default is the
// MEASURED choice (tools/w32_rate.py, profiles/w32_rate.json, docs/kernels_field.md 4.5): on tiles of 4096 at 2^24 elements ONE
// element per lane in workgroups of 256 streamed best for modmul and modsqr of all three primes -- 0.79-0.82 of the HBM peak against
// 0.77-0.80 at two and 0.75-0.79 at four elements per lane -- so the wider accesses are kept as alternatives, not used by default.
// MA_W32_EPT=1|2|4 raises the widest access the library may take and MA_W32_BLOCK=64|128|256|512 sets the workgroup size, for the
// calls that follow (read at every call): testing and measuring knobs, like MA_FORCE_EXACT of the 64-bit form.  Same words on every path.
// A generated unit (modarith_amd/generate.py generate_w32) defines MA_W32_EPT_MAX, the widest width its limb count leaves without
// scratch or accumulation registers (four up to 16 limbs, two for 17 and 18: docs/kernels_field.md 4.5); wider requests are clamped
// to it and the wider kernels are not compiled (capi_field.inc EPT_COMPILED).
constexpr int EPT_DEFAULT = 1;
int ept_cap() {                  // (read at every call: tools/w32_rate.py measures the widths side by side in one process)
    const char* e = getenv("MA_W32_EPT");
    const int x = e ? atoi(e) : 0;
    const int cap = (x == 1 || x == 2 || x == 4) ? x : EPT_DEFAULT;
#ifdef MA_W32_EPT_MAX
    static_assert(MA_W32_EPT_MAX == 1 || MA_W32_EPT_MAX == 2 || MA_W32_EPT_MAX == 4, "MA_W32_EPT_MAX is 1, 2 or 4");
    return cap < MA_W32_EPT_MAX ? cap : MA_W32_EPT_MAX;
#else
    return cap;
#endif
}

// workgroup size of the streaming kernels (MA_W32_BLOCK=64|128|256 overrides it for a process, like MA_W32_EPT)
constexpr int STREAM_BLOCK_DEFAULT = 256;
int stream_block() {
    const char* e = getenv("MA_W32_BLOCK");
    const int x = e ? atoi(e) : 0;
    return (x == 64 || x == 128 || x == 256 || x == 512) ? x : STREAM_BLOCK_DEFAULT;
}

// Whether elements of a large batch may share an inversion (kernels.h k_inv_simul).  The admission predicate inv_in_contract is
// justified prime by prime: by hand for the three built-in primes (the comment above it), by the driver for a generated one
// (modarith_amd/params.py w32_inv_closure, which writes its verdict into the parameter struct as INV_CLOSED).  A struct without the
// member is a built-in one; a generated prime whose closure the driver could not show keeps one inversion per element at every
// batch size -- the same words, under the launch name "modinv(w32)" -- and does not compile the shared kernel at all.
template <class Q, class = void> struct inv_closed_of : std::true_type {};
template <class Q> struct inv_closed_of<Q, std::void_t<decltype(Q::INV_CLOSED)>> : std::bool_constant<Q::INV_CLOSED> {};
constexpr bool INV_SIMUL = inv_closed_of<P>::value;   // (thresholds and dispatch of the 64-bit form: capi_field.inc)
}  // namespace
#include "capi_field.inc"

namespace {
int modinv_each(const spint* x, spint* z, size_t n, size_t ld, void* st) { return launch_unary_heavy<OpInv<P>>(x, z, n, ld, st, "modinv(w32)"); }
bool inv_may_share() { return INV_SIMUL; }
}  // namespace

extern "C" {

// ------------------------------------------------------------------ batched form: the entry points that choose a product policy at 64 bits
int BATCH(modmul)(const ma_spint32* a, const ma_spint32* b, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_binary<OpMul<P>>(a, b, c, n, ld, st, "modmul(w32)"); }
int BATCH(modsqr)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpSqr<P>>(a, c, n, ld, st, "modsqr(w32)"); }
int BATCH(nres)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpNres<P>>(a, c, n, ld, st, "nres(w32)"); }
int BATCH(redc)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary<OpRedc<P>>(a, c, n, ld, st, "redc(w32)"); }
int BATCH(modpro)(const ma_spint32* a, ma_spint32* c, size_t n, size_t ld, void* st) { return launch_unary_heavy<OpPro<P>>(a, c, n, ld, st, "modpro(w32)"); }

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

}  // extern "C"
