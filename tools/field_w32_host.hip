// tools/field_w32_host.hip -- the 32-bit word form of csrc/field.h (MA_WL = 32: ma32::Field<P_<PRIME>_W32>, spint = uint32_t,
// dpint = uint64_t) compiled for the HOST into a shared library, so that tests/test_w32_host.py can run all 32 field functions of
// the three primes on every record of tests/golden/field_w32_<PRIME>.json.xz (the reference's emitted C at word length 32) and
// compare word for word, before any GPU is involved.  Test tooling, not product code.
//   hipcc -O1 -std=c++17 -w -shared -fPIC --offload-host-only -I modarith_amd/csrc/generated -I modarith_amd/csrc \
//         tools/field_w32_host.hip -o /tmp/libfield_w32_host.so
// One element per call: a, b inputs, o0 / o1 outputs (Nlimbs words each), k the integer argument, bytes a big-endian record of
// Nbytes, the function's integer result as the return value (0 for void functions; -1000 unknown prime, -1001 unknown function).
#define MA_WL 32
#define MA_DEV __host__ __device__ inline
#include <hip/hip_runtime.h>
// field.h's out-of-line chain primitives and the generated progenitor chains are declared __device__ only; for this host-only
// build they become host functions as well (as in tools/field_fast_host.hip)
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "../modarith_amd/csrc/field.h"
#include "w32_X25519.h"
#include "w32_NIST256.h"
#include "w32_X448.h"
#include <stddef.h>
#include <string.h>

namespace {
using ma32::spint;
using ma32::word_t;

template <class P>
long run(const char* fn, const spint* a, const spint* b, spint* o0, spint* o1, long k, unsigned char* bytes) {
    using F = ma32::Field<P>;
    constexpr int N = P::N, NB = P::NBYTES, NW = F::NW;
    spint x[N], y[N], z[N];
    for (int i = 0; i < N; i++) { x[i] = a ? a[i] : 7; y[i] = b ? b[i] : 7; z[i] = 7; }
    auto out = [&](spint* o, const spint* v) { for (int i = 0; i < N; i++) o[i] = v[i]; };
    auto is = [&](const char* s) { return strcmp(fn, s) == 0; };
    long r = 0;
    if (is("modadd")) { F::modadd(x, y, z); out(o0, z); }
    else if (is("modsub")) { F::modsub(x, y, z); out(o0, z); }
    else if (is("modmul")) { F::modmul(x, y, z); out(o0, z); }
    else if (is("modneg")) { F::modneg(x, z); out(o0, z); }
    else if (is("modsqr")) { F::modsqr(x, z); out(o0, z); }
    else if (is("modcpy")) { F::modcpy(x, z); out(o0, z); }
    else if (is("nres")) { F::nres(x, z); out(o0, z); }
    else if (is("redc")) { F::redc(x, z); out(o0, z); }
    else if (is("modpro")) { F::modpro(x, z); out(o0, z); }
    else if (is("modinv")) { F::modinv(x, b ? y : nullptr, z); out(o0, z); }
    else if (is("modsqrt")) { F::modsqrt(x, b ? y : nullptr, z); out(o0, z); }
    else if (is("modqr")) { r = F::modqr(b ? y : nullptr, x); }
    else if (is("prop")) { r = (long)F::prop(x); out(o0, x); }
    else if (is("flatten")) { r = (long)F::flatten(x); out(o0, x); }
    else if (is("modfsb")) { r = (long)F::modfsb(x); out(o0, x); }
    else if (is("modhaf")) { F::modhaf(x); out(o0, x); }
    else if (is("modnsqr")) { F::modnsqr(x, (int)k); out(o0, x); }
    else if (is("modmli")) { F::modmli(x, (int)k, z); out(o0, z); }
    else if (is("modshl")) { F::modshl((unsigned)k, x); out(o0, x); }
    else if (is("modshr")) { r = F::modshr((unsigned)k, x); out(o0, x); }
    else if (is("modint")) { F::modint((int)k, z); out(o0, z); }
    else if (is("mod2r")) { F::mod2r((unsigned)k, z); out(o0, z); }
    else if (is("modzer")) { F::modzer(z); out(o0, z); }
    else if (is("modone")) { F::modone(z); out(o0, z); }
    else if (is("modis1")) { r = F::modis1(x); }
    else if (is("modis0")) { r = F::modis0(x); }
    else if (is("modsign")) { r = F::modsign(x); }
    else if (is("modcmp")) { r = F::modcmp(x, y); }
    else if (is("modcmv")) { F::modcmv((int)k, x, y); out(o0, y); }
    else if (is("modcsw")) { F::modcsw((int)k, x, y); out(o0, x); out(o1, y); }
    else if (is("modexp")) {
        word_t w[NW];
        F::modexp_words(x, w);
        for (int B = 0; B < NB; B++) { const int pos = NB - 1 - B; bytes[B] = (unsigned char)(w[pos / 8] >> (8 * (pos % 8))); }
    } else if (is("modimp")) {
        word_t w[NW];
        for (int K = 0; K < NW; K++) w[K] = 0;
        for (int B = 0; B < NB; B++) { const int pos = NB - 1 - B; w[pos / 8] |= (word_t)bytes[B] << (8 * (pos % 8)); }
        r = F::modimp_words(w, z);
        out(o0, z);
    } else {
        return -1001;
    }
    return r;
}
}  // namespace

extern "C" long w32h_call(const char* prime, const char* fn, const uint32_t* a, const uint32_t* b, uint32_t* o0, uint32_t* o1, long k, unsigned char* bytes) {
    if (strcmp(prime, "X25519") == 0) return run<ma32::P_X25519_W32>(fn, a, b, o0, o1, k, bytes);
    if (strcmp(prime, "NIST256") == 0) return run<ma32::P_NIST256_W32>(fn, a, b, o0, o1, k, bytes);
    if (strcmp(prime, "X448") == 0) return run<ma32::P_X448_W32>(fn, a, b, o0, o1, k, bytes);
    return -1000;
}
// facts: Nlimbs, Radix, Nbits, Nbytes, Montgomery, sizeof(spint)
extern "C" int w32h_facts(const char* prime, int* out) {
#define W32H_X(T) if (strcmp(prime, #T) == 0) { using P = ma32::P_##T##_W32; const int v[] = {P::N, P::RADIX, P::NBITS, P::NBYTES, P::MONTGOMERY, (int)sizeof(ma32::spint)}; for (int i = 0; i < 6; i++) out[i] = v[i]; return 0; }
    W32H_X(X25519) W32H_X(NIST256) W32H_X(X448)
#undef W32H_X
    return -1;
}
