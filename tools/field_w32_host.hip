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
#include "field_w32_host_run.h"

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
