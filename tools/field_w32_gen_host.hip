// tools/field_w32_gen_host.hip -- the 32-bit word form of csrc/field.h for GENERATED fields (modarith_amd.generate.generate_w32),
// compiled for the HOST into a shared library: tests/test_w32_gen_host.py runs all 32 field functions of every example on every
// record of tests/golden/field_w32gen_<TAG>.json.xz (the reference's emitted C at word length 32) and compares word for word, before
// any GPU is involved.  The fields are named by a list file the caller writes (one line per field, next to their emitted
// params_<TAG>_w32.h):
//     #include "params_2519_w32.h"
//     ...
//     #define W32G_FIELDS(X) X(2519) X(BP256) ...
//   hipcc -O1 -std=c++17 -w -shared -fPIC --offload-host-only -I modarith_amd/csrc/generated -I modarith_amd/csrc -I <dir of the list> \
//         -DW32G_LIST='"fields.inc"' tools/field_w32_gen_host.hip -o libfield_w32_gen_host.so
// Test tooling, not product code.
#define MA_WL 32
#define MA_DEV __host__ __device__ inline
#include <hip/hip_runtime.h>
// (field.h's out-of-line chain primitives and the generated progenitor chains are declared __device__ only: host functions as well here)
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "../modarith_amd/csrc/field.h"
#include W32G_LIST
#include "field_w32_host_run.h"

extern "C" long w32h_call(const char* prime, const char* fn, const uint32_t* a, const uint32_t* b, uint32_t* o0, uint32_t* o1, long k, unsigned char* bytes) {
#define W32G_X(T) if (strcmp(prime, #T) == 0) return run<ma32::P_##T##_W32>(fn, a, b, o0, o1, k, bytes);
    W32G_FIELDS(W32G_X)
#undef W32G_X
    return -1000;
}
// facts: Nlimbs, Radix, Nbits, Nbytes, Montgomery, sizeof(spint), INV_CLOSED (the driver's verdict on the shared inversion)
extern "C" int w32h_facts(const char* prime, int* out) {
#define W32G_X(T) if (strcmp(prime, #T) == 0) { using P = ma32::P_##T##_W32; const int v[] = {P::N, P::RADIX, P::NBITS, P::NBYTES, P::MONTGOMERY, (int)sizeof(ma32::spint), (int)P::INV_CLOSED}; for (int i = 0; i < 7; i++) out[i] = v[i]; return 0; }
    W32G_FIELDS(W32G_X)
#undef W32G_X
    return -1;
}
