// tools/curve_w32_gen_host.hip -- tools/curve_w32_host.hip for GENERATED curves (modarith_amd.generate.generate_curve(..., wl=32)): the
// classes the kernels of a capi_curve_<CURVE>_w32.hip plug-in wrap, compiled for the HOST over the emitted w32_curve_<CURVE>.h, so that
// tests/test_w32_curve_gen_host.py can run every record of tests/golden/curveref_w32_<CURVE>.json.xz through them limb for limb before
// any GPU is involved.  The curves are named by a list file the caller writes next to the emitted headers (as tools/field_w32_gen_host.hip):
//     #include "w32_curve_SECP256K1.h"
//     ...
//     #define W32CG_CURVES(X) X(SECP256K1, Weierstrass) X(NUMS256E, Edwards) ...
//   hipcc -O1 -std=c++17 -w --offload-host-only -I modarith_amd/csrc/generated -I modarith_amd/csrc -I <dir of the list> \
//         -DW32CG_LIST='"curves.inc"' tools/curve_w32_gen_host.hip -o curve_w32_gen_host
// A stand-alone program with the request lines of tools/curve_w32_host.hip:
//   <CURVE> <fn> <P: 3*N hex limbs> <Q: 3*N hex limbs> <e: Nbytes hex> <f: Nbytes hex> <s>
// Test tooling, not product code.
#define MA_WL 32
#define MA_DEV __host__ __device__ inline
#include <hip/hip_runtime.h>
// (field.h's out-of-line chain primitives, the generated progenitor chains and the record helpers of kernels.h are declared __device__
// only: host functions as well here)
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include W32CG_LIST
#include "../modarith_amd/csrc/edwards.h"
#include "../modarith_amd/csrc/weierstrass.h"
#include "curve_w32_host_run.h"

namespace {
constexpr int MAXN = 18, MAXNB = 72;

template <class E>
int one(const char* fn, const char* ps, const char* qs, const char* es, const char* fs, int s) {
    constexpr int N = E::N, NB = E::NB;
    static_assert(N <= MAXN && NB <= MAXNB, "operand buffers");
    spint P[3 * MAXN], Q[3 * MAXN];
    alignas(8) unsigned char e[MAXNB], f[MAXNB];
    if (!hex_words(ps, P, 3 * N) || !hex_words(qs, Q, 3 * N) || !hex_bytes(es, e, NB) || !hex_bytes(fs, f, NB)) { printf("error operand\n"); return 2; }
    const long r = run<E>(fn, P, Q, e, f, s);
    printf("%ld", r);
    for (int i = 0; i < 3 * N; i++) printf(" %x", P[i]);
    printf("\n");
    return 0;
}
}  // namespace

int main() {
    static char line[1 << 16], curve[32], fn[32], ps[1 << 14], qs[1 << 14], es[256], fs[256];
    int s;
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%31s %31s %16383s %16383s %255s %255s %d", curve, fn, ps, qs, es, fs, &s) != 7) { printf("error parse\n"); return 2; }
        int rc = -1;
#define W32CG_X(C, K) if (rc < 0 && strcmp(curve, #C) == 0) rc = one<ma32::K<ma32::C_##C##_W32>>(fn, ps, qs, es, fs, s);
        W32CG_CURVES(W32CG_X)
#undef W32CG_X
        if (rc < 0) { printf("error curve\n"); return 2; }
        if (rc) return rc;
    }
    return 0;
}
