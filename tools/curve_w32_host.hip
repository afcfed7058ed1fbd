// tools/curve_w32_host.hip -- the curve layer at word length 32 (csrc/curve.h, edwards.h, weierstrass.h at MA_WL = 32) compiled for the
// HOST: the very classes the kernels of capi_<CURVE>_w32_ecn.hip wrap -- ma32::Edwards<C_ED25519_W32>, ma32::Weierstrass<C_NIST256_W32>,
// ma32::Edwards<C_ED448_W32> -- with MA_DEV = __host__ __device__, so that tests/test_w32_curve_host.py can run every record of
// tests/golden/curveref_w32_<CURVE>.json.xz (the reference's emitted C at word length 32) through them limb for limb before any GPU is
// involved.  The scalar multiplications run exactly as in k_ed_mul / k_ed_mul2x: recode / jsf_digits into a digit column of stride
// 64, the window table in a one-wave slab (lane 0), CurveOps::mul / mul2_exact.  Test tooling, not product code.
//   hipcc -O1 -std=c++17 -w --offload-host-only -I modarith_amd/csrc/generated -I modarith_amd/csrc tools/curve_w32_host.hip -o curve_w32_host
// A stand-alone program: it reads one request per line on standard input --
//   <CURVE> <fn> <P: 3*N hex limbs> <Q: 3*N hex limbs> <e: Nbytes hex> <f: Nbytes hex> <s>
// and answers each with one line: the function's integer result followed by the 3*N limbs of the resulting point.
#define MA_WL 32
#define MA_DEV __host__ __device__ inline
#include <hip/hip_runtime.h>
// field.h's out-of-line chain primitives, the generated progenitor chains and the record helpers of kernels.h are declared __device__
// only; for this host-only build they become host functions as well (as in tools/field_w32_host.hip)
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "w32_curve_ED25519.h"
#include "w32_curve_NIST256.h"
#include "w32_curve_ED448.h"
#include "../modarith_amd/csrc/edwards.h"
#include "../modarith_amd/csrc/weierstrass.h"
#include "curve_w32_host_run.h"

int main() {
    static char line[1 << 16], curve[32], fn[32], ps[1 << 14], qs[1 << 14], es[256], fs[256];
    int s;
    while (fgets(line, sizeof line, stdin)) {
        if (sscanf(line, "%31s %31s %16383s %16383s %255s %255s %d", curve, fn, ps, qs, es, fs, &s) != 7) { printf("error parse\n"); return 2; }
        const int N = strcmp(curve, "ED448") == 0 ? 16 : 9, NB = strcmp(curve, "ED448") == 0 ? 56 : 32;
        spint P[48], Q[48];
        alignas(8) unsigned char e[56], f[56];
        if (!hex_words(ps, P, 3 * N) || !hex_words(qs, Q, 3 * N) || !hex_bytes(es, e, NB) || !hex_bytes(fs, f, NB)) { printf("error operand\n"); return 2; }
        long r;
        if (strcmp(curve, "ED25519") == 0) r = run<ma32::Edwards<ma32::C_ED25519_W32>>(fn, P, Q, e, f, s);
        else if (strcmp(curve, "NIST256") == 0) r = run<ma32::Weierstrass<ma32::C_NIST256_W32>>(fn, P, Q, e, f, s);
        else if (strcmp(curve, "ED448") == 0) r = run<ma32::Edwards<ma32::C_ED448_W32>>(fn, P, Q, e, f, s);
        else r = -1000;
        printf("%ld", r);
        for (int i = 0; i < 3 * N; i++) printf(" %x", P[i]);
        printf("\n");
    }
    return 0;
}
