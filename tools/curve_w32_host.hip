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
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

namespace {
using ma32::spint;
using ma32::word_t;

template <class E>
long run(const char* fn, spint* P, const spint* Q, const unsigned char* e, const unsigned char* f, int s) {
    using F = typename E::F;
    constexpr int N = E::N, NW = E::NW;
    typename E::Point p, q, r;
    F::from_limbs(P, p.x); F::from_limbs(P + N, p.y); F::from_limbs(P + 2 * N, p.z);
    F::from_limbs(Q, q.x); F::from_limbs(Q + N, q.y); F::from_limbs(Q + 2 * N, q.z);
    auto is = [&](const char* t) { return strcmp(fn, t) == 0; };
    auto out = [&](const typename E::Point& w) { F::to_limbs(w.x, P); F::to_limbs(w.y, P + N); F::to_limbs(w.z, P + 2 * N); };
    word_t ew[NW], fw[NW];
    ma32::load_be_record<typename E::P>(e, 0, ew);
    ma32::load_be_record<typename E::P>(f, 0, fw);
    std::vector<typename E::row_t> slab(E::SLAB_WORDS);
    const typename E::Table W{slab.data(), 0};
    long ret = 0;
    if (is("add")) { E::add(q, p); out(p); }
    else if (is("sub")) { E::sub(q, p); out(p); }
    else if (is("dbl")) { E::dbl(p); out(p); }
    else if (is("neg")) { E::neg(p); out(p); }
    else if (is("cof")) { E::cof(p); out(p); }
    else if (is("inf")) { E::inf(p); out(p); }
    else if (is("gen")) { E::gen(p); out(p); }
    else if (is("cpy")) { E::cpy(q, p); out(p); }
    else if (is("affine")) { E::affine(p); out(p); }
    else if (is("ran")) { E::ran(s, p); out(p); }
    else if (is("isinf")) ret = E::isinf(p);
    else if (is("cmp")) ret = E::cmp(p, q);
    else if (is("mul")) {
        std::vector<signed char> dg((size_t)E::NDIG * 64);
        E::recode(ew, dg.data());
        E::mul(dg.data(), p, W);
        out(p);
    } else if (is("mul2")) {
        std::vector<unsigned char> dj((size_t)E::JSF_BYTES * 64);
        E::jsf_digits(ew, fw, dj.data());
        E::mul2_exact(dj.data(), p, q, r, W);
        out(r);
    } else if (is("setxy") || is("setx") || is("sety")) {          // e, f carry the coordinate records x, y
        spint X[N], Y[N];
        (void)F::modimp_words(ew, X);
        (void)F::modimp_words(fw, Y);
        if (is("setxy")) E::template setxy<0>(s, X, Y, p);
        else if (is("setx")) E::template setxy<1>(s, X, nullptr, p);
        else if constexpr (E::HAS_Y_ONLY_SET) E::template setxy<2>(s, nullptr, Y, p);
        else return -1001;
        out(p);
    } else return -1001;
    return ret;
}

bool hex_words(const char* t, spint* v, int n) {
    for (int i = 0; i < n; i++) {
        char* end;
        v[i] = (spint)strtoul(t, &end, 16);
        if (end == t) return false;
        t = end;
        if (*t == ',') t++;
    }
    return true;
}
bool hex_bytes(const char* t, unsigned char* v, int n) {
    if ((int)strlen(t) != 2 * n) return false;
    for (int i = 0; i < n; i++) { unsigned x; if (sscanf(t + 2 * i, "%2x", &x) != 1) return false; v[i] = (unsigned char)x; }
    return true;
}
}  // namespace

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
