// tools/field_w32_host_run.h -- one call of one field function of ma32::Field<P> on the host: the part of tools/field_w32_host.hip
// (the three built-in primes) that tools/field_w32_gen_host.hip (generated fields) uses as well.  Include after csrc/field.h at
// MA_WL = 32 and the parameter structs.  Test tooling, not product code.
// One element per call: a, b inputs, o0 / o1 outputs (Nlimbs words each), k the integer argument, bytes a big-endian record of
// Nbytes, the function's integer result as the return value (0 for void functions; -1001 unknown function).
#pragma once
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

