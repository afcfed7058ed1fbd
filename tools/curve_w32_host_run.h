// tools/curve_w32_host_run.h -- one request of tools/curve_w32_host.hip / tools/curve_w32_gen_host.hip: a function of the curve layer at
// word length 32 on a host-compiled curve class (ma32::Edwards<...> / ma32::Weierstrass<...>), and the hex parsing of a request line.
// Included after csrc/edwards.h and csrc/weierstrass.h.  Test tooling, not product code.
#pragma once
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

