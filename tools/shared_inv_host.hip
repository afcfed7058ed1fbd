// tools/shared_inv_host.hip -- the shared inversion (csrc/shared_inv.h) with each of its four item policies, compiled for the HOST: every
// lane of a small batch through the shared form, every output word against the UNSHARED form -- F::invert of that item's own
// denominator, the same numerator products, the same to_words -- for exact equality.  Shapes: the smallest at which the walk can go
// wrong (one item; a ragged last group; full columns; the deepest column the host side asks for), L and rounds given directly; zero
// denominators at the first, a middle, the last valid and all items of one lane's column: the zero item must leave as its caller's
// answer for zero and every other item as if it were alone.  Operands: a fixed splitmix64 stream, canonical words for fe26 / fe28,
// outputs of F::mul for fm26 / fk26 (the limb bounds their producers keep).  Test tooling, not product code; no GPU, no oracle.
//   hipcc -O1 -g -std=c++17 --offload-host-only -fsanitize=address,undefined -fno-sanitize-recover=all tools/shared_inv_host.hip -o /tmp/shared_inv_host
// exit code 0 = all equal (tests/test_shared_inv_host.py)
#define MA_DEV __host__ __device__ inline
#include "../modarith_amd/csrc/fe26.h"
#include "../modarith_amd/csrc/fe28.h"
#include "../modarith_amd/csrc/fm26.h"
#include "../modarith_amd/csrc/fk26.h"
#include "../modarith_amd/csrc/wn_export.h"
#include "../modarith_amd/csrc/wn_affine.h"
#include <stdio.h>
#include <vector>

static uint64_t sm_state = 0x5eed1e55;
static uint64_t sm() {
    uint64_t z = (sm_state += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// records (or table records) m, lanes L, rounds
struct Shape { size_t m, L; int rounds; };
static const Shape SHAPES[] = {{1, 1, 1}, {5, 2, 3}, {6, 2, 3}, {64, 2, 32}};
// where the zero denominators of lane jz's column go: item i of its nv valid ones
enum Place { FIRST, MIDDLE, LAST, ALL, NONE, PLACES };
static bool zero_at(int place, int i, int nv) {
    return place == FIRST ? i == 0 : place == MIDDLE ? i == nv / 2 : place == LAST ? i == nv - 1 : place == ALL;
}
// a column of one item has one place for a zero: MIDDLE, LAST and ALL would repeat FIRST and are not run (nor counted)
static bool repeats(int place, int nv) { return nv == 1 && (place == MIDDLE || place == LAST || place == ALL); }
static int differ(const char* what, const char* form, const Shape& s, size_t jz, int place, size_t e) {
    printf("%s %s: m %zu L %zu rounds %d, zeros of lane %zu at place %d: item %zu differs\n", what, form, s.m, s.L, s.rounds, jz, place, e);
    return 1;
}

// ---- fe26 / fe28: k_fe_finish (one numerator, in the output record) and k_fe_batch_div (two, to SinkWords)
template <class F, int NL, int NW, int TOPBITS>
static int fe_cases(const char* name) {
    int bad = 0, cases = 0;
    auto canon = [](uint64_t* w) {
        uint64_t r[NW];
        uint32_t f[NL];
        for (int k = 0; k < NW; k++) r[k] = sm();
        if (TOPBITS < 64) r[NW - 1] &= (1ull << TOPBITS) - 1;
        F::from_words(r, f);
        F::to_words(f, w);
    };
    for (const Shape& s : SHAPES)
        for (size_t jz = 0; jz < s.L; jz++)
            for (int place = 0; place < PLACES; place++) {
                const size_t m = s.m;
                std::vector<uint64_t> A(NW * m), B(NW * m), C(NW * m), bv(NW * m), want(3 * NW * m);
                std::vector<uint32_t> wc(NL * m);
                for (size_t e = 0; e < m; e++) {
                    uint64_t w[4][NW];
                    for (int q = 0; q < 4; q++) canon(w[q]);
                    for (int k = 0; k < NW; k++) { A[k * m + e] = w[0][k]; B[k * m + e] = w[1][k]; C[k * m + e] = w[2][k]; bv[e * NW + k] = w[3][k]; }
                }
                int nv = 0;
                for (int r = 0; r < s.rounds; r++) nv += (size_t)r * s.L + jz < m;
                if (repeats(place, nv)) continue;
                cases++;
                for (int r = 0; r < nv; r++)
                    if (zero_at(place, r, nv))
                        for (int k = 0; k < NW; k++) A[k * m + (size_t)r * s.L + jz] = 0;
                // the unshared form: want[q][e][k], q = B / A, C / A, bv / A
                for (size_t e = 0; e < m; e++) {
                    uint64_t zw[NW], any = 0;
                    for (int k = 0; k < NW; k++) any |= zw[k] = A[k * m + e];
                    uint32_t z[NL], inv[NL];
                    F::from_words(zw, z);
                    F::invert(z, inv);
                    for (int q = 0; q < 3; q++) {
                        uint64_t xw[NW], ow[NW];
                        uint32_t x[NL];
                        for (int k = 0; k < NW; k++) xw[k] = q == 0 ? B[k * m + e] : q == 1 ? C[k * m + e] : bv[e * NW + k];
                        F::from_words(xw, x);
                        F::mul(x, inv, x);
                        F::to_words(x, ow);
                        for (int k = 0; k < NW; k++) want[(q * m + e) * NW + k] = any ? ow[k] : 0;          // zero -> 0
                    }
                }
                for (size_t j = 0; j < s.L; j++) ma::FeFinish<F, NL, NW>::run(bv.data(), A.data(), wc.data(), m, s.L, s.rounds, j);
                ma::SinkWords<NW> sink{B.data(), C.data(), m};
                for (size_t j = 0; j < s.L; j++) ma::FeBatchDiv<F, NL, NW>::run(A.data(), B.data(), C.data(), wc.data(), m, s.L, s.rounds, j, sink);
                for (size_t e = 0; e < m; e++)
                    for (int k = 0; k < NW; k++) {
                        if (bv[e * NW + k] != want[(2 * m + e) * NW + k]) { bad += differ(name, "finish", s, jz, place, e); break; }
                        if (B[k * m + e] != want[e * NW + k] || C[k * m + e] != want[(m + e) * NW + k]) { bad += differ(name, "batch_div", s, jz, place, e); break; }
                    }
            }
    printf("%s finish + batch_div: %d cases, %d differ\n", name, cases, bad);
    return bad;
}

// ---- fm26 / fk26: an element as its producers leave it (the output of a product of tight limbs), and a zero mod p in either spelling
template <class F>
static void mul_output(int32_t* r) {
    int32_t a[10], b[10];
    for (int i = 0; i < 10; i++) { a[i] = (int32_t)(sm() & F::M26); b[i] = (int32_t)(sm() & F::M26); }
    F::mul(a, b, r);
}
template <class F>
static void zero_mod_p(int32_t* r, bool as_p) {
    for (int i = 0; i < 10; i++) r[i] = as_p ? F::prime(i) : 0;
}
template <class F>
static bool is_zero(const int32_t* z) {
    uint64_t zw[4];
    F::to_words(z, zw);
    return (zw[0] | zw[1] | zw[2] | zw[3]) == 0;
}

// k_wn_export: x = X / Z, y = Y / Z; zero -> (0, 1)
template <class F>
static int export_cases(const char* name) {
    int bad = 0, cases = 0;
    for (const Shape& s : SHAPES)
        for (size_t jz = 0; jz < s.L; jz++)
            for (int place = 0; place < PLACES; place++) {
                const size_t m = s.m;
                std::vector<uint64_t> buf(20 * m), want(8 * m), got(8 * m);
                std::vector<int> seen(m);
                ma::WnExpWs ws(buf.data(), m);
                int nv = 0;
                for (int r = 0; r < s.rounds; r++) nv += (size_t)r * s.L + jz < m;
                if (repeats(place, nv)) continue;
                cases++;
                for (size_t t = 0; t < m; t++) {
                    int32_t x[10], y[10], z[10];
                    mul_output<F>(x);
                    mul_output<F>(y);
                    mul_output<F>(z);
                    if (t % s.L == jz && zero_at(place, (int)(t / s.L), nv)) zero_mod_p<F>(z, (t / s.L) & 1);
                    ws.store<F>(t, x, y, z);
                }
                for (size_t e = 0; e < m; e++) {
                    int32_t x[10], z[10], inv[10];
                    ws.load<F>(ws.Z, e, z);
                    const bool zero = is_zero<F>(z);
                    F::invert(z, inv);
                    ws.load<F>(ws.X, e, x);
                    F::mul(x, inv, x);
                    F::to_words(x, &want[8 * e]);
                    ws.load<F>(ws.Y, e, x);
                    F::mul(x, inv, x);
                    F::to_words(x, &want[8 * e + 4]);
                    if (zero)
                        for (int k = 0; k < 8; k++) want[8 * e + k] = k == 4;
                }
                auto sink = [&](size_t e, const uint64_t* xw, const uint64_t* yw) {
                    seen[e]++;
                    for (int k = 0; k < 4; k++) { got[8 * e + k] = xw[k]; got[8 * e + 4 + k] = yw[k]; }
                };
                for (size_t j = 0; j < s.L; j++) ma::wn_export_lane<F>(ws, s.L, s.rounds, j, sink);
                for (size_t e = 0; e < m; e++)
                    for (int k = 0; k < 8; k++)
                        if (seen[e] != 1 || got[8 * e + k] != want[8 * e + k]) { bad += differ(name, "export", s, jz, place, e); break; }
            }
    printf("%s export: %d cases, %d differ\n", name, cases, bad);
    return bad;
}

// k_wn_table_affine: the entries of a window table to Z = 1 (x = X / Z^2, y = Y / Z^3, or X / Z, Y / Z); an entry with Z = 0 keeps its
// X, Y; flag bit 0 / 1 = entry 0 / 8 has Z = 0
template <class F, bool JAC>
static int table_cases(const char* name) {
    struct TShape { int ne, R; size_t m, L; };
    static const TShape TS[] = {{8, 1, 2, 2}, {8, 2, 3, 2}, {8, 4, 8, 2}, {16, 1, 2, 2}, {16, 2, 3, 2}};     // (m = 3: ragged)
    int bad = 0, cases = 0;
    for (const TShape& s : TS)
        for (size_t jz = 0; jz < s.L; jz++)
            for (int place = 0; place < PLACES; place++) {
                const size_t m = s.m;
                const int ne = s.ne;
                std::vector<uint64_t> buf((size_t)ne * 20 * m + (m + 1) / 2), want((size_t)ne * 8 * m);
                std::vector<uint32_t> wflag(m);
                ma::WnAffWs ws(buf.data(), m, ne);
                int nv = 0;
                for (int g = 0; g < ne * s.R; g++) nv += (size_t)(g / ne) * s.L + jz < m;
                if (repeats(place, nv)) continue;
                cases++;
                for (size_t t = 0; t < m; t++)
                    for (int e = 0; e < ne; e++) {
                        int32_t f[10];
                        for (int c = 0; c < 3; c++) {
                            mul_output<F>(f);
                            const int g = (int)(t / s.L) * ne + e;                          // the item this entry is in its lane's column
                            if (c == 2 && t % s.L == jz && zero_at(place, g, nv)) zero_mod_p<F>(f, g & 1);
                            ws.store<F>(e, c, t, f);
                        }
                    }
                for (size_t t = 0; t < m; t++)
                    for (int e = 0; e < ne; e++) {
                        int32_t x[10], z[10], zi[10], zx[10], zy[10];
                        ws.load<F>(e, 2, t, z);
                        const bool zero = is_zero<F>(z);
                        if (e == 0) wflag[t] = zero ? 1u : 0u;
                        if (e == 8) wflag[t] |= zero ? 2u : 0u;
                        F::invert(z, zi);
                        if (JAC) {
                            F::sqr(zi, zx);
                            F::mul(zx, zi, zy);
                        } else {
                            F::copy(zi, zx);
                            F::copy(zi, zy);
                        }
                        uint64_t* w = &want[((size_t)t * ne + e) * 8];
                        ws.load<F>(e, 0, t, x);
                        if (!zero) F::mul(x, zx, x);
                        F::to_words(x, w);
                        ws.load<F>(e, 1, t, x);
                        if (!zero) F::mul(x, zy, x);
                        F::to_words(x, w + 4);
                    }
                for (size_t j = 0; j < s.L; j++) ma::wn_table_affine_lane<F, JAC>(ws, s.L, s.R, j);
                for (size_t t = 0; t < m; t++) {
                    bool ok = ws.flag[t] == wflag[t];
                    for (int e = 0; e < ne; e++) {
                        int32_t x[10];
                        uint64_t w[8];
                        ws.load<F>(e, 0, t, x);
                        F::to_words(x, w);
                        ws.load<F>(e, 1, t, x);
                        F::to_words(x, w + 4);
                        for (int k = 0; k < 8; k++) ok = ok && w[k] == want[((size_t)t * ne + e) * 8 + k];
                    }
                    if (!ok) bad += differ(name, JAC ? "table (Jacobian)" : "table (homogeneous)", Shape{m, s.L, s.R}, jz, place, t);
                }
            }
    printf("%s table %s: %d cases, %d differ\n", name, JAC ? "(Jacobian)" : "(homogeneous)", cases, bad);
    return bad;
}

int main() {
    int bad = 0;
    bad += fe_cases<ma::Fe26, 10, 4, 63>("fe26");
    bad += fe_cases<ma::Fe28, 16, 7, 64>("fe28");
    bad += export_cases<ma::Fm26>("fm26");
    bad += export_cases<ma::Fk26>("fk26");
    bad += table_cases<ma::Fm26, true>("fm26");
    bad += table_cases<ma::Fm26, false>("fm26");
    printf("shared inversion on the host: %d differ\n", bad);
    return bad ? 1 : 0;
}
