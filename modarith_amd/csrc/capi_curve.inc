// modarith_amd/csrc/capi_curve.inc -- C-ABI entry points of the batched curve layer (SURVEY 8 f1, f3).
// Included by capi_<CURVE>.hip with MA_CURVE_CLASS (ma::Edwards<...> or ma::Weierstrass<...>) and MA_CNAME
// (lower-case token used in the symbol names, as curve.py:344-345 substitutes XXX -> _<curve>_) defined.
// MA_CURVE_PART splits the unit for the build (the two scalar-multiplication kernels dominate compile time and are
// compiled in parallel): 1 = only ecn_<c>_mul_batch, 2 = only ecn_<c>_mul2_batch, 3 = everything else; undefined = all.
//
// One body for both word lengths (csrc/curve.h): a capi_<CURVE>_w32.hip unit includes generated/w32_curve_<CURVE>.h (MA_WL = 32,
// classes in ma32) and defines MA_CNAME <c>_w32, which names the entry points of include/modarith_amd_w32_curve.h --
// ecn_<c>_w32_<fn>[_batch] over uint32_t limbs, ma_point_<c>_w32_t.  There the field is exact for every limb pattern (one launch, no
// vote), and mul2 IS the reference's own walk: there is no separate mul2_exact.
#if MA_WL == 32
#include "../../include/modarith_amd_w32_curve.h"
typedef ma_spint32 ma_limb;
#define EB_MUL2_WALK EB(mul2)
#else
#include "../../include/modarith_amd.h"
typedef ma_spint ma_limb;
#define EB_MUL2_WALK EB(mul2_exact)
#endif
#include "capi_common.h"
#include "edwards.h"
#include "weierstrass.h"
#include <string.h>

#define MA_ECAT_(a, b, c) a##_##b##_##c
#define MA_ECAT(a, b, c) MA_ECAT_(a, b, c)
#define EB(fn) MA_ECAT(ecn, MA_CNAME, fn##_batch)
#define ES(fn) MA_ECAT(ecn, MA_CNAME, fn)
#define EPOINT MA_ECAT(ma_point, MA_CNAME, t)

// MA_CURVE_MUL_CLASS: the class the three scalar-multiplication kernels are built from -- the same curve on a resident form of
// its field (csrc/fh51.h) where one exists; everything else (and the table / workspace geometry, which is the same) uses
// MA_CURVE_CLASS.  MA_MUL_WPS (curve.h) may be defined by the unit before its includes.
#ifndef MA_CURVE_MUL_CLASS
#define MA_CURVE_MUL_CLASS MA_CURVE_CLASS
#endif

namespace {
using namespace MA_NS;
using namespace ma;             // (the host helpers of capi_common.h)
using E = MA_CURVE_CLASS;
using EM = MA_CURVE_MUL_CLASS;
static_assert(EM::TABLE_WORDS == E::TABLE_WORDS && EM::N == E::N && EM::NB == E::NB, "the multiplication class is the same curve");
// the limb contract (curve.h): where EM's field is not exact for every 64-bit limb pattern, the scalar multiplications are two launches --
// EM with the vote at point load, then EX (the same curve on Field<P, false>) for the passes EM left alone
using EX = typename exact_class<EM>::type;
constexpr bool GUARDED = !field_is_exact<typename EM::F>::value;
static_assert(MA_WL == 64 || !GUARDED, "the 32-bit field has one product policy, exact for every limb pattern");
static_assert(EX::TABLE_WORDS == EM::TABLE_WORDS && EX::SLAB_WORDS == EM::SLAB_WORDS && EX::NDIG == EM::NDIG, "the exact class shares the table geometry");
constexpr int NL = E::N;
constexpr int NB = E::NB;
constexpr size_t MUL_BLOCK = 64;
// resident grid of the scalar multiplications: 4 SIMDs x MA_MUL_WPS waves on each of the 256 CUs; the window-table
// workspace is sized to it (one 9-entry table per lane is what ecn mul touches: 141 MB for 5-limb fields and 226 MB for ED448 at
// two waves per SIMD, inside the 256 MiB Infinity Cache; 283 MB for ED25519 at its four waves)
constexpr size_t MUL_MAX_LANES = (size_t)(4 * MA_MUL_WPS) * 256 * MUL_BLOCK;

// byte records are moved as 64-bit words when Nbytes is a multiple of 8 (then they must be 8-byte aligned), byte by
// byte otherwise (the 66-byte NIST521 records)
inline bool rec_aligned(const void* p) { return (E::NB % 8 != 0) || (reinterpret_cast<uintptr_t>(p) & 7u) == 0; }

// grid of the exact class behind a fast scalar multiplication (curve.h "the limb contract"): ONE wave per CU.  For every legitimate batch
// it only reads the points, votes and leaves (20 us for 2^20 points); a full resident grid of this 190-250-register kernel -- 3 072 waves
// that exit at once -- made the NEXT launch of the fast kernel 18 % slower on P-256 / secp256k1 (16.5 -> 19.7 ms, same box, same code:
// profiles/r06_limb_guard.log; an empty kernel or the vote alone on that grid does not, nor does this kernel on 256 waves).
unsigned exact_grid(size_t lanes) { const size_t w = lanes / MUL_BLOCK; return (unsigned)(w < 256 ? w : 256); }

size_t mul_lanes(size_t n) {
    size_t lanes = (n + MUL_BLOCK - 1) / MUL_BLOCK * MUL_BLOCK;
    return lanes < MUL_MAX_LANES ? lanes : MUL_MAX_LANES;
}

using EStage = StageBase;

template <int OP>
int launch_op(const spint* Q, spint* P, size_t n, size_t ld, void* st, const char* what) {
    if (n == 0) return 0;
    k_ed_op<E, OP><<<grid_for(n), BLOCK, 0, (hipStream_t)st>>>(Q, P, n, ld);
    return check_launch(what);
}
}  // namespace

extern "C" {

#if !defined(MA_CURVE_PART) || MA_CURVE_PART == 3
size_t ES(mul_workspace_bytes)(size_t n) { return mul_lanes(n) * E::TABLE_BYTES; }
#endif

#if !defined(MA_CURVE_PART) || MA_CURVE_PART == 1
int EB(mul)(const char* e, ma_limb* P, size_t n, size_t ld, void* workspace, size_t workspace_bytes, void* st) {
    if (n == 0) return 0;
    const size_t lanes = mul_lanes(n);
    if (workspace == nullptr || workspace_bytes < lanes * E::TABLE_BYTES) {
        set_error("ecn mul: workspace too small (see ecn_<curve>_mul_workspace_bytes)");
        return (int)hipErrorInvalidValue;
    }
    if (!rec_aligned(e)) { set_error("ecn mul: scalar records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    const unsigned char* eb = reinterpret_cast<const unsigned char*>(e);
    spint* ws = reinterpret_cast<spint*>(workspace);
    if constexpr (GUARDED) {
        k_ed_mul<EM, 1><<<(unsigned)(lanes / MUL_BLOCK), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, n, ld, ws);
        k_ed_mul<EX, -1><<<exact_grid(lanes), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, n, ld, ws);       // (reads the points again and leaves at once where the vote passes)
    } else {
        k_ed_mul<EM><<<(unsigned)(lanes / MUL_BLOCK), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, n, ld, ws);
    }
    return check_launch("ecn mul");
}
#endif
#if (!defined(MA_CURVE_PART) || MA_CURVE_PART == 2) && MA_WL == 64
int EB(mul2)(const char* e, const ma_limb* P, const char* f, const ma_limb* Q, ma_limb* R, size_t n, size_t ld,
             void* workspace, size_t workspace_bytes, void* st) {
    if (n == 0) return 0;
    const size_t lanes = mul_lanes(n);
    if (workspace == nullptr || workspace_bytes < lanes * E::TABLE_BYTES) {
        set_error("ecn mul2: workspace too small (see ecn_<curve>_mul_workspace_bytes)");
        return (int)hipErrorInvalidValue;
    }
    if (!rec_aligned(e) || !rec_aligned(f)) { set_error("ecn mul2: scalar records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    const unsigned char *eb = reinterpret_cast<const unsigned char*>(e), *fb = reinterpret_cast<const unsigned char*>(f);
    spint* ws = reinterpret_cast<spint*>(workspace);
    if constexpr (GUARDED) {
        k_ed_mul2<EM, 1><<<(unsigned)(lanes / MUL_BLOCK), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, fb, Q, R, n, ld, ws);
        k_ed_mul2<EX, -1><<<exact_grid(lanes), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, fb, Q, R, n, ld, ws);       // (reads the points again and leaves at once where the vote passes)
    } else {
        k_ed_mul2<EM><<<(unsigned)(lanes / MUL_BLOCK), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, fb, Q, R, n, ld, ws);
    }
    return check_launch("ecn mul2");
}
#endif
#if !defined(MA_CURVE_PART) || MA_CURVE_PART == 2
// the same with the reference's own joint-sparse-form walk (csrc/curve.h mul2_exact): the reference's projective limbs, variable time
int EB_MUL2_WALK(const char* e, const ma_limb* P, const char* f, const ma_limb* Q, ma_limb* R, size_t n, size_t ld,
             void* workspace, size_t workspace_bytes, void* st) {
    if (n == 0) return 0;
    const size_t lanes = mul_lanes(n);
    if (workspace == nullptr || workspace_bytes < lanes * E::TABLE_BYTES) {
        set_error("ecn mul2_exact: workspace too small (see ecn_<curve>_mul_workspace_bytes)");
        return (int)hipErrorInvalidValue;
    }
    if (!rec_aligned(e) || !rec_aligned(f)) { set_error("ecn mul2_exact: scalar records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    const unsigned char *eb = reinterpret_cast<const unsigned char*>(e), *fb = reinterpret_cast<const unsigned char*>(f);
    spint* ws = reinterpret_cast<spint*>(workspace);
    if constexpr (GUARDED) {
        k_ed_mul2x<EM, 1><<<(unsigned)(lanes / MUL_BLOCK), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, fb, Q, R, n, ld, ws);
        k_ed_mul2x<EX, -1><<<exact_grid(lanes), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, fb, Q, R, n, ld, ws);       // (reads the points again and leaves at once where the vote passes)
    } else {
        k_ed_mul2x<EM><<<(unsigned)(lanes / MUL_BLOCK), (unsigned)MUL_BLOCK, 0, (hipStream_t)st>>>(eb, P, fb, Q, R, n, ld, ws);
    }
    return check_launch("ecn mul2_exact");
}
#endif
#if !defined(MA_CURVE_PART) || MA_CURVE_PART == 3
int EB(ran)(int r, ma_limb* P, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    k_ed_ran<E><<<grid_for(n), BLOCK, 0, (hipStream_t)st>>>(r, P, n, ld);
    return check_launch("ecn ran");
}
int EB(add)(const ma_limb* Q, ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_ADD>(Q, P, n, ld, st, "ecn add"); }
int EB(sub)(const ma_limb* Q, ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_SUB>(Q, P, n, ld, st, "ecn sub"); }
int EB(cpy)(const ma_limb* Q, ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_CPY>(Q, P, n, ld, st, "ecn cpy"); }
int EB(dbl)(ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_DBL>(nullptr, P, n, ld, st, "ecn dbl"); }
int EB(neg)(ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_NEG>(nullptr, P, n, ld, st, "ecn neg"); }
int EB(inf)(ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_INF>(nullptr, P, n, ld, st, "ecn inf"); }
int EB(gen)(ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_GEN>(nullptr, P, n, ld, st, "ecn gen"); }
int EB(cof)(ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_COF>(nullptr, P, n, ld, st, "ecn cof"); }
int EB(affine)(ma_limb* P, size_t n, size_t ld, void* st) { return launch_op<ED_AFFINE>(nullptr, P, n, ld, st, "ecn affine"); }

int EB(cmp)(const ma_limb* P, const ma_limb* Q, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    k_ed_pred<E, true><<<grid_for(n), BLOCK, 0, (hipStream_t)st>>>(P, Q, out, n, ld);
    return check_launch("ecn cmp");
}
int EB(isinf)(const ma_limb* P, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    k_ed_pred<E, false><<<grid_for(n), BLOCK, 0, (hipStream_t)st>>>(P, nullptr, out, n, ld);
    return check_launch("ecn isinf");
}
int EB(set)(const int* s, const char* x, const char* y, ma_limb* P, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    if (!rec_aligned(x) || !rec_aligned(y)) { set_error("ecn set: records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    const unsigned char* xw = reinterpret_cast<const unsigned char*>(x);
    const unsigned char* yw = reinterpret_cast<const unsigned char*>(y);
    hipStream_t hs = (hipStream_t)st;
    if (x && y) k_ed_set<E, 0><<<grid_for(n), BLOCK, 0, hs>>>(s, xw, yw, P, n, ld);
    else if (x) k_ed_set<E, 1><<<grid_for(n), BLOCK, 0, hs>>>(s, xw, nullptr, P, n, ld);
    else if (y) {
        if constexpr (E::HAS_Y_ONLY_SET) k_ed_set<E, 2><<<grid_for(n), BLOCK, 0, hs>>>(s, nullptr, yw, P, n, ld);
        else { set_error("ecn set: this curve form needs x (weierstrass.c:417-428)"); return (int)hipErrorInvalidValue; }
    } else { set_error("ecn set: x and y are both NULL"); return (int)hipErrorInvalidValue; }
    return check_launch("ecn set");
}
int EB(get)(ma_limb* P, char* x, char* y, int* sign, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    if (!rec_aligned(x) || !rec_aligned(y)) { set_error("ecn get: records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    k_ed_get<E><<<grid_for(n), BLOCK, 0, (hipStream_t)st>>>(P, reinterpret_cast<unsigned char*>(x), reinterpret_cast<unsigned char*>(y), sign, n, ld);
    return check_launch("ecn get");
}

// ------------------------------------------------------------------ scalar form (curve.h:13-29 signatures), n = 1
// A host `point` {x[N],y[N],z[N]} is exactly the SoA layout with ld = 1.
#define MA_ES_UN(fn)                                                                 \
    void ES(fn)(EPOINT* P) {                                                         \
        EStage s;                                                                    \
        spint* dp = (spint*)s.take(sizeof(EPOINT));                                  \
        s.h2d(dp, P, sizeof(EPOINT));                                          \
        if (!s.bad) s.check(EB(fn)(dp, 1, 1, nullptr), "ecn " #fn);                           \
        s.d2h(P, dp, sizeof(EPOINT));                                          \
    }
MA_ES_UN(dbl)
MA_ES_UN(neg)
MA_ES_UN(inf)
MA_ES_UN(gen)
MA_ES_UN(cof)
MA_ES_UN(affine)
#define MA_ES_BIN(fn)                                                                \
    void ES(fn)(EPOINT* Q, EPOINT* P) {                                              \
        EStage s;                                                                    \
        spint *dq = (spint*)s.take(sizeof(EPOINT)), *dp = (spint*)s.take(sizeof(EPOINT)); \
        s.h2d(dq, Q, sizeof(EPOINT));                                          \
        s.h2d(dp, P, sizeof(EPOINT));                                          \
        if (!s.bad) s.check(EB(fn)(dq, dp, 1, 1, nullptr), "ecn " #fn);                       \
        s.d2h(P, dp, sizeof(EPOINT));                                          \
    }
MA_ES_BIN(add)
MA_ES_BIN(sub)
MA_ES_BIN(cpy)
int ES(cmp)(EPOINT* P, EPOINT* Q) {
    EStage s;
    spint *dq = (spint*)s.take(sizeof(EPOINT)), *dp = (spint*)s.take(sizeof(EPOINT));
    int* dr = (int*)s.take(sizeof(int));
    s.h2d(dq, Q, sizeof(EPOINT));
    s.h2d(dp, P, sizeof(EPOINT));
    if (!s.bad) s.check(EB(cmp)(dp, dq, dr, 1, 1, nullptr), "ecn cmp");
    int r;
    s.d2h(&r, dr, sizeof(int));
    return s.answer(r);
}
int ES(isinf)(EPOINT* P) {
    EStage s;
    spint* dp = (spint*)s.take(sizeof(EPOINT));
    int* dr = (int*)s.take(sizeof(int));
    s.h2d(dp, P, sizeof(EPOINT));
    if (!s.bad) s.check(EB(isinf)(dp, dr, 1, 1, nullptr), "ecn isinf");
    int r;
    s.d2h(&r, dr, sizeof(int));
    return s.answer(r);
}
void ES(mul)(const char* e, EPOINT* P) {
    EStage s;
    spint* dp = (spint*)s.take(sizeof(EPOINT));
    char* de = (char*)s.take(NB);
    const size_t wsb = ES(mul_workspace_bytes)(1);
    void* ws = s.take(wsb);
    s.h2d(dp, P, sizeof(EPOINT));
    s.h2d(de, e, NB);
    if (!s.bad) s.check(EB(mul)(de, dp, 1, 1, ws, wsb, nullptr), "ecn mul");
    s.d2h(P, dp, sizeof(EPOINT));
}
void ES(mul2)(const char* e, EPOINT* P, const char* f, EPOINT* Q, EPOINT* R) {
    EStage s;
    spint *dp = (spint*)s.take(sizeof(EPOINT)), *dq = (spint*)s.take(sizeof(EPOINT)), *dr = (spint*)s.take(sizeof(EPOINT));
    char *de = (char*)s.take(NB), *df = (char*)s.take(NB);
    const size_t wsb = ES(mul_workspace_bytes)(1);
    void* ws = s.take(wsb);
    s.h2d(dp, P, sizeof(EPOINT));
    s.h2d(dq, Q, sizeof(EPOINT));
    s.h2d(de, e, NB);
    s.h2d(df, f, NB);
    // one element: no lanes to keep in step, so the scalar entry point -- the reference's own signature -- takes the reference's own
    // walk (mul2_exact) and returns the reference's limbs
    if (!s.bad) s.check(EB_MUL2_WALK(de, dp, df, dq, dr, 1, 1, ws, wsb, nullptr), "ecn mul2");
    s.d2h(R, dr, sizeof(EPOINT));
}
void ES(ran)(int r, EPOINT* P) {
    EStage s;
    spint* dp = (spint*)s.take(sizeof(EPOINT));
    s.h2d(dp, P, sizeof(EPOINT));
    if (!s.bad) s.check(EB(ran)(r, dp, 1, 1, nullptr), "ecn ran");
    s.d2h(P, dp, sizeof(EPOINT));
}
void ES(set)(int sgn, const char* x, const char* y, EPOINT* P) {
    EStage s;
    spint* dp = (spint*)s.take(sizeof(EPOINT));
    int* ds = (int*)s.take(sizeof(int));
    char *dx = nullptr, *dy = nullptr;
    s.h2d(ds, &sgn, sizeof(int));
    if (x) { dx = (char*)s.take(NB); s.h2d(dx, x, NB); }
    if (y) { dy = (char*)s.take(NB); s.h2d(dy, y, NB); }
    if (!x && !y) return;   /* edwards.c:347-366 does nothing in that case */
    if (!s.bad) s.check(EB(set)(ds, dx, dy, dp, 1, 1, nullptr), "ecn set");
    s.d2h(P, dp, sizeof(EPOINT));
}
int ES(get)(EPOINT* P, char* x, char* y) {
    EStage s;
    spint* dp = (spint*)s.take(sizeof(EPOINT));
    int* dr = (int*)s.take(sizeof(int));
    char *dx = x ? (char*)s.take(NB) : nullptr, *dy = y ? (char*)s.take(NB) : nullptr;
    s.h2d(dp, P, sizeof(EPOINT));
    if (!s.bad) s.check(EB(get)(dp, dx, dy, dr, 1, 1, nullptr), "ecn get");
    s.d2h(P, dp, sizeof(EPOINT));
    if (x) s.d2h(x, dx, NB);
    if (y) s.d2h(y, dy, NB);
    int r;
    s.d2h(&r, dr, sizeof(int));
    return s.answer(r);
}
#endif  // MA_CURVE_PART

}  // extern "C"
