/* include/modarith_amd_w32_curve.h -- the curve layer (curve.h of the reference) at word length 32.
 *
 * `curve.py 32 <CURVE>` builds edwards.c / weierstrass.c over the 32-bit field.c: a `point` is three arrays of uint32_t limbs --
 * 9 x 29 for ED25519, 9 x 29 in Montgomery form for NIST256, 16 x 28 in Montgomery form for ED448 (the fields of modarith_amd_w32.h:
 * X25519, NIST256, X448).  A caller who holds such points hands them to the entry points below; the projective limbs that come back
 * are the limbs of the reference's emitted C for EVERY 32-bit limb pattern, not only for limbs a field function returns
 * (tests/golden/curveref_w32_<CURVE>.json.xz): the 32-bit field has one product policy, exact for all inputs, so there is no limb
 * contract at this word length.  The functions that run an inversion or a square root (get, affine, set from one coordinate) return
 * the same field elements as the reference, normalised as at 64 bits.
 *
 *   ecn_<c>_w32_<fn>(...)        scalar form: the reference's signature over ma_point_<c>_w32_t, host pointers, one point through the GPU.
 *   ecn_<c>_w32_<fn>_batch(...)  batched form: DEVICE pointers, n points, the argument order of the 64-bit ecn_<c>_<fn>_batch forms
 *                                (modarith_amd.h).  A batch of points is [3][Nlimbs] limb rows of uint32_t at stride ld >= n:
 *                                P[(coord * Nlimbs + limb) * ld + j]; a host `point` is that layout with ld = 1.
 *
 * for <c> = ed25519, nist256, ed448.  Scalars and coordinates are big-endian byte records of Nbytes (32, 32, 56) bytes, 8-byte aligned,
 * exactly as at 64 bits: they do not depend on the word length.
 *   mul   the constant-time signed 4-bit fixed-window multiplication (edwards.c:435-482, weierstrass.c:494-543): the table is selected
 *         by lane predication, no branch or address depends on the scalar.  Workspace: ecn_<c>_w32_mul_workspace_bytes(n) bytes of
 *         device memory (window tables of the resident grid), caller-owned; a workspace that is NULL or too small is refused with an
 *         error status and no output is written.
 *   mul2  the reference's own walk over its joint sparse form (edwards.c:404-431, 486-510: "not constant time"), the counterpart of the
 *         64-bit ecn_<c>_mul2_exact_batch: the reference's limbs, variable time.  Same workspace.
 *   set   x and/or y may be NULL as at 64 bits (nist256: x is mandatory); s: device int[n] or NULL.  cof on nist256 is a no-op.
 * Not offered at this word length: the fused byte-output forms (mul_get, mulgen_get, mul2_get, mulgen2_get), which speak bytes on both
 * sides and are word-length independent.  Ownership, aliasing (add(P, P) and cpy(P, P) are allowed), errors, streams and threading: as
 * in modarith_amd.h.  MODARITH_AMD_ABI is unchanged by this header: nothing existing changed.
 */
#ifndef MODARITH_AMD_W32_CURVE_H
#define MODARITH_AMD_W32_CURVE_H

#include "modarith_amd_w32.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MODARITH_AMD_DECLARE_W32_CURVE(c, NL)                                                                                       \
    typedef struct { uint32_t x[NL], y[NL], z[NL]; } ma_point_##c##_w32_t;                                                          \
    /* ---------------- scalar form: curve.h:13-29 over uint32_t points, host pointers ---------------- */                          \
    int ecn_##c##_w32_get(ma_point_##c##_w32_t *P, char *x, char *y);                                                               \
    void ecn_##c##_w32_set(int s, const char *x, const char *y, ma_point_##c##_w32_t *P);                                           \
    void ecn_##c##_w32_inf(ma_point_##c##_w32_t *P);                                                                                \
    int ecn_##c##_w32_isinf(ma_point_##c##_w32_t *P);                                                                               \
    void ecn_##c##_w32_neg(ma_point_##c##_w32_t *P);                                                                                \
    void ecn_##c##_w32_add(ma_point_##c##_w32_t *Q, ma_point_##c##_w32_t *P);          /* P += Q */                                 \
    void ecn_##c##_w32_sub(ma_point_##c##_w32_t *Q, ma_point_##c##_w32_t *P);          /* P -= Q */                                 \
    void ecn_##c##_w32_dbl(ma_point_##c##_w32_t *P);                                                                                \
    void ecn_##c##_w32_gen(ma_point_##c##_w32_t *P);                                                                                \
    void ecn_##c##_w32_mul(const char *e, ma_point_##c##_w32_t *P);                                                                 \
    void ecn_##c##_w32_mul2(const char *e, ma_point_##c##_w32_t *P, const char *f, ma_point_##c##_w32_t *Q, ma_point_##c##_w32_t *R); \
    void ecn_##c##_w32_ran(int r, ma_point_##c##_w32_t *P);                                                                         \
    int ecn_##c##_w32_cmp(ma_point_##c##_w32_t *P, ma_point_##c##_w32_t *Q);                                                        \
    void ecn_##c##_w32_affine(ma_point_##c##_w32_t *P);                                                                             \
    void ecn_##c##_w32_cpy(ma_point_##c##_w32_t *Q, ma_point_##c##_w32_t *P);                                                       \
    void ecn_##c##_w32_cof(ma_point_##c##_w32_t *P);                                                                                \
    /* ---------------- batched form: device pointers, [3][NL] limb rows of uint32_t at stride ld ---------------- */               \
    size_t ecn_##c##_w32_mul_workspace_bytes(size_t n);                                                                             \
    int ecn_##c##_w32_mul_batch(const char *e, ma_spint32 *P, size_t n, size_t ld, void *workspace, size_t workspace_bytes,         \
                                void *stream);                                                                                      \
    int ecn_##c##_w32_mul2_batch(const char *e, const ma_spint32 *P, const char *f, const ma_spint32 *Q, ma_spint32 *R, size_t n,   \
                                 size_t ld, void *workspace, size_t workspace_bytes, void *stream);                                 \
    int ecn_##c##_w32_ran_batch(int r, ma_spint32 *P, size_t n, size_t ld, void *stream);                                           \
    int ecn_##c##_w32_add_batch(const ma_spint32 *Q, ma_spint32 *P, size_t n, size_t ld, void *stream);                             \
    int ecn_##c##_w32_sub_batch(const ma_spint32 *Q, ma_spint32 *P, size_t n, size_t ld, void *stream);                             \
    int ecn_##c##_w32_cpy_batch(const ma_spint32 *Q, ma_spint32 *P, size_t n, size_t ld, void *stream);                             \
    int ecn_##c##_w32_dbl_batch(ma_spint32 *P, size_t n, size_t ld, void *stream);                                                  \
    int ecn_##c##_w32_neg_batch(ma_spint32 *P, size_t n, size_t ld, void *stream);                                                  \
    int ecn_##c##_w32_inf_batch(ma_spint32 *P, size_t n, size_t ld, void *stream);                                                  \
    int ecn_##c##_w32_gen_batch(ma_spint32 *P, size_t n, size_t ld, void *stream);                                                  \
    int ecn_##c##_w32_cof_batch(ma_spint32 *P, size_t n, size_t ld, void *stream);                                                  \
    int ecn_##c##_w32_affine_batch(ma_spint32 *P, size_t n, size_t ld, void *stream);                                               \
    int ecn_##c##_w32_cmp_batch(const ma_spint32 *P, const ma_spint32 *Q, int *out, size_t n, size_t ld, void *stream);             \
    int ecn_##c##_w32_isinf_batch(const ma_spint32 *P, int *out, size_t n, size_t ld, void *stream);                                \
    int ecn_##c##_w32_set_batch(const int *s, const char *x, const char *y, ma_spint32 *P, size_t n, size_t ld, void *stream);      \
    int ecn_##c##_w32_get_batch(ma_spint32 *P, char *x, char *y, int *sign, size_t n, size_t ld, void *stream);

MODARITH_AMD_DECLARE_W32_CURVE(ed25519, 9)
MODARITH_AMD_DECLARE_W32_CURVE(nist256, 9)
MODARITH_AMD_DECLARE_W32_CURVE(ed448, 16)

#ifdef __cplusplus
}
#endif
#endif
