/* include/modarith_amd_w32.h -- the 32-bit word form (Wordlength 32) of libmodarith_amd.so's field API.
 *
 * The reference generators take the word length as their first argument: `pseudo.py 32 X25519`, `monty.py 32 NIST256` and
 * `monty.py 32 X448` emit a field.c with spint = uint32_t and dpint = uint64_t -- 9 x 29-bit limbs for 2^255-19, 9 x 29 in
 * Montgomery form (R = 2^261) for P-256, 16 x 28 in Montgomery form (R = 2^476, virtual limb) for 2^448-2^224-1 -- and this is the
 * form the reference itself runs on a GPU (simd/pseudo_cuda.py, monty_cuda.py: field.cu).  A caller who holds uint32_t limb
 * arrays of that form hands them to the entry points below; the words that come back are the words of the reference's emitted C
 * for EVERY input, non-canonical limbs included (tests/golden/field_w32_<PRIME>.json.xz).  modarith_amd.h (the 64-bit form: 5 x 51,
 * 5 x 52, 8 x 56 limbs in uint64_t) is unchanged; both forms live in one library and share its utilities (modarith_amd_last_error,
 * modarith_amd_malloc, streams, ... of modarith_amd.h).
 *
 *   <fn>_<PRIME>_w32_ct(...)     scalar form: the reference's signature over uint32_t, host pointers, one element through the GPU.
 *   <fn>_<PRIME>_w32_batch(...)  batched form: DEVICE pointers, n elements, limb stride ld, stream -- the argument order of the
 *                                64-bit <fn>_<PRIME>_batch forms.
 *
 * for all 32 functions of field.c (prop flatten modfsb modadd modsub modneg modmli modmul modsqr modcpy modnsqr modpro modinv modqr
 * modsqrt nres redc modis1 modis0 modzer modone modint modcmv modcsw modshl modshr modhaf mod2r modexp modimp modsign modcmp), plus
 * the batched moduniform and modlimbs.  Not offered at this word length: modmuls, the _lazy forms, time_protocol and the ladders
 * (rfc7748_* speaks bytes and does not depend on the word length).  The curve layer over these fields -- ecn_<c>_w32_* on points of
 * uint32_t limbs, `curve.py 32` -- is declared in modarith_amd_w32_curve.h.
 *
 * Batched layout: limb-interleaved SoA of uint32_t, FLAT (ld >= n: buf[limb*ld + j]) or TILED (ld < n, a power of two >= 128:
 * buf[((j / ld)*Nlimbs + limb)*ld + (j % ld)]), exactly as in modarith_amd.h with 32-bit words.  An element is 36 bytes (X25519,
 * NIST256) or 64 bytes (X448).  Per-lane access width: 16 bytes (four elements per lane) for the 9-limb fields and 8 bytes (two)
 * for X448 when every buffer is 16- / 8-byte aligned and ld is a multiple of 4 / 2; 4 bytes otherwise.  Same results on every path.
 * One product policy: a 32-bit limb product is one 32 x 32 -> 64 multiply-add into a 64-bit column, the reference's own dpint
 * arithmetic -- exact for every limb pattern, no limb contract.  modinv returns the NORMALISED inverse nres of redc of 1/x as at 64
 * bits; without progenitors and from 32 768 elements on, the batched modinv shares one inversion between up to 64 elements
 * (Montgomery's simultaneous inversion; in place it takes stream-ordered scratch of the library's own, and under stream capture or
 * with MA_INV_SIMUL=0 it keeps one inversion per element) -- the same words either way, for every limb pattern; which path ran is
 * what modarith_amd_last_launch reports.  Sequences of calls per element fuse into one kernel through modarith_amd/fuse.py at this
 * word length too (plug-ins exporting chain_<name>_<PRIME>_w32_batch).  Ownership, aliasing (an output may be an input: modmul(a, a, a), modsqr(a, a)), errors, streams
 * and threading: as in modarith_amd.h.  MODARITH_AMD_ABI is unchanged by this header: nothing existing changed.
 */
#ifndef MODARITH_AMD_W32_H
#define MODARITH_AMD_W32_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint32_t ma_spint32; /* spint of the 32-bit field.c */

/* per-prime macro block of the 32-bit field.c (Nlimbs Radix Nbits Nbytes, Montgomery form or not): returns 0 if `prime` is not built at this word length */
int modarith_amd_w32_field_info(const char *prime, int *nlimbs, int *radix, int *nbits, int *nbytes, int *montgomery);
/* element-major (uint32_t x[n][nlimbs], how a field.cu-style caller holds arrays of elements) <-> SoA (flat or tiled, by ld); any limb count */
int modarith_amd_w32_aos_to_soa(const ma_spint32 *aos, ma_spint32 *soa, size_t n, int nlimbs, size_t ld, void *stream);
int modarith_amd_w32_soa_to_aos(const ma_spint32 *soa, ma_spint32 *aos, size_t n, int nlimbs, size_t ld, void *stream);
/* the number of 32-bit words a batch of n elements of nlimbs limbs occupies with stride ld (flat: nlimbs*ld; tiled: whole tiles) */
size_t modarith_amd_w32_batch_words(size_t n, int nlimbs, size_t ld);

#define MODARITH_AMD_DECLARE_W32(P)                                                                                                 \
    /* ---------------- scalar form: reference signatures over uint32_t, host pointers ---------------- */                          \
    ma_spint32 prop_##P##_w32_ct(ma_spint32 *n);     /* static in field.c; exported so that all 32 emitted names exist */           \
    ma_spint32 flatten_##P##_w32_ct(ma_spint32 *n);                                                                                 \
    ma_spint32 modfsb_##P##_w32_ct(ma_spint32 *n);                                                                                  \
    void modadd_##P##_w32_ct(const ma_spint32 *a, const ma_spint32 *b, ma_spint32 *n);                                              \
    void modsub_##P##_w32_ct(const ma_spint32 *a, const ma_spint32 *b, ma_spint32 *n);                                              \
    void modneg_##P##_w32_ct(const ma_spint32 *b, ma_spint32 *n);                                                                   \
    void modmli_##P##_w32_ct(const ma_spint32 *a, int b, ma_spint32 *c);                                                            \
    void modmul_##P##_w32_ct(const ma_spint32 *a, const ma_spint32 *b, ma_spint32 *c);                                              \
    void modsqr_##P##_w32_ct(const ma_spint32 *a, ma_spint32 *c);                                                                   \
    void modcpy_##P##_w32_ct(const ma_spint32 *a, ma_spint32 *c);                                                                   \
    void modnsqr_##P##_w32_ct(ma_spint32 *a, int n);                                                                                \
    void modpro_##P##_w32_ct(const ma_spint32 *w, ma_spint32 *z);                                                                   \
    void modinv_##P##_w32_ct(const ma_spint32 *x, const ma_spint32 *h, ma_spint32 *z); /* h may be NULL */                          \
    int modqr_##P##_w32_ct(const ma_spint32 *h, const ma_spint32 *x);                  /* h may be NULL */                          \
    void modsqrt_##P##_w32_ct(const ma_spint32 *x, const ma_spint32 *h, ma_spint32 *r); /* h may be NULL */                         \
    void nres_##P##_w32_ct(const ma_spint32 *m, ma_spint32 *n);                                                                     \
    void redc_##P##_w32_ct(const ma_spint32 *n, ma_spint32 *m);                                                                     \
    int modis1_##P##_w32_ct(const ma_spint32 *a);                                                                                   \
    int modis0_##P##_w32_ct(const ma_spint32 *a);                                                                                   \
    void modzer_##P##_w32_ct(ma_spint32 *a);                                                                                        \
    void modone_##P##_w32_ct(ma_spint32 *a);                                                                                        \
    void modint_##P##_w32_ct(int x, ma_spint32 *a);                                                                                 \
    void modcmv_##P##_w32_ct(int b, const ma_spint32 *g, volatile ma_spint32 *f);                                                   \
    void modcsw_##P##_w32_ct(int b, volatile ma_spint32 *g, volatile ma_spint32 *f);                                                \
    void modshl_##P##_w32_ct(unsigned int n, ma_spint32 *a);                                                                        \
    int modshr_##P##_w32_ct(unsigned int n, ma_spint32 *a);                                                                         \
    void modhaf_##P##_w32_ct(ma_spint32 *n);                                                                                        \
    void mod2r_##P##_w32_ct(unsigned int r, ma_spint32 *a);                                                                         \
    void modexp_##P##_w32_ct(const ma_spint32 *a, char *b);                                                                         \
    int modimp_##P##_w32_ct(const char *b, ma_spint32 *a);                                                                          \
    int modsign_##P##_w32_ct(const ma_spint32 *a);                                                                                  \
    int modcmp_##P##_w32_ct(const ma_spint32 *a, const ma_spint32 *b);                                                              \
    /* ---------------- batched form: device pointers, SoA of uint32_t, limb stride ld ---------------- */                          \
    int modadd_##P##_w32_batch(const ma_spint32 *a, const ma_spint32 *b, ma_spint32 *n_, size_t n, size_t ld, void *stream);        \
    int modsub_##P##_w32_batch(const ma_spint32 *a, const ma_spint32 *b, ma_spint32 *n_, size_t n, size_t ld, void *stream);        \
    int modneg_##P##_w32_batch(const ma_spint32 *b, ma_spint32 *n_, size_t n, size_t ld, void *stream);                             \
    int modmul_##P##_w32_batch(const ma_spint32 *a, const ma_spint32 *b, ma_spint32 *c, size_t n, size_t ld, void *stream);         \
    int modsqr_##P##_w32_batch(const ma_spint32 *a, ma_spint32 *c, size_t n, size_t ld, void *stream);                              \
    int modmli_##P##_w32_batch(const ma_spint32 *a, int b, ma_spint32 *c, size_t n, size_t ld, void *stream);                       \
    int modcpy_##P##_w32_batch(const ma_spint32 *a, ma_spint32 *c, size_t n, size_t ld, void *stream);                              \
    int modnsqr_##P##_w32_batch(ma_spint32 *a, int k, size_t n, size_t ld, void *stream);                                           \
    int modpro_##P##_w32_batch(const ma_spint32 *w, ma_spint32 *z, size_t n, size_t ld, void *stream);                              \
    int modinv_##P##_w32_batch(const ma_spint32 *x, const ma_spint32 *h, ma_spint32 *z, size_t n, size_t ld, void *stream);         \
    int modsqrt_##P##_w32_batch(const ma_spint32 *x, const ma_spint32 *h, ma_spint32 *r, size_t n, size_t ld, void *stream);        \
    int modqr_##P##_w32_batch(const ma_spint32 *h, const ma_spint32 *x, int *out, size_t n, size_t ld, void *stream);               \
    int nres_##P##_w32_batch(const ma_spint32 *m, ma_spint32 *n_, size_t n, size_t ld, void *stream);                               \
    int redc_##P##_w32_batch(const ma_spint32 *n_, ma_spint32 *m, size_t n, size_t ld, void *stream);                               \
    /* in place; flag (device int[n], may be NULL) receives the return value per element */                                         \
    int modfsb_##P##_w32_batch(ma_spint32 *a, int *flag, size_t n, size_t ld, void *stream);                                        \
    int flatten_##P##_w32_batch(ma_spint32 *a, int *flag, size_t n, size_t ld, void *stream);                                       \
    int prop_##P##_w32_batch(ma_spint32 *a, int *flag, size_t n, size_t ld, void *stream);   /* flag: -1 / 0 (the mask) */          \
    int modhaf_##P##_w32_batch(ma_spint32 *a, size_t n, size_t ld, void *stream);                                                   \
    int modshl_##P##_w32_batch(unsigned int k, ma_spint32 *a, size_t n, size_t ld, void *stream);                                   \
    int modshr_##P##_w32_batch(unsigned int k, ma_spint32 *a, int *out, size_t n, size_t ld, void *stream);                         \
    /* predicates: out = device int[n] */                                                                                           \
    int modis1_##P##_w32_batch(const ma_spint32 *a, int *out, size_t n, size_t ld, void *stream);                                   \
    int modis0_##P##_w32_batch(const ma_spint32 *a, int *out, size_t n, size_t ld, void *stream);                                   \
    int modsign_##P##_w32_batch(const ma_spint32 *a, int *out, size_t n, size_t ld, void *stream);                                  \
    /* not in field.c: out[j] = 1 when every limb of element j is below 2^(Radix+2) */                                              \
    int modlimbs_##P##_w32_batch(const ma_spint32 *a, int *out, size_t n, size_t ld, void *stream);                                 \
    int modcmp_##P##_w32_batch(const ma_spint32 *a, const ma_spint32 *b, int *out, size_t n, size_t ld, void *stream);              \
    /* fills */                                                                                                                     \
    int modzer_##P##_w32_batch(ma_spint32 *a, size_t n, size_t ld, void *stream);                                                   \
    int modone_##P##_w32_batch(ma_spint32 *a, size_t n, size_t ld, void *stream);                                                   \
    int modint_##P##_w32_batch(int x, ma_spint32 *a, size_t n, size_t ld, void *stream);                                            \
    int mod2r_##P##_w32_batch(unsigned int r, ma_spint32 *a, size_t n, size_t ld, void *stream);                                    \
    /* constant-time conditional move/swap, one selector d[j] in {0,1} per element (device int[n]) */                               \
    int modcmv_##P##_w32_batch(const int *d, const ma_spint32 *g, ma_spint32 *f, size_t n, size_t ld, void *stream);                \
    int modcsw_##P##_w32_batch(const int *d, ma_spint32 *g, ma_spint32 *f, size_t n, size_t ld, void *stream);                      \
    /* synthetic inputs: the integers of moduniform_<P>_batch for the same (seed, array, first), as canonical limbs of this form */ \
    int moduniform_##P##_w32_batch(unsigned long long seed, unsigned long long array, size_t first, int plus_p,                     \
                                   ma_spint32 *out, size_t n, size_t ld, void *stream);                                             \
    /* byte records: device char[n*Nbytes], big-endian per record as modimp/modexp take them, 8-byte aligned */                     \
    int modimp_##P##_w32_batch(const char *b, ma_spint32 *a, int *flag, size_t n, size_t ld, void *stream);                         \
    int modexp_##P##_w32_batch(const ma_spint32 *a, char *b, size_t n, size_t ld, void *stream);

MODARITH_AMD_DECLARE_W32(X25519)
MODARITH_AMD_DECLARE_W32(NIST256)
MODARITH_AMD_DECLARE_W32(X448)

#ifdef __cplusplus
}
#endif
#endif
