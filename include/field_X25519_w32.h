/* include/field_X25519_w32.h -- EMITTED by modarith_amd/emit.py field_shim_text(); do not edit.
 *
 * The 32-bit word form of field_X25519.h (Wordlength 32: spint = uint32_t, dpint = uint64_t, the limbs of the reference's
 * `pseudo.py 32 X25519` and of simd/pseudo_cuda.py's field.cu).  Put  #include "field_X25519_w32.h"  where the
 * reference's templates say "paste field.c here" and link libmodarith_amd.so: modmul(a, b, c) ... then run on the GPU one
 * element at a time (host pointers, the reference's signatures and aliasing rules; throughput comes from the
 * <fn>_X25519_w32_batch entry points of modarith_amd_w32.h).
 * prime X25519 = 0x7fffffffffffffffffffffffffffffffffffffffffffffffffffffffffffffed, pseudo.py form
 */
#ifndef MODARITH_AMD_FIELD_X25519_W32_H
#define MODARITH_AMD_FIELD_X25519_W32_H
#include <stdio.h>
#include <stdint.h>
#include "modarith_amd_w32.h"

#define sspint int32_t
#define spint uint32_t
#define dpint uint64_t
#define sdpint int64_t
#define Wordlength 32
#define Nlimbs 9
#define Radix 29
#define Nbits 255
#define Nbytes 32

#define MERSENNE
#define MULBYINT
#define X25519

#define prop prop_X25519_w32_ct
#define flatten flatten_X25519_w32_ct
#define modfsb modfsb_X25519_w32_ct
#define modadd modadd_X25519_w32_ct
#define modsub modsub_X25519_w32_ct
#define modneg modneg_X25519_w32_ct
#define modmli modmli_X25519_w32_ct
#define modmul modmul_X25519_w32_ct
#define modsqr modsqr_X25519_w32_ct
#define modcpy modcpy_X25519_w32_ct
#define modnsqr modnsqr_X25519_w32_ct
#define modpro modpro_X25519_w32_ct
#define modinv modinv_X25519_w32_ct
#define nres nres_X25519_w32_ct
#define redc redc_X25519_w32_ct
#define modis1 modis1_X25519_w32_ct
#define modis0 modis0_X25519_w32_ct
#define modzer modzer_X25519_w32_ct
#define modone modone_X25519_w32_ct
#define modint modint_X25519_w32_ct
#define modqr modqr_X25519_w32_ct
#define modcmv modcmv_X25519_w32_ct
#define modcsw modcsw_X25519_w32_ct
#define modsqrt modsqrt_X25519_w32_ct
#define modshl modshl_X25519_w32_ct
#define modshr modshr_X25519_w32_ct
#define modhaf modhaf_X25519_w32_ct
#define mod2r mod2r_X25519_w32_ct
#define modexp modexp_X25519_w32_ct
#define modimp modimp_X25519_w32_ct
#define modsign modsign_X25519_w32_ct
#define modcmp modcmp_X25519_w32_ct

#endif
