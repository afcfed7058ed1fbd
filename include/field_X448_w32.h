/* include/field_X448_w32.h -- EMITTED by modarith_amd/emit.py field_shim_text(); do not edit.
 *
 * The 32-bit word form of field_X448.h (Wordlength 32: spint = uint32_t, dpint = uint64_t, the limbs of the reference's
 * `monty.py 32 X448` and of simd/monty_cuda.py's field.cu).  Put  #include "field_X448_w32.h"  where the
 * reference's templates say "paste field.c here" and link libmodarith_amd.so: modmul(a, b, c) ... then run on the GPU one
 * element at a time (host pointers, the reference's signatures and aliasing rules; throughput comes from the
 * <fn>_X448_w32_batch entry points of modarith_amd_w32.h).
 * prime X448 = 0xfffffffffffffffffffffffffffffffffffffffffffffffffffffffeffffffffffffffffffffffffffffffffffffffffffffffffffffffff, monty.py form
 */
#ifndef MODARITH_AMD_FIELD_X448_W32_H
#define MODARITH_AMD_FIELD_X448_W32_H
#include <stdio.h>
#include <stdint.h>
#include "modarith_amd_w32.h"

#define sspint int32_t
#define spint uint32_t
#define dpint uint64_t
#define sdpint int64_t
#define Wordlength 32
#define Nlimbs 16
#define Radix 28
#define Nbits 448
#define Nbytes 56

#define MONTGOMERY
#define X448
#define MULBYINT

#define prop prop_X448_w32_ct
#define flatten flatten_X448_w32_ct
#define modfsb modfsb_X448_w32_ct
#define modadd modadd_X448_w32_ct
#define modsub modsub_X448_w32_ct
#define modneg modneg_X448_w32_ct
#define modmli modmli_X448_w32_ct
#define modmul modmul_X448_w32_ct
#define modsqr modsqr_X448_w32_ct
#define modcpy modcpy_X448_w32_ct
#define modnsqr modnsqr_X448_w32_ct
#define modpro modpro_X448_w32_ct
#define modinv modinv_X448_w32_ct
#define nres nres_X448_w32_ct
#define redc redc_X448_w32_ct
#define modis1 modis1_X448_w32_ct
#define modis0 modis0_X448_w32_ct
#define modzer modzer_X448_w32_ct
#define modone modone_X448_w32_ct
#define modint modint_X448_w32_ct
#define modqr modqr_X448_w32_ct
#define modcmv modcmv_X448_w32_ct
#define modcsw modcsw_X448_w32_ct
#define modsqrt modsqrt_X448_w32_ct
#define modshl modshl_X448_w32_ct
#define modshr modshr_X448_w32_ct
#define modhaf modhaf_X448_w32_ct
#define mod2r mod2r_X448_w32_ct
#define modexp modexp_X448_w32_ct
#define modimp modimp_X448_w32_ct
#define modsign modsign_X448_w32_ct
#define modcmp modcmp_X448_w32_ct

#endif
