/* include/field_NIST256_w32.h -- EMITTED by modarith_amd/emit.py field_shim_text(); do not edit.
 *
 * The 32-bit word form of field_NIST256.h (Wordlength 32: spint = uint32_t, dpint = uint64_t, the limbs of the reference's
 * `monty.py 32 NIST256` and of simd/monty_cuda.py's field.cu).  Put  #include "field_NIST256_w32.h"  where the
 * reference's templates say "paste field.c here" and link libmodarith_amd.so: modmul(a, b, c) ... then run on the GPU one
 * element at a time (host pointers, the reference's signatures and aliasing rules; throughput comes from the
 * <fn>_NIST256_w32_batch entry points of modarith_amd_w32.h).
 * prime NIST256 = 0xffffffff00000001000000000000000000000000ffffffffffffffffffffffff, monty.py form
 */
#ifndef MODARITH_AMD_FIELD_NIST256_W32_H
#define MODARITH_AMD_FIELD_NIST256_W32_H
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
#define Nbits 256
#define Nbytes 32

#define MONTGOMERY
#define NIST256

#define prop prop_NIST256_w32_ct
#define flatten flatten_NIST256_w32_ct
#define modfsb modfsb_NIST256_w32_ct
#define modadd modadd_NIST256_w32_ct
#define modsub modsub_NIST256_w32_ct
#define modneg modneg_NIST256_w32_ct
#define modmli modmli_NIST256_w32_ct
#define modmul modmul_NIST256_w32_ct
#define modsqr modsqr_NIST256_w32_ct
#define modcpy modcpy_NIST256_w32_ct
#define modnsqr modnsqr_NIST256_w32_ct
#define modpro modpro_NIST256_w32_ct
#define modinv modinv_NIST256_w32_ct
#define nres nres_NIST256_w32_ct
#define redc redc_NIST256_w32_ct
#define modis1 modis1_NIST256_w32_ct
#define modis0 modis0_NIST256_w32_ct
#define modzer modzer_NIST256_w32_ct
#define modone modone_NIST256_w32_ct
#define modint modint_NIST256_w32_ct
#define modqr modqr_NIST256_w32_ct
#define modcmv modcmv_NIST256_w32_ct
#define modcsw modcsw_NIST256_w32_ct
#define modsqrt modsqrt_NIST256_w32_ct
#define modshl modshl_NIST256_w32_ct
#define modshr modshr_NIST256_w32_ct
#define modhaf modhaf_NIST256_w32_ct
#define mod2r mod2r_NIST256_w32_ct
#define modexp modexp_NIST256_w32_ct
#define modimp modimp_NIST256_w32_ct
#define modsign modsign_NIST256_w32_ct
#define modcmp modcmp_NIST256_w32_ct

#endif
