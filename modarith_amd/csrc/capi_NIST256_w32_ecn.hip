// modarith_amd/csrc/capi_NIST256_w32_ecn.hip -- the curve layer of NIST P-256 at word length 32 (ecn_nist256_w32_*: include/modarith_amd_w32_curve.h)
// over the 9 x 29-bit Montgomery field of w32_NIST256.h; body: capi_curve.inc.
#define MA_MUL_WPS 3
#include "generated/w32_curve_NIST256.h"
#include "weierstrass.h"
// The table layout that ships is one limb per row.  MA_W32_TABLE_PACKED (csrc/curve.h) with a MA_CNAME of its own builds the measured
// alternative for tools/w32_curve_rate.py: its kernels get names of their own through a curve struct of their own.
#ifdef MA_W32_TABLE_PACKED
namespace ma32 { struct C_NIST256_W32P : C_NIST256_W32 {}; }
#define MA_CURVE_CLASS ma32::Weierstrass<ma32::C_NIST256_W32P>
#else
#define MA_CURVE_CLASS ma32::Weierstrass<ma32::C_NIST256_W32>
#endif
#ifndef MA_CNAME
#define MA_CNAME nist256_w32
#endif
#include "capi_curve.inc"
