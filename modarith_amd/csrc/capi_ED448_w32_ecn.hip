// modarith_amd/csrc/capi_ED448_w32_ecn.hip -- the curve layer of ED448 at word length 32 (ecn_ed448_w32_*: include/modarith_amd_w32_curve.h)
// over the 16 x 28-bit Montgomery field of w32_X448.h; body: capi_curve.inc.
#define MA_MUL_WPS 2
#include "generated/w32_curve_ED448.h"
#include "edwards.h"
// The table layout that ships is one limb per row.  MA_W32_TABLE_PACKED (csrc/curve.h) with a MA_CNAME of its own builds the measured
// alternative for tools/w32_curve_rate.py: its kernels get names of their own through a curve struct of their own.
#ifdef MA_W32_TABLE_PACKED
namespace ma32 { struct C_ED448_W32P : C_ED448_W32 {}; }
#define MA_CURVE_CLASS ma32::Edwards<ma32::C_ED448_W32P>
#else
#define MA_CURVE_CLASS ma32::Edwards<ma32::C_ED448_W32>
#endif
#ifndef MA_CNAME
#define MA_CNAME ed448_w32
#endif
#include "capi_curve.inc"
