// C-ABI entry points of the 32-bit word form of X448 (Wordlength 32: <fn>_X448_w32_batch / <fn>_X448_w32_ct); body: capi_w32.inc
#include "generated/w32_X448.h"
#define MA_P ma32::P_X448_W32
#define MA_NAME X448
#include "capi_w32.inc"
