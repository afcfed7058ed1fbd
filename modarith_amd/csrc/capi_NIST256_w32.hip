// C-ABI entry points of the 32-bit word form of NIST256 (Wordlength 32: <fn>_NIST256_w32_batch / <fn>_NIST256_w32_ct); body: capi_w32.inc
#include "generated/w32_NIST256.h"
#define MA_P ma32::P_NIST256_W32
#define MA_NAME NIST256
#include "capi_w32.inc"
