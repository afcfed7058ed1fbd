// C-ABI entry points of the 32-bit word form of X25519 (Wordlength 32: <fn>_X25519_w32_batch / <fn>_X25519_w32_ct); body: capi_w32.inc
#include "generated/w32_X25519.h"
#define MA_P ma32::P_X25519_W32
#define MA_NAME X25519
#include "capi_w32.inc"
