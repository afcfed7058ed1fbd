// modarith_amd/csrc/kernels32.h -- the batched field kernels of the 32-bit word form (Wordlength 32): csrc/kernels.h compiled with
// MA_WL = 32 (namespace ma32: spint = uint32_t, dpint = uint64_t; field.h).  kernels.h says what the word length changes.
#pragma once
#ifndef MA_WL
#define MA_WL 32
#endif
#if MA_WL != 32
#error "kernels32.h is the 32-bit word form: a translation unit holds one word length"
#endif
#include "kernels.h"
