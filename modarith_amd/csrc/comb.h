// modarith_amd/csrc/comb.h -- the fixed-base ("comb") walk of the fused generator multiplications, once: the biased scalar, the
// signed digits, the scan of the window's table entries, and the declaration of a unit's table.  No curve and no field in here: the
// callers (ed26.h, ed28.h, wn26.h) apply the digit's sign and add.  What the comb is and what was measured: docs/curve_layer.md,
// "The fixed-base comb".
#pragma once
#include "field.h"

namespace ma {

// s = e + bias, NO words from the bottom (e: NS words); bias: a 1 in every bit position b < BITS with b % W == W - 1, folded per
// word at compile time.  Window i of s minus 2^(W-1) is then the signed digit i of e, with no carries between digits.
template <int W, int BITS, int NS, int NO = NS + 1>
MA_DEV void comb_bias_add(const uint64_t* ew, uint64_t* s) {
    constexpr auto cw = [](int k) {
        uint64_t v = 0;
        for (int b = 0; b < 64; b++) {
            const int pos = 64 * k + b;
            if (pos < BITS && pos % W == W - 1) v |= (uint64_t)1 << b;
        }
        return v;
    };
    unsigned __int128 acc = 0;
    static_for<0, NO>([&](auto K) {
        constexpr int k = K;
        acc += (unsigned __int128)(k < NS ? ew[k < NS ? k : 0] : 0) + cw(k);
        s[k] = (uint64_t)acc;
        acc >>= 64;
    });
}

// The walk over the TAB::NW windows of e (NS words), from the bottom: step(sel, neg, m) is handed the window's entry |digit| = m --
// NC coordinates of NL limbs of type T, read as TAB::get(((window * 2^(W-1) + m - 1) * NC + coordinate) * NL + limb) -- and the
// digit's sign.  For m = 0 no entry is selected: all limbs are 0, but for limb 0 of the coordinates whose bit is set in ONES, which is 1.
template <class TAB, int NS, int NC, int NL, unsigned ONES, class T, class STEP>
MA_DEV void comb_walk(const uint64_t* ew, STEP step) {
    constexpr int W = TAB::W, NW = TAB::NW, E2 = 1 << (W - 1);       // window width, windows, entries per window
    static_assert(W * NW > 64 * NS && W * NW <= 64 * (NS + 1), "e + bias must fit the windows and NS + 1 words");
    uint64_t w[NS + 1];
    comb_bias_add<W, W * NW, NS>(ew, w);
#pragma unroll 1
    for (int i = 0; i < NW; i++) {
        const int dgt = (int)((uint32_t)w[0] & (uint32_t)(2 * E2 - 1)) - E2;        // [-2^(W-1), 2^(W-1) - 1]
        static_for<0, NS + 1>([&](auto K) {
            constexpr int k = K;
            w[k] >>= W;
            if constexpr (k < NS) w[k] |= w[k + 1] << (64 - W);
        });
        const bool neg = dgt < 0;
        const uint32_t m = (uint32_t)(neg ? -dgt : dgt);        // 0 .. 2^(W-1)
        // selection as OR of masked entries (exactly one mask is set, none for a zero digit): the entries sit in scalar
        // registers, and v_and_or_b32 takes one of those next to two vector operands -- a v_cndmask would need a move first
        // (its lane mask already uses the one scalar operand an instruction may read).  A limb that starts at 1 does so only
        // for a zero digit, so the OR never meets a set bit.
        T sel[NC][NL];
        static_for<0, NC>([&](auto CI) {
            static_for<0, NL>([&](auto K) { sel[CI][K] = (K == 0 && ((ONES >> CI) & 1u) && m == 0) ? 1 : 0; });
        });
        static_for<0, E2>([&](auto MM) {
            constexpr int mm = MM;
            uint32_t mask = (m == (uint32_t)(mm + 1)) ? 0xffffffffu : 0u;
#if defined(__HIP_DEVICE_COMPILE__)
            asm("" : "+v"(mask));       // opaque: otherwise the compiler turns (entry & mask) back into a select with a move
#endif
            static_for<0, NC>([&](auto CI) {
                static_for<0, NL>([&](auto K) {
                    sel[CI][K] = (T)((uint32_t)sel[CI][K] | ((uint32_t)TAB::get(((i * E2 + mm) * NC + CI) * NL + K) & mask));
                });
            });
        });
        step(sel, neg, m);
    }
}

// MA_COMB_TABLE(TAB, ARRAY, C): this unit's table is COMB_<C>_VALUES with COMB_<C>_W and COMB_<C>_WINDOWS (generated/comb_<C>.h,
// included by the unit) -- windows x 2^(W-1) multiples x coordinates x limbs, the same for every lane, read through wave-uniform
// indices.  On the device ARRAY lies in the constant address space (scalar loads); a host-only compile (tools/fe_host_check.hip,
// tools/wn26_host.hip) defines MA_COMB_SPACE as `static const` first and gets a plain array.  TAB is the type the walk takes.
#ifndef MA_COMB_SPACE
#define MA_COMB_SPACE __constant__
#endif
#define MA_COMB_TABLE(TAB, ARRAY, C)                                                \
    MA_COMB_SPACE int32_t ARRAY[] = { COMB_##C##_VALUES };                          \
    struct TAB {                                                                    \
        static constexpr int W = COMB_##C##_W, NW = COMB_##C##_WINDOWS;             \
        static MA_DEV int32_t get(int idx) { return ARRAY[idx]; }                   \
    }

}  // namespace ma
