// modarith_amd/csrc/window.h -- the signed-window digit source of the variable-base multiplications, once: s = e + bias (comb.h
// comb_bias_add: a 1 in the top bit of every W-bit window below BITS), so that window i of s minus 2^(W-1) is the signed digit i of e
// with no carries between digits; the windows are handed out from the top.  No curve and no field in here.  Users: the Straus forms
// (ed26s.h <4, 260, 4>, ed28s.h <4, 452, 7>), the Weierstrass windows (wn26.h <4, 260, 4> and <3, 258, 4>; wj26.h with a parked flag),
// each half scalar of the secp256k1 split (glv26.h <4, 132, 3>).  NI = the words of e; e + bias must stay below 2^BITS.
#pragma once
#include "comb.h"

namespace ma {

// the digits in shift registers: s left-aligned in NS words; window(i) for i = 0, 1, ... in order
template <int W, int BITS, int NI>
struct WinRegs {
    static constexpr int NS = (BITS + 63) / 64, COUNT = (BITS + W - 1) / W;
    static_assert(NI <= NS && BITS % W == 0, "whole windows, and the scalar's words within the state");
    uint64_t w[NS];
    MA_DEV void init(const uint64_t* e) {
        comb_bias_add<W, BITS, NI, NS>(e, w);
        shl_words<64 * NS - BITS, NS>(w);           // the top window (bits BITS-W .. BITS-1 of s) to the top of w[NS - 1]
    }
    MA_DEV uint32_t window(int) { return take_top_bits<W, NS>(w); }
};
// one byte per window in the lane's column of an LDS array (64 lanes a row), written once before the point is loaded
template <int W, int BITS, int NI>
struct WinLds {
    static constexpr int COUNT = (BITS + W - 1) / W;
    unsigned char* col;
    static MA_DEV void fill(const uint64_t* e, unsigned char* col) {
        WinRegs<W, BITS, NI> r;
        r.init(e);
#pragma unroll 1
        for (int i = 0; i < COUNT; i++) col[(size_t)i * 64] = (unsigned char)r.window(i);
    }
    MA_DEV uint32_t window(int i) const { return col[(size_t)i * 64]; }
};
// ... with one per-lane flag kept beside the digits (wj26.h): in a register, or in one more row of the LDS column
template <class REGS>
struct WinRegsPark : REGS {
    uint32_t flag = 0;
    MA_DEV void park(uint32_t v) { flag = v; }
    MA_DEV uint32_t parked() const { return flag; }
};
template <class LDS>
struct WinLdsPark : LDS {
    static constexpr int ROWS = LDS::COUNT + 1;
    MA_DEV void park(uint32_t v) { this->col[(size_t)LDS::COUNT * 64] = (unsigned char)v; }
    MA_DEV uint32_t parked() const { return this->col[(size_t)LDS::COUNT * 64]; }
};

}  // namespace ma
