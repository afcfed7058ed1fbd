// tools/window_host.hip -- the signed-window digit source (csrc/window.h) and take_top_bit (csrc/field.h) compiled for the HOST as a
// stand-alone program, so that tests/test_host_arith.py can hold them against Python integers.  Test tooling, not product code.
//   hipcc -O1 -g -std=c++17 --offload-host-only -fsanitize=address,undefined tools/window_host.hip -o window_host
// One request per line of standard input, one answer per line of standard output (numbers in hex, no prefix):
//   w SET E  -> the COUNT windows of E from WinRegs, then those WinLds::fill wrote into (and window() read back from) a plain array
//               standing in for the LDS column, as two strings of one hex digit per window; SET: 0 <4, 260, 4>, 1 <3, 258, 4>,
//               2 <4, 452, 7>, 3 <4, 132, 3>
//   t NW V   -> the 64 NW bits take_top_bit<NW> hands out of V, as a string of 0 / 1, then V after the first call; NW: 4 or 7
#define MA_DEV __host__ __device__ inline
#include "../modarith_amd/csrc/window.h"

#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>

template <int NW>
static void parse(const char* hex, uint64_t* w) {
    for (int k = 0; k < NW; k++) w[k] = 0;
    const int n = (int)strlen(hex);
    for (int i = 0; i < n && i < 16 * NW; i++) {
        const char c = hex[n - 1 - i];
        const uint64_t d = (uint64_t)(c <= '9' ? c - '0' : (c | 0x20) - 'a' + 10);
        w[i / 16] |= d << (4 * (i % 16));
    }
}

template <int W, int BITS, int NI>
static void windows(const char* hex) {
    using REGS = ma::WinRegs<W, BITS, NI>;
    using LDS = ma::WinLds<W, BITS, NI>;
    uint64_t e[NI];
    parse<NI>(hex, e);
    REGS r;
    r.init(e);
    for (int i = 0; i < REGS::COUNT; i++) printf("%x", r.window(i));
    printf(" ");
    // the column of lane 63, the last one: its last byte is the last byte of the array
    std::vector<unsigned char> lds((size_t)LDS::COUNT * 64, 0xff);
    LDS::fill(e, lds.data() + 63);
    const LDS d{lds.data() + 63};
    for (int i = 0; i < LDS::COUNT; i++) printf("%x", d.window(i));
    size_t untouched = 0;
    for (size_t i = 0; i < lds.size(); i++) untouched += (i % 64 != 63 && lds[i] == 0xff);
    printf(" %zu\n", lds.size() - untouched);           // bytes written: COUNT
}

template <int NW>
static void top_bits(const char* hex) {
    uint64_t v[NW];
    parse<NW>(hex, v);
    std::string bits, first;
    for (int i = 0; i < 64 * NW; i++) {
        bits += (char)('0' + ma::take_top_bit<NW>(v));
        if (i == 0) {
            char buf[17];
            for (int k = NW - 1; k >= 0; k--) { snprintf(buf, sizeof buf, "%016llx", (unsigned long long)v[k]); first += buf; }
        }
    }
    printf("%s %s\n", bits.c_str(), first.c_str());
}

int main() {
    char kind[8], hex[256];
    int which;
    while (scanf("%7s %d %255s", kind, &which, hex) == 3) {
        if (kind[0] == 'w' && which == 0) windows<4, 260, 4>(hex);
        else if (kind[0] == 'w' && which == 1) windows<3, 258, 4>(hex);
        else if (kind[0] == 'w' && which == 2) windows<4, 452, 7>(hex);
        else if (kind[0] == 'w' && which == 3) windows<4, 132, 3>(hex);
        else if (kind[0] == 't' && which == 4) top_bits<4>(hex);
        else if (kind[0] == 't' && which == 7) top_bits<7>(hex);
        else return 2;
    }
    return 0;
}
