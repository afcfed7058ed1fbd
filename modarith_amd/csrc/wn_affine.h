// modarith_amd/csrc/wn_affine.h -- AFFINE window tables for the fused P-256 kernels (round 5): the multiples 1P .. 8P of every record
// are brought to Z = 1 with one inversion per up to 32 table entries, so that the window loop adds them with the Jacobian MIXED addition
// (7M + 4S = 1 360 multiply-adds against the 2 035 of the general one): 64 additions per scalar at 675 multiply-adds less, for about
// 1 000 per table entry (8 000 per record) in the kernel below -- mul_get 5.2 -> 5.9-6.1e7/s.  (secp256k1 stays on projective tables:
// its complete mixed addition, 11M = 1 310 multiply-adds, saves too little against the complete addition's 12M = 1 433 to pay for the
// normalisation; built and measured, 8.3 -> 8.4e7/s for mul_get, 6.2 -> 5.9e7/s for mulgen2_get.)
//
// The table is per RECORD of a chunk, not per resident lane: T[entry][word][record] (wn26.h's put / get with the record count as the
// stride), 15 words per entry while it is projective, the first 10 (x, y) after k_wn_table_affine; C holds the prefix products of the
// shared inversion, flag[record] = "P is the point at infinity" (then every multiple is, and the window kernels never use the
// entries).  An entry with Z = 0 counts as 1 in the shared inversion in BOTH passes, whatever the flag says: a record whose point is
// not on the curve cannot disturb the records it shares an inversion with.  1 284 bytes per record (2 564 with two tables) for at most WNAFF_CHUNK records.  Pipeline per chunk: the table kernel of the curve (wj26.h) ->
// k_wn_table_affine -> the window kernel -> wn_export.h.
//
// JAC = true: entries are Jacobian (x = X / Z^2, y = Y / Z^3); false: homogeneous (x = X / Z, y = Y / Z).
#pragma once
#include "capi_common.h"
#include "kernels.h"
#include "shared_inv.h"

namespace ma {

constexpr size_t WNAFF_CHUNK = (size_t)1 << 19;

struct WnAffWs {
    uint64_t *T, *C;
    uint32_t* flag;
    size_t m;                               // records of this chunk = row length
    int ne;                                 // entries per record: 8 (one table) or 16 (two: e P + f Q)
    static size_t bytes_per_record(int ne_) { return (size_t)(ne_ * 15 + ne_ * 5) * sizeof(uint64_t) + sizeof(uint32_t); }
    static size_t bytes(size_t n, int ne_ = 8) { return ((n < WNAFF_CHUNK ? n : WNAFF_CHUNK) * bytes_per_record(ne_) + 7) & ~(size_t)7; }    // (what follows it in a workspace stays 8-byte aligned)
    WnAffWs(void* ws, size_t m_, int ne_ = 8) : m(m_), ne(ne_) {
        T = reinterpret_cast<uint64_t*>(ws);
        C = T + (size_t)ne * 15 * m;
        flag = reinterpret_cast<uint32_t*>(C + (size_t)ne * 5 * m);
    }
    // limbs of coordinate c (0: X / x, 1: Y / y, 2: Z) of entry e of record t
    template <class F>
    MA_DEV void load(int e, int c, size_t t, int32_t* f) const {
        uint64_t w[5];
        static_for<0, 5>([&](auto K) { w[K] = T[(size_t)(e * 15 + c * 5 + K) * m + t]; });
        F::unpack(w, f);
    }
    template <class F>
    MA_DEV void store(int e, int c, size_t t, const int32_t* f) const {
        uint64_t w[5];
        F::pack(f, w);
        static_for<0, 5>([&](auto K) { T[(size_t)(e * 15 + c * 5 + K) * m + t] = w[K]; });
    }
};

// The items of lane j for shared_inv_walk() (shared_inv.h): the ne entries of records j, j + L, ..., j + (R - 1) L -- up to 32 entries
// under one inversion --, item g = entry g % ne of record (g / ne) L + j, its Z the denominator; (x, y) go back into the entry.  An entry
// with Z = 0 keeps the X, Y it has (nobody reads it).  flag[t], written on the way down (entry 8 comes before entry 0): bit 0 = the
// first table's point is at infinity (its entry 1 has Z = 0; then all its multiples have), bit 1 = the second table's (entries 8..15)
template <class F, bool JAC>
struct WnAffItems {
    const WnAffWs& ws;
    size_t L, j;
    MA_DEV int entry(int g) const { return g % ws.ne; }
    MA_DEV size_t record(int g) const { return (size_t)(g / ws.ne) * L + j; }
    MA_DEV bool valid(int g) const { return record(g) < ws.m; }
    MA_DEV bool load_den(int g, int32_t* z) const {
        ws.load<F>(entry(g), 2, record(g), z);
        return den_or_one<F>(z);
    }
    MA_DEV void store_prefix(int g, const int32_t* c) const {
        uint64_t w[5];
        F::pack(c, w);
        static_for<0, 5>([&](auto K) { ws.C[(size_t)(entry(g) * 5 + K) * ws.m + record(g)] = w[K]; });
    }
    MA_DEV void load_prefix(int g, int32_t* c) const {
        uint64_t w[5];
        static_for<0, 5>([&](auto K) { w[K] = ws.C[(size_t)(entry(g) * 5 + K) * ws.m + record(g)]; });
        F::unpack(w, c);
    }
    MA_DEV void emit(int g, const int32_t* zi, bool zero) const {
        const int e = entry(g);
        const size_t t = record(g);
        if (e == 8) ws.flag[t] = zero ? 2u : 0u;
        if (e == 0) ws.flag[t] = (ws.ne > 8 ? ws.flag[t] : 0u) | (zero ? 1u : 0u);
        int32_t x[10], zx[10];
        if constexpr (JAC) F::sqr(zi, zx);
        else F::copy(zi, zx);
        ws.load<F>(e, 0, t, x);
        F::mul(x, zx, x);
        ws.store<F>(e, 0, t, x);
        if constexpr (JAC) F::mul(zx, zi, zx);
        ws.load<F>(e, 1, t, x);
        F::mul(x, zx, x);
        ws.store<F>(e, 1, t, x);
    }
};
template <class F, bool JAC>
MA_DEV void wn_table_affine_lane(const WnAffWs& ws, size_t L, int R, size_t j) {
    shared_inv_walk<F>(ws.ne * R, WnAffItems<F, JAC>{ws, L, j});
}

template <class F, bool JAC, int TAG>
__global__ __launch_bounds__(64) void k_wn_table_affine(WnAffWs ws, size_t L, int R) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L) wn_table_affine_lane<F, JAC>(ws, L, R, j);
}

template <class F, bool JAC, int TAG>
void wn_table_affine(const WnAffWs& ws, hipStream_t s) {
    const auto [L, rounds] = shared_inv_rounds(ws.m, (size_t)(32 / ws.ne));
    k_wn_table_affine<F, JAC, TAG><<<(unsigned)((L + 63) / 64), 64, 0, s>>>(ws, L, rounds);
}

// +- entry base + |m| - 1 of record t's affine table (m = 1..8; 0 leaves (0, 0)), all eight entries from base on read (wn26.h lookup),
// the sign applied to y
template <class F>
MA_DEV void wn_affine_lookup(const WnAffWs& ws, size_t t, uint32_t m, bool neg, int32_t* sx, int32_t* sy, int base = 0) {
    uint64_t sel[10];
    static_for<0, 10>([&](auto K) { sel[K] = 0; });
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("" ::: "memory");
#endif
#pragma unroll 1
    for (int e = 0; e < 8; e += 2) {
        uint64_t ent[2][10];
        static_for<0, 2>([&](auto EI) {
            static_for<0, 10>([&](auto K) { ent[EI][K] = ws.T[(size_t)((base + e + EI) * 15 + K) * ws.m + t]; });
        });
        static_for<0, 2>([&](auto EI) {
            const bool hit = (m == (uint32_t)(e + EI + 1));
            static_for<0, 10>([&](auto K) {
                const uint64_t a = ent[EI][K], b = sel[K];
                sel[K] = hit ? a : b;
            });
        });
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" ::: "memory");
#endif
    }
    int32_t ny[10];
    F::unpack(sel, sx);
    F::unpack(sel + 5, sy);
    F::neg(sy, ny);
    F::select(neg, sy, ny, sy);
}

}  // namespace ma
