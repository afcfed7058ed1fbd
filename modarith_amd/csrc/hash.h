// modarith_amd/csrc/hash.h -- the reference's hash.c per lane: SHA-256, SHA-384 / SHA-512, SHA-3 and SHAKE over a byte record that
// is handed over as up to eight PARTS (dom4, R, A, M of ed448.c:219-225 without a concatenation pass).  __host__ __device__, so that
// tools/hash_host.hip runs these very functions on the CPU against hashlib before a GPU is involved.
//
// What is restated from the reference (values only; the text is new):
//   sha256_compress   hash.c:47-88    (HASH256_transform; the 64-word schedule becomes a rolling window of 16)
//   sha512_compress   hash.c:194-232  (HASH512_transform, shared by SHA-384; rolling window of 16)
//   keccak_f          hash.c:359-442  (SHA3_transform)
//   KeccakPad         hash.c:507-540  (0x06 ... 0x80 / 0x86 for SHA-3, 0x1f ... 0x80 / 0x9f for SHAKE)
//   keccak_squeeze    hash.c:474-505  (SHA3_squeeze)
//   Sha2Pad           hash.c:129-147, 312-330 (0x80, zeros, the bit length in the last words of the block)
//
// The one design rule: state and schedule are indexed by compile-time constants only (hash_for), so they stay in registers.
// hash.c's SHA3_process writes S[cnt / 8] ^= byte << 8 * b: a dynamically indexed array, which would send the 200-byte state to
// scratch.  Here the bytes come from a per-lane cursor (part, offset); each rate word (Keccak) or block word (SHA-2) is put together
// from the next bytes of the cursor and XORed or assigned at a static index.  Past the end of the message the cursor hands out the
// padding bytes (and for SHA-2 the length words), so ONE absorb loop serves every length.
//
// Timing: the instruction sequence of a lane depends on the LENGTHS of its parts only (number of blocks, where a part ends).  No
// table is indexed by message data and no branch tests message data: the round constants are indexed by the round counter.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <type_traits>

#ifndef MA_HASH_DEV
#define MA_HASH_DEV __host__ __device__ __forceinline__
#endif

namespace ma {
namespace hash {

template <int I, int End, class Fn>
MA_HASH_DEV void hash_for(Fn&& fn) {
    if constexpr (I < End) {
        fn(std::integral_constant<int, I>{});
        hash_for<I + 1, End>(fn);
    }
}

// ---- the record: up to 8 parts, by value in the kernel arguments (the layout of ma_hash_part, include/modarith_amd_hash.h)
struct Part {
    const unsigned char* ptr;   // record j starts at ptr + j * stride; any alignment
    size_t stride;              // 0: one record shared by the whole batch
    const uint32_t* lens;       // n entries or null; record j contributes min(lens[j], len) bytes
    uint32_t len;
};
constexpr int MAX_PARTS = 8;
struct Parts {
    Part p[MAX_PARTS];
    int n;
};

// ---- padding rules: the byte at stream position pos >= total (total: the message length), and the length of the padded stream
template <int BLOCK, int LENFIELD>                       // SHA-2: BLOCK 64 / 128 bytes, the bit length in the last LENFIELD bytes
struct Sha2Pad {
    static MA_HASH_DEV uint64_t padded(uint64_t total) { return (total + 1 + LENFIELD + (BLOCK - 1)) & ~(uint64_t)(BLOCK - 1); }
    static MA_HASH_DEV uint32_t byte(uint64_t pos, uint64_t total, uint64_t end) {
        const uint64_t back = end - pos;                 // 1 for the last byte of the stream
        uint32_t b = pos == total ? 0x80u : 0u;
        // records stay below 2^32 bytes: the bit length fits 8 bytes, the upper half of SHA-512's 16-byte field is zero
        if (back <= 8) b = (uint32_t)((total << 3) >> (8 * (back - 1))) & 0xffu;
        return b;
    }
};
template <int RATE, int DOM>                             // Keccak: DOM 0x06 (SHA-3) / 0x1f (SHAKE); one byte free: DOM | 0x80
struct KeccakPad {
    static MA_HASH_DEV uint64_t padded(uint64_t total) { return (total / RATE + 1) * RATE; }
    static MA_HASH_DEV uint32_t byte(uint64_t pos, uint64_t total, uint64_t end) {
        return (pos == total ? (uint32_t)DOM : 0u) | (pos + 1 == end ? 0x80u : 0u);
    }
};

// ---- the byte source: walks the parts of record j, then the padding
template <class PAD>
struct Cursor {
    const unsigned char* p;     // next byte of the current part
    uint32_t left;              // bytes left in the current part
    int k;                      // the next part to open
    uint64_t pos, total, end;   // bytes handed out so far; the message length; the padded length

    static MA_HASH_DEV uint32_t part_len(const Part& q, size_t j) {
        uint32_t l = q.len;
        if (q.lens) { const uint32_t v = q.lens[j]; l = v < l ? v : l; }       // the clamp: never outside the row the caller described
        return l;
    }
    MA_HASH_DEV void open(const Parts& P, size_t j) {
        p = nullptr; left = 0; k = 0; pos = 0; total = 0;
        hash_for<0, MAX_PARTS>([&](auto I) { if (I < P.n) total += part_len(P.p[I], j); });
        end = PAD::padded(total);
    }
    MA_HASH_DEV uint64_t blocks(int block_bytes) const { return end / (uint64_t)block_bytes; }
    // open part k.  P is the kernel-argument block itself (passed down by reference, never copied to a private array), so P.p[k] with
    // a per-lane k is a load from constant memory; a select over the eight static indices instead keeps all 56 words of the parts in
    // scalar registers for the whole kernel and spills some of them to vector lanes
    MA_HASH_DEV void next_part(const Parts& P, size_t j) {
        const Part& q = P.p[k];
        left = part_len(q, j);
        p = q.ptr + j * q.stride;
        k++;
    }
    MA_HASH_DEV uint32_t next_byte(const Parts& P, size_t j) {
        while (left == 0 && k < P.n) next_part(P, j);
        uint32_t b;
        if (left) { b = *p++; left--; }
        else b = PAD::byte(pos, total, end);
        pos++;
        return b;
    }
    // the next NB bytes as one word, first byte most (BE) or least significant
    template <class W, bool BE>
    MA_HASH_DEV W next_word(const Parts& P, size_t j) {
        constexpr int NB = (int)sizeof(W);
        W w = 0;
        if (left >= (uint32_t)NB) {                      // wholly inside the current part
            hash_for<0, NB>([&](auto B) { w |= (W)p[B] << (8 * (BE ? NB - 1 - B : (int)B)); });
            p += NB; left -= NB; pos += NB;
        } else {
#pragma unroll 1
            for (int b = 0; b < NB; b++) w |= (W)next_byte(P, j) << (8 * (BE ? NB - 1 - b : b));
        }
        return w;
    }
    // one block of NW words: put(I, word, take) for I = 0 .. NW - 1, I a compile-time constant; the word is for place I when take is set.
    //  - the block lies wholly inside the current part: straight loads at static offsets;
    //  - otherwise (a part ends in it, or the padding begins): ONE copy of the byte walk in a loop over the word number i, which is
    //    the same in every lane, and the word goes to its place through a select on i == I over the static indices -- never state[i] (and not `if (i == I)`
    //    either: the compiler folds that chain back into an indexed private array, 144 bytes of scratch).
    // (One inlined copy of the walk per word instead costs a divergent region per word and, on gfx950, 60 more registers.)
    template <class W, bool BE, int NW, class Put>
    MA_HASH_DEV void next_block(const Parts& P, size_t j, Put&& put) {
        constexpr int NB = (int)sizeof(W);
        if (left >= (uint32_t)(NW * NB)) {
            hash_for<0, NW>([&](auto I) {
                W w = 0;
                hash_for<0, NB>([&](auto B) { w |= (W)p[I * NB + B] << (8 * (BE ? NB - 1 - B : (int)B)); });
                put(I, w, true);
#if defined(__HIP_DEVICE_COMPILE__)
                // at most four words of byte loads in flight: hoisted over the whole block they hold a register per BYTE (the Keccak
                // kernels then need more than 256 registers and fall back to accumulation registers)
                if constexpr (I % 4 == 3) __builtin_amdgcn_sched_barrier(0);
#endif
            });
            p += NW * NB; left -= NW * NB; pos += NW * NB;
        } else {
#pragma unroll 1
            for (int i = 0; i < NW; i++) {
                const W w = next_word<W, BE>(P, j);
                hash_for<0, NW>([&](auto I) { put(I, w, i == I); });
            }
        }
    }
};

template <class W> MA_HASH_DEV W rotr(W x, int n) { return (x >> n) | (x << (8 * (int)sizeof(W) - n)); }
template <class W> MA_HASH_DEV W ch(W x, W y, W z) { return z ^ (x & (y ^ z)); }                 // (x & y) ^ (~x & z)
template <class W> MA_HASH_DEV W maj(W x, W y, W z) { return (x & y) | (z & (x | y)); }           // (x & y) ^ (x & z) ^ (y & z)

// ---- SHA-256 (FIPS 180-4 6.2): 32-bit words
struct Sha256 {
    using word = uint32_t;
    static constexpr int ROUNDS = 64, BLOCK = 64;
    using Pad = Sha2Pad<64, 8>;
    static MA_HASH_DEV word K(int j) {
        constexpr word k[64] = {
            0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
            0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
            0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
            0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
            0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
            0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
        return k[j];
    }
    static MA_HASH_DEV word S0(word x) { return rotr(x, 2) ^ rotr(x, 13) ^ rotr(x, 22); }
    static MA_HASH_DEV word S1(word x) { return rotr(x, 6) ^ rotr(x, 11) ^ rotr(x, 25); }
    static MA_HASH_DEV word t0(word x) { return rotr(x, 7) ^ rotr(x, 18) ^ (x >> 3); }
    static MA_HASH_DEV word t1(word x) { return rotr(x, 17) ^ rotr(x, 19) ^ (x >> 10); }
    template <int DIGEST>
    static MA_HASH_DEV void init(word* h) {
        h[0] = 0x6a09e667u; h[1] = 0xbb67ae85u; h[2] = 0x3c6ef372u; h[3] = 0xa54ff53au;
        h[4] = 0x510e527fu; h[5] = 0x9b05688cu; h[6] = 0x1f83d9abu; h[7] = 0x5be0cd19u;
    }
};

// ---- SHA-512 and SHA-384 (FIPS 180-4 6.4, 6.5): 64-bit words, register pairs on the device
struct Sha512 {
    using word = uint64_t;
    static constexpr int ROUNDS = 80, BLOCK = 128;
    using Pad = Sha2Pad<128, 16>;
    static MA_HASH_DEV word K(int j) {
        constexpr word k[80] = {
            0x428a2f98d728ae22ull, 0x7137449123ef65cdull, 0xb5c0fbcfec4d3b2full, 0xe9b5dba58189dbbcull, 0x3956c25bf348b538ull, 0x59f111f1b605d019ull,
            0x923f82a4af194f9bull, 0xab1c5ed5da6d8118ull, 0xd807aa98a3030242ull, 0x12835b0145706fbeull, 0x243185be4ee4b28cull, 0x550c7dc3d5ffb4e2ull,
            0x72be5d74f27b896full, 0x80deb1fe3b1696b1ull, 0x9bdc06a725c71235ull, 0xc19bf174cf692694ull, 0xe49b69c19ef14ad2ull, 0xefbe4786384f25e3ull,
            0x0fc19dc68b8cd5b5ull, 0x240ca1cc77ac9c65ull, 0x2de92c6f592b0275ull, 0x4a7484aa6ea6e483ull, 0x5cb0a9dcbd41fbd4ull, 0x76f988da831153b5ull,
            0x983e5152ee66dfabull, 0xa831c66d2db43210ull, 0xb00327c898fb213full, 0xbf597fc7beef0ee4ull, 0xc6e00bf33da88fc2ull, 0xd5a79147930aa725ull,
            0x06ca6351e003826full, 0x142929670a0e6e70ull, 0x27b70a8546d22ffcull, 0x2e1b21385c26c926ull, 0x4d2c6dfc5ac42aedull, 0x53380d139d95b3dfull,
            0x650a73548baf63deull, 0x766a0abb3c77b2a8ull, 0x81c2c92e47edaee6ull, 0x92722c851482353bull, 0xa2bfe8a14cf10364ull, 0xa81a664bbc423001ull,
            0xc24b8b70d0f89791ull, 0xc76c51a30654be30ull, 0xd192e819d6ef5218ull, 0xd69906245565a910ull, 0xf40e35855771202aull, 0x106aa07032bbd1b8ull,
            0x19a4c116b8d2d0c8ull, 0x1e376c085141ab53ull, 0x2748774cdf8eeb99ull, 0x34b0bcb5e19b48a8ull, 0x391c0cb3c5c95a63ull, 0x4ed8aa4ae3418acbull,
            0x5b9cca4f7763e373ull, 0x682e6ff3d6b2b8a3ull, 0x748f82ee5defb2fcull, 0x78a5636f43172f60ull, 0x84c87814a1f0ab72ull, 0x8cc702081a6439ecull,
            0x90befffa23631e28ull, 0xa4506cebde82bde9ull, 0xbef9a3f7b2c67915ull, 0xc67178f2e372532bull, 0xca273eceea26619cull, 0xd186b8c721c0c207ull,
            0xeada7dd6cde0eb1eull, 0xf57d4f7fee6ed178ull, 0x06f067aa72176fbaull, 0x0a637dc5a2c898a6ull, 0x113f9804bef90daeull, 0x1b710b35131c471bull,
            0x28db77f523047d84ull, 0x32caab7b40c72493ull, 0x3c9ebe0a15c9bebcull, 0x431d67c49c100d4cull, 0x4cc5d4becb3e42b6ull, 0x597f299cfc657e2aull,
            0x5fcb6fab3ad6faecull, 0x6c44198c4a475817ull};
        return k[j];
    }
    static MA_HASH_DEV word S0(word x) { return rotr(x, 28) ^ rotr(x, 34) ^ rotr(x, 39); }
    static MA_HASH_DEV word S1(word x) { return rotr(x, 14) ^ rotr(x, 18) ^ rotr(x, 41); }
    static MA_HASH_DEV word t0(word x) { return rotr(x, 1) ^ rotr(x, 8) ^ (x >> 7); }
    static MA_HASH_DEV word t1(word x) { return rotr(x, 19) ^ rotr(x, 61) ^ (x >> 6); }
    template <int DIGEST>
    static MA_HASH_DEV void init(word* h) {
        if constexpr (DIGEST == 48) {
            h[0] = 0xcbbb9d5dc1059ed8ull; h[1] = 0x629a292a367cd507ull; h[2] = 0x9159015a3070dd17ull; h[3] = 0x152fecd8f70e5939ull;
            h[4] = 0x67332667ffc00b31ull; h[5] = 0x8eb44a8768581511ull; h[6] = 0xdb0c2e0d64f98fa7ull; h[7] = 0x47b5481dbefa4fa4ull;
        } else {
            h[0] = 0x6a09e667f3bcc908ull; h[1] = 0xbb67ae8584caa73bull; h[2] = 0x3c6ef372fe94f82bull; h[3] = 0xa54ff53a5f1d36f1ull;
            h[4] = 0x510e527fade682d1ull; h[5] = 0x9b05688c2b3e6c1full; h[6] = 0x1f83d9abfb41bd6bull; h[7] = 0x5be0cd19137e2179ull;
        }
    }
};

// one block: h += compress(h, w).  w[16] is the block on entry and the rolling schedule afterwards (W[t] lives in w[t & 15])
template <class A>
MA_HASH_DEV void sha2_compress(typename A::word* h, typename A::word* w) {
    using word = typename A::word;
    word v[8];
    hash_for<0, 8>([&](auto I) { v[I] = h[I]; });
    // rounds in groups of 16 (the schedule window; a multiple of 8, so v[] is back in place after each group): the first group takes
    // the block as it is, the others roll the window on first.  K is read by the round number from constant memory: with all rounds unrolled the
    // constants become 64 / 160 scalar registers hoisted out of the block loop, more than there are
    auto round = [&](auto J, int base) {
        constexpr int j = J;
        // the eight working variables rotate through v[] by index instead of by copy: a of round j is v[(8 - j) & 7]
        constexpr int a = (16 - j) & 7, b = (a + 1) & 7, c = (a + 2) & 7, d = (a + 3) & 7, e = (a + 4) & 7, f = (a + 5) & 7, g = (a + 6) & 7, hh = (a + 7) & 7;
        const word T1 = v[hh] + A::S1(v[e]) + ch(v[e], v[f], v[g]) + A::K(base + j) + w[j];
        const word T2 = A::S0(v[a]) + maj(v[a], v[b], v[c]);
        v[d] += T1;
        v[hh] = T1 + T2;
    };
#pragma unroll 1
    for (int base = 0; base < A::ROUNDS; base += 16) {
        if (base)                                         // W[t] = s1(W[t-2]) + W[t-7] + s0(W[t-15]) + W[t-16], in place and in order
            hash_for<0, 16>([&](auto J) {
                constexpr int j = J;
                w[j] += A::t1(w[(j + 14) & 15]) + w[(j + 9) & 15] + A::t0(w[(j + 1) & 15]);
            });
        hash_for<0, 16>([&](auto J) { round(J, base); });
    }
    hash_for<0, 8>([&](auto I) { h[I] += v[I]; });
}
MA_HASH_DEV void sha256_compress(uint32_t* h, uint32_t* w) { sha2_compress<Sha256>(h, w); }
MA_HASH_DEV void sha512_compress(uint64_t* h, uint64_t* w) { sha2_compress<Sha512>(h, w); }

// record j of P -> DIGEST bytes at out (big-endian words, HASH256_hash / HASH512_hash)
template <class A, int DIGEST>
MA_HASH_DEV void sha2_record(const Parts& P, size_t j, unsigned char* out) {
    using word = typename A::word;
    constexpr int WB = (int)sizeof(word);
    Cursor<typename A::Pad> cur;
    cur.open(P, j);
    word h[8], w[16];
    A::template init<DIGEST>(h);
    for (uint64_t nb = cur.blocks(A::BLOCK); nb; nb--) {
        cur.template next_block<word, true, 16>(P, j, [&](auto I, word x, bool take) { w[I] = take ? x : w[I]; });
        sha2_compress<A>(h, w);
    }
    hash_for<0, DIGEST / WB>([&](auto I) {
        hash_for<0, WB>([&](auto B) { out[I * WB + B] = (unsigned char)(h[I] >> (8 * (WB - 1 - B))); });
    });
}

// ---- Keccak-f[1600]: 25 lanes of 64 bits, 24 rounds (FIPS 202 3.2-3.3)
MA_HASH_DEV uint64_t rotl64(uint64_t x, int n) { return (x << n) | (x >> (64 - n)); }
MA_HASH_DEV uint64_t keccak_rc(int round) {
    constexpr uint64_t rc[24] = {
        0x0000000000000001ull, 0x0000000000008082ull, 0x800000000000808aull, 0x8000000080008000ull, 0x000000000000808bull, 0x0000000080000001ull,
        0x8000000080008081ull, 0x8000000000008009ull, 0x000000000000008aull, 0x0000000000000088ull, 0x0000000080008009ull, 0x000000008000000aull,
        0x000000008000808bull, 0x800000000000008bull, 0x8000000000008089ull, 0x8000000000008003ull, 0x8000000000008002ull, 0x8000000000000080ull,
        0x000000000000800aull, 0x800000008000000aull, 0x8000000080008081ull, 0x8000000000008080ull, 0x0000000080000001ull, 0x8000000080008008ull};
    return rc[round];                                     // indexed by the round counter, never by data
}
MA_HASH_DEV void keccak_f(uint64_t* s) {
    // rho offsets by lane index x + 5 y, and pi: lane (x, y) moves to (y, 2x + 3y)
    constexpr int RHO[25] = {0, 1, 62, 28, 27, 36, 44, 6, 55, 20, 3, 10, 43, 25, 39, 41, 45, 15, 21, 8, 18, 2, 61, 56, 14};
#pragma unroll 1
    for (int round = 0; round < 24; round++) {
        uint64_t c[5], d[5], b[25];
        hash_for<0, 5>([&](auto X) { c[X] = s[X] ^ s[X + 5] ^ s[X + 10] ^ s[X + 15] ^ s[X + 20]; });
        hash_for<0, 5>([&](auto X) { d[X] = c[(X + 4) % 5] ^ rotl64(c[(X + 1) % 5], 1); });
        hash_for<0, 25>([&](auto I) {
            constexpr int x = I % 5, y = I / 5, to = y + 5 * ((2 * x + 3 * y) % 5), r = RHO[I];
            const uint64_t t = s[I] ^ d[x];
            if constexpr (r == 0) b[to] = t;
            else b[to] = rotl64(t, r);
        });
        hash_for<0, 25>([&](auto I) {
            constexpr int x = I % 5, y = I / 5;
            s[I] = b[I] ^ (~b[y * 5 + (x + 1) % 5] & b[y * 5 + (x + 2) % 5]);
        });
        s[0] ^= keccak_rc(round);
    }
}

// record j of P -> olen bytes at out.  RATE in bytes (200 - 2 * security bytes), DOM 0x06 / 0x1f
template <int RATE, int DOM>
MA_HASH_DEV void keccak_squeeze(uint64_t* s, unsigned char* out, size_t olen) {
    size_t m = 0;
    for (;;) {
        hash_for<0, RATE / 8>([&](auto I) {
            hash_for<0, 8>([&](auto B) {
                if (m + I * 8 + B < olen) out[m + I * 8 + B] = (unsigned char)(s[I] >> (8 * B));
            });
        });
        m += RATE;
        if (m >= olen) break;
        keccak_f(s);
    }
}
template <int RATE, int DOM>
MA_HASH_DEV void keccak_record(const Parts& P, size_t j, unsigned char* out, size_t olen) {
    static_assert(RATE % 8 == 0 && RATE > 0 && RATE < 200, "rate");
    Cursor<KeccakPad<RATE, DOM>> cur;
    cur.open(P, j);
    uint64_t s[25];
    hash_for<0, 25>([&](auto I) { s[I] = 0; });
    for (uint64_t nb = cur.blocks(RATE); nb; nb--) {
        cur.template next_block<uint64_t, false, RATE / 8>(P, j, [&](auto I, uint64_t x, bool take) { s[I] ^= take ? x : 0; });
        keccak_f(s);
    }
    keccak_squeeze<RATE, DOM>(s, out, olen);
}

}  // namespace hash
}  // namespace ma
