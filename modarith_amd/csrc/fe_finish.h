// modarith_amd/csrc/fe_finish.h -- the end of a BATCH of RFC 7748 ladders with one inversion per `rounds` scalars
// (Montgomery's simultaneous inversion), for the fused ladders of fe26.h (X25519) and fe28.h (X448).
//
// rfc7748() ends every scalar multiplication in modinv + modmul + modexp (rfc7748.c:225-254): for X25519 254 squarings and
// 11 multiplications, 7.7 % of the whole function (X448: 447 + 13, about the same share).  The batched entry point does not
// owe one inversion to each lane: a first kernel (k_x25519_fe26_xz / k_x448_fe28_xz) runs the ladders and leaves canonical
// x2 in the output record and canonical z2 in a workspace; the second (k_fe_finish) gives lane j the elements
// {r * L + j : r < rounds} (L lanes, so that every access of a wave is one coalesced row), multiplies their z up into
// prefix products, inverts the last one, and walks back with three multiplications per element (shared_inv.h: the walk).  A z2 of
// zero (u = 0, the low-order points of RFC 7748 section 7) enters the product as 1 and its output -- x2 * 0^(p-2) = 0 in the
// reference -- leaves as zero, by a select and a per-lane mask.  Same bytes as the one-inversion-per-lane kernels for every input.
#pragma once
#include "shared_inv.h"

namespace ma {

// The items of lane j for shared_inv_walk(): elements r * L + j < n, canonical denominators A[NW][n] (word-major, as the kernel in front
// left them), prefix products wc[NL][n] (limb-major, 32-bit), NUM numerators: num(Q, K, e) = word K of numerator Q of element e, and
// sink(e, q0, q1) takes the canonical quotients (q1 = q0 where NUM = 1), all zero where the denominator was zero
template <class F, int NL, int NW, int NUM, class NUMS, class SINK>
struct FeDivItems {
    const uint64_t* A;
    uint32_t* wc;
    size_t n, L, j;
    const NUMS& num;
    SINK& sink;
    MA_DEV size_t element(int r) const { return (size_t)r * L + j; }
    MA_DEV bool valid(int r) const { return element(r) < n; }
    MA_DEV bool load_den(int r, uint32_t* z) const {
        const size_t e = element(r);
        uint64_t zw[NW], any = 0;
        static_for<0, NW>([&](auto K) { any |= zw[K] = A[(size_t)K * n + e]; });
        const bool zero = any == 0;
        zw[0] = zero ? 1 : zw[0];
        F::from_words(zw, z);
        return zero;
    }
    MA_DEV void store_prefix(int r, const uint32_t* c) const {
        static_for<0, NL>([&](auto I) { wc[(size_t)I * n + element(r)] = c[I]; });
    }
    // the walk asks for r = i - 1 while it is at element(i): element(r + 1) is that index, already in registers, and one subtraction
    // gives this one; written as element(r) the compiler forms r L + j again (a second v_mad_u64_u32 per item in every instance)
    MA_DEV void load_prefix(int r, uint32_t* c) const {
        const size_t e = element(r + 1) - L;
        static_for<0, NL>([&](auto I) { c[I] = wc[(size_t)I * n + e]; });
    }
    MA_DEV void emit(int r, const uint32_t* zinv, bool zero) const {
        const size_t e = element(r);
        const uint64_t keep = lane_mask(!zero);
        uint64_t q[NUM][NW];
        static_for<0, NUM>([&](auto Q) {
            uint64_t xw[NW];
            uint32_t x[NL];
            static_for<0, NW>([&](auto K) { xw[K] = num(Q, K, e); });
            F::from_words(xw, x);
            F::mul(x, zinv, x);
            F::to_words(x, q[Q]);
        });
        static_for<0, NUM>([&](auto Q) { static_for<0, NW>([&](auto K) { q[Q][K] &= keep; }); });
        sink(e, q[0], q[NUM - 1]);
    }
};
template <class F, int NL, int NW, int NUM, class NUMS, class SINK>
MA_DEV void fe_div_lane(const uint64_t* A, uint32_t* wc, size_t n, size_t L, int rounds, size_t j, const NUMS& num, SINK& sink) {
    shared_inv_walk<F>(rounds, FeDivItems<F, NL, NW, NUM, NUMS, SINK>{A, wc, n, L, j, num, sink});
}

// the ladders: x2 in the output record bv[n][NW], divided in place
template <class F, int NL, int NW>
struct FeFinish {
    static MA_DEV void run(uint64_t* bv, const uint64_t* wz, uint32_t* wc, size_t n, size_t L, int rounds, size_t j) {
        auto sink = [&](size_t e, const uint64_t* q, const uint64_t*) { static_for<0, NW>([&](auto K) { bv[e * NW + K] = q[K]; }); };
        fe_div_lane<F, NL, NW, 1>(wz, wc, n, L, rounds, j, [&](int, int K, size_t e) { return bv[e * NW + K]; }, sink);
    }
};

// one inversion per `rounds` elements; wc[NL][n] receives the prefix products (limb-major, 32-bit)
template <class F, int NL, int NW>
__global__ __launch_bounds__(256) void k_fe_finish(uint64_t* bv, const uint64_t* wz, uint32_t* wc, size_t n, size_t L, int rounds) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L) FeFinish<F, NL, NW>::run(bv, wz, wc, n, L, rounds, j);
}

// ---- round 5: the same trick with TWO numerators per denominator, for the ladder form of the fused Edwards multiplications
// (ed26l.h: u = nu / D and w = nw / D in front of the ladder, x = X / Z and y = Y / Z behind it).  A, B, C: canonical words,
// word-major [NW][n] (every access of a wave is one coalesced row).  B[e] / A[e], C[e] / A[e] are handed to sink(e, bw, cw).
template <class F, int NL, int NW>
struct FeBatchDiv {
    template <class SINK>
    static MA_DEV void run(const uint64_t* A, const uint64_t* B, const uint64_t* Cn, uint32_t* wc, size_t n, size_t L, int rounds, size_t j, SINK& sink) {
        fe_div_lane<F, NL, NW, 2>(A, wc, n, L, rounds, j, [&](int Q, int K, size_t e) { return (Q == 0 ? B : Cn)[(size_t)K * n + e]; }, sink);
    }
};
// TAG keeps the instantiations of different translation units apart (one code object each)
template <class F, int NL, int NW, class SINK, int TAG>
__global__ __launch_bounds__(64) void k_fe_batch_div(const uint64_t* A, const uint64_t* B, const uint64_t* Cn, uint32_t* wc, size_t n, size_t L, int rounds, SINK sink) {
    const size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < L) FeBatchDiv<F, NL, NW>::run(A, B, Cn, wc, n, L, rounds, j, sink);
}
// the quotients back into their own arrays as canonical words
template <int NW>
struct SinkWords {
    uint64_t *B, *Cn;
    size_t n;
    MA_DEV void operator()(size_t e, uint64_t* bw, uint64_t* cw) const {
        static_for<0, NW>([&](auto K) { B[(size_t)K * n + e] = bw[K]; Cn[(size_t)K * n + e] = cw[K]; });
    }
};

}  // namespace ma
