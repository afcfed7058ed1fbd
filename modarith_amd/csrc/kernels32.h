// modarith_amd/csrc/kernels32.h -- batched element-wise field kernels of the 32-bit word form (Wordlength 32) for gfx950.
//
// The sibling of kernels.h over csrc/field.h compiled with MA_WL = 32 (namespace ma32: spint = uint32_t, dpint = uint64_t -- the
// arithmetic `pseudo.py 32` / `monty.py 32` emit, the limbs of simd/pseudo_cuda.py's field.cu).  Same house shape: limb-interleaved
// SoA buf[limb * ld + j] of uint32_t, flat or tiled through the same Ld descriptor, one element per lane-slot, grid-stride, all limb
// rows of all operands loaded before the arithmetic, non-temporal loads and stores.  What differs from the 64-bit kernels:
//   * one product policy.  CDNA4 multiplies 32 x 32 -> 64 (v_mad_u64_u32); a 32-bit limb product IS one such instruction into a
//     64-bit column, exactly the reference's dpint arithmetic, for every limb pattern: no split forms, no wave vote, no contract.
//   * per-lane access width in ELEMENTS: EPT = 4 (16 bytes, global_load/store_dwordx4), 2 (8 bytes) or 1 (4 bytes: unaligned
//     buffers, odd limb strides, the tail of a batch).  element j = EPT * t + e of thread t, slot e.
#pragma once
#ifndef MA_WL
#define MA_WL 32
#endif
#if MA_WL != 32
#error "kernels32.h is the 32-bit word form: a translation unit holds one word length"
#endif
#include "field.h"

namespace ma32 {

constexpr int BLOCK = 256;
// largest workgroup of a streaming kernel: one element per lane may run 512 threads (95 VGPRs at most: no occupancy lost)
constexpr int stream_block_max(int ept) { return ept == 1 ? 512 : 256; }

template <class T> __device__ __forceinline__ T ld_stream(const T* p) { return __builtin_nontemporal_load(p); }
template <class T> __device__ __forceinline__ void st_stream(T* p, T v) { __builtin_nontemporal_store(v, p); }

// limb stride descriptor of a batch: the same two layouts and the same formula as kernels.h (ma::Ld), in words of this form
struct Ld {
    size_t ld;
    unsigned s;
    __host__ __device__ Ld(size_t ld_ = 0) : ld(ld_), s(63) {}
    __host__ __device__ Ld(size_t ld_, unsigned s_) : ld(ld_), s(s_) {}
    template <int N>
    __host__ __device__ __forceinline__ size_t off(size_t j) const { return (((j >> s) * (size_t)N) << s) + (j & ((((size_t)1) << s) - 1)); }
};

template <int EPT> struct VecOf { typedef spint type __attribute__((ext_vector_type(EPT))); };
template <> struct VecOf<1> { typedef spint type; };

template <class P, int EPT>
__device__ __forceinline__ void load_soa(const spint* base, Ld L, size_t t, spint (*x)[P::N]) {
    static_assert(EPT == 1 || EPT == 2 || EPT == 4, "one, two or four elements per lane");
    const spint* p = base + L.template off<P::N>((size_t)EPT * t);
    if constexpr (EPT == 1) {
        static_for<0, P::N>([&](auto I) { x[0][I] = ld_stream(p + (size_t)I * L.ld); });
    } else {
        using V = typename VecOf<EPT>::type;
        static_for<0, P::N>([&](auto I) {
            V v = ld_stream(reinterpret_cast<const V*>(p + (size_t)I * L.ld));
            static_for<0, EPT>([&](auto E) { constexpr int e = E; x[e][I] = v[e]; });
        });
    }
}
template <class P, int EPT>
__device__ __forceinline__ void store_soa(spint* base, Ld L, size_t t, spint (*x)[P::N]) {
    spint* p = base + L.template off<P::N>((size_t)EPT * t);
    if constexpr (EPT == 1) {
        static_for<0, P::N>([&](auto I) { st_stream(p + (size_t)I * L.ld, x[0][I]); });
    } else {
        using V = typename VecOf<EPT>::type;
        static_for<0, P::N>([&](auto I) {
            V v;
            static_for<0, EPT>([&](auto E) { constexpr int e = E; v[e] = x[e][I]; });
            st_stream(reinterpret_cast<V*>(p + (size_t)I * L.ld), v);
        });
    }
}

// ---- operation functors: apply() works on register-resident elements
template <class P> struct OpMul { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modmul(a, b, c); } };
template <class P> struct OpAdd { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modadd(a, b, c); } };
template <class P> struct OpSub { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modsub(a, b, c); } };
template <class P> struct OpSqr { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modsqr(a, c); } };
template <class P> struct OpNeg { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modneg(a, c); } };
template <class P> struct OpNres { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::nres(a, c); } };
template <class P> struct OpRedc { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::redc(a, c); } };
template <class P> struct OpCpy { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modcpy(a, c); } };
// modinv of the batched API returns the inverse in NORMALISED form nres(redc(1/a)), as at 64 bits (kernels.h inv_normalise): limbs
// that are a function of the value alone -- the reference's modinv leaves whatever its addition chain leaves, a chain this library
// does not share
template <class F> MA_DEV void inv_normalise(spint* z) {
    spint t[F::N];
    F::redc(z, t);
    F::nres(t, z);
}
template <class P> struct OpInv {
    static MA_DEV void apply(const spint* a, spint* c) {
        Field<P>::modinv(a, nullptr, c);
        inv_normalise<Field<P>>(c);
    }
};
template <class P> struct OpSqrt { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modsqrt(a, nullptr, c); } };
template <class P> struct OpPro { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modpro(a, c); } };

// The streaming kernels (k_binary, k_unary, k_mli) take their workgroup size from the launch (at most BLOCK): on tiles the rate
// depends on how many elements one workgroup covers (docs/kernels_field.md), and the C-ABI picks width and workgroup size together.
// c[j] = op(a[j], b[j]).  The slots are written out (not a loop over e): a loop the optimizer declines to unroll leaves x[e]
// indexed at run time, i.e. in scratch (kernels.h k_binary).
template <class P, class Op, int EPT>
__global__ __launch_bounds__(stream_block_max(EPT)) void k_binary(const spint* a, const spint* b, spint* c, size_t nthreads, Ld lda, Ld ldb, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * blockDim.x) {
        spint x[EPT][P::N], y[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        load_soa<P, EPT>(b, ldb, t, y);
        static_for<0, EPT>([&](auto E) { Op::apply(x[E], y[E], z[E]); });
        store_soa<P, EPT>(c, ldc, t, z);
    }
}
// c[j] = op(a[j])
template <class P, class Op, int EPT>
__global__ __launch_bounds__(stream_block_max(EPT)) void k_unary(const spint* a, spint* c, size_t nthreads, Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * blockDim.x) {
        spint x[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        static_for<0, EPT>([&](auto E) { Op::apply(x[E], z[E]); });
        store_soa<P, EPT>(c, ldc, t, z);
    }
}
// c[j] = op(a[j]) for the long chains (modinv, modsqrt, modpro): one element per lane, at least three waves per SIMD
template <class P, class Op>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(3)))
void k_unary_heavy(const spint* a, spint* c, size_t nthreads, Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], z[1][P::N];
        load_soa<P, 1>(a, lda, t, x);
        Op::apply(x[0], z[0]);
        store_soa<P, 1>(c, ldc, t, z);
    }
}
// c[j] = a[j] * b (small integer)
template <class P, int EPT>
__global__ __launch_bounds__(stream_block_max(EPT)) void k_mli(const spint* a, int b, spint* c, size_t nthreads, Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * blockDim.x) {
        spint x[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        static_for<0, EPT>([&](auto E) { Field<P>::modmli(x[E], b, z[E]); });
        store_soa<P, EPT>(c, ldc, t, z);
    }
}
// a[j] = a[j]^(2^k)
template <class P>
__global__ __launch_bounds__(BLOCK) void k_nsqr(spint* a, int k, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N];
        load_soa<P, 1>(a, ld, t, x);
        Field<P>::modnsqr(x[0], k);
        store_soa<P, 1>(a, ld, t, x);
    }
}
// z[j] = 1/x[j] with caller-supplied progenitor h[j] (modinv(x,h,z), pseudo.py:788-812)
template <class P>
__global__ __launch_bounds__(BLOCK) void k_inv_h(const spint* xs, const spint* hs, spint* zs, size_t n, Ld ldx, Ld ldh, Ld ldz) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], h[1][P::N], z[1][P::N];
        load_soa<P, 1>(xs, ldx, t, x);
        load_soa<P, 1>(hs, ldh, t, h);
        Field<P>::modinv(x[0], h[0], z[0]);
        inv_normalise<Field<P>>(z[0]);
        store_soa<P, 1>(zs, ldz, t, z);
    }
}
// In-contract predicate of the simultaneous inversion: DIGIT FORM BELOW 2^(Nbits+1) -- limbs 0..N-2 below 2^Radix and the top limb
// below 2^TOPB, TOPB = Nbits + 1 - Radix (N-1) (24 / 25 / 29 bits for X25519 / NIST256 / X448).  Every element below 2p in digit form
// passes (2p < 2^(Nbits+1)): that is what the field functions return and accept.  modarith_amd/params.py w32_inv_in_contract restates it.
//
// Why modmul(c, x) is congruent to c x (times R^-1 for Montgomery) and modis0 is exact on it, for every admitted x and every c that
// is itself a product output or the constant one.  Write W for the operand set: limbs 0..N-2 below 2^Radix -- but limb 1 of a
// pseudo-Mersenne product output, which is left unmasked, below 2^Radix + 2^15 -- and the top limb below 2^TOPB.  The emitted
// arithmetic is an identity over the integers as long as no 64-bit column and no 32-bit word wraps, so only sizes have to be shown.
//   * X25519 (pseudo.py, Radix 29, N 9, overflow form, mm = 19 * 2^6 = 1216).  Operands a, b in W.  Row r folds the products
//     a_k b_(9+r-k), k = r+1..8.  Row 0 folds eight: a_1 b_8 and a_8 b_1 hold a top limb (< 2^(29.001+24) each), six are below
//     (2^29 - 1)^2: tt < 6.1 * 2^58.  Rows 1..7 fold at most seven products and only limbs 2..8 meet there (k >= 2 and
//     9 + r - k >= 2): tt <= 7 (2^29 - 1)^2.  So hi = tt >> 29 <= 7 * 2^29 - 14 fits a word -- this is what a single limb at
//     2^31 - 1 breaks -- and lo + hi <= (2^29 - 1) + 7 * 2^29 - 14 < 2^32 does not wrap.  A column holds at most nine products
//     (< 2^61.2), (lo + hi) mm < 2^42.3 and a carry below 2^33: < 2^62.  The second pass takes ut = 19 (64 t + (v_8 >> 23)) < 2^44
//     with t < 2^33, leaves limb 0 masked, adds (s >> 29) + (ut >> 29) < 2^15 to limb 1 (the slack of W) and masks the top limb
//     to 23 bits.  So a product output is in W, is congruent to a b, and its value is below 2^255 + 2^45 < 2p.
//   * NIST256 (monty.py, Radix 29, N 9, R = 2^261).  Operands in W have limbs below 2^29.001 and a top limb below 2^25: a column holds
//     at most nine products (< 2^61.2), the reduction adds four digit-times-prime-limb products (< 2^60), two shifted digits and a
//     carry: < 2^62.  Nothing wraps, so c = (a b + q p) / R with q < R: c < 2^514 / 2^261 + p < 2p, in digit form by construction
//     (limbs masked, the top limb takes the rest, below 2^25).
//   * X448 (monty.py, Radix 28, N 16 and the virtual seventeenth limb: R = 2^476, not 2^448 -- modarith_amd/params.py derive_monty;
//     this is where the slack above p comes from).  Limbs below 2^28.001, top limb below 2^29: a column holds at most sixteen products
//     of which two hold a top limb (< 14 * 2^56.001 + 2^58.1 < 2^60.4), prime limbs are -1 / 0 / +1 so the reduction adds a few
//     words: < 2^61.  c = (a b + q p) / R < 2^898 / 2^476 + p < 2p, in digit form, top limb below 2^29.
// So every product output lies in W below 2p, whatever admitted operands it came from, and by induction every prefix c_r and the running
// inverse do.  modis0 is redc -- the identity (pseudo) or a product by one (below p + 1) -- followed by modfsb, which is exact below
// 2p: 1 exactly for the values 0 and p, i.e. for every representation of zero a product can return.
template <class P> MA_DEV bool inv_in_contract(const spint* x) {
    constexpr int TOPB = P::NBITS + 1 - P::RADIX * (P::N - 1);
    static_assert(TOPB > 0 && TOPB <= 29 && P::RADIX <= 29, "the bounds of the comment above");
    spint m = 0;
    static_for<0, P::N - 1>([&](auto I) { m |= x[I]; });
    return ((m >> P::RADIX) | (x[P::N - 1] >> TOPB)) == 0;
}

// z[j] = 1/x[j] for a whole batch with ONE inversion per `rounds` elements (Montgomery's simultaneous inversion): the 32-bit
// counterpart of kernels.h k_inv_simul, whose header comment describes the scheme.  Lane j of L takes the elements {r * L + j}
// (every access of a wave is one coalesced row); forward it multiplies them up and stores the prefix products c_r in cs (the output
// buffer, or scratch when the output is the input); one Field<P>::modinv on the last prefix; backward 1/x_r = inv * c_{r-1},
// inv *= x_r.  Outputs in the normalised form nres(redc(.)): the words of the per-element kernel (OpInv).
// No element may spoil another.  Two kinds stay out of the running product by lane predication (c_r = c_{r-1}); their verdicts
// travel to the backward pass in two per-lane 64-bit masks, bit r for round r (the 29-bit limbs of this form have no spare bits
// once the top limb is unmasked, and rounds <= 64):
//   * zero values, detected on the PRODUCT c_{r-1} * x_r where modis0 is exact whatever the representation of x_r (0, p, 2p): output 0,
//     as the per-element kernel gives (every product of its chain is then 0 or p, and the normalisation makes that 0);
//   * elements outside inv_in_contract (fabricated limbs: the emitted arithmetic wraps on them): an inversion of their own in the
//     backward pass, the very function the per-element kernel runs, paid by the waves that hold one.
template <class P>
struct InvSimul {
    using F = Field<P>;
    static MA_DEV void run(const spint* xs, spint* zs, spint* cs, size_t n, size_t L, int rounds, Ld ldx, Ld ldz, Ld ldc, size_t j) {
        spint c[P::N], x[1][P::N], t[1][P::N];
        uint64_t zeros = 0, oocs = 0;
        F::modone(c);
#pragma unroll 1
        for (int r = 0; r < rounds; r++) {
            const size_t e = (size_t)r * L + j;
            if (e >= n) break;                                  // (e grows with r)
            load_soa<P, 1>(xs, ldx, e, x);
            const bool ooc = !inv_in_contract<P>(x[0]);
            F::modmul(c, x[0], t[0]);                           // (discarded for an out-of-contract x)
            const bool zero = !ooc && F::modis0(t[0]) != 0;
            const bool skip = ooc || zero;
            static_for<0, P::N>([&](auto I) { c[I] = skip ? c[I] : t[0][I]; });
            static_for<0, P::N>([&](auto I) { t[0][I] = c[I]; });
            zeros |= (uint64_t)zero << r;
            oocs |= (uint64_t)ooc << r;
            store_soa<P, 1>(cs, ldc, e, t);
        }
        spint inv[P::N];
        F::modinv(c, nullptr, inv);
#pragma unroll 1
        for (int r = rounds - 1; r >= 0; r--) {
            const size_t e = (size_t)r * L + j;
            if (e >= n) continue;
            load_soa<P, 1>(xs, ldx, e, x);
            const bool zero = (zeros >> r) & 1, ooc = (oocs >> r) & 1;
            spint zi[P::N];
            if (r > 0) {
                load_soa<P, 1>(cs, ldc, e - L, t);
                F::modmul(inv, t[0], zi);                       // inv * c_{r-1}
                F::modmul(inv, x[0], t[0]);
                static_for<0, P::N>([&](auto I) { inv[I] = (zero || ooc) ? inv[I] : t[0][I]; });
            } else {
                static_for<0, P::N>([&](auto I) { zi[I] = inv[I]; });
            }
            inv_normalise<F>(zi);
            static_for<0, P::N>([&](auto I) { zi[I] = zero ? (spint)0 : zi[I]; });
            if (__any(ooc)) {                                   // fabricated limbs somewhere in this wave: their own inversion
                spint w[P::N];
                F::modinv(x[0], nullptr, w);
                inv_normalise<F>(w);
                static_for<0, P::N>([&](auto I) { zi[I] = ooc ? w[I] : zi[I]; });
            }
            static_for<0, P::N>([&](auto I) { t[0][I] = zi[I]; });
            store_soa<P, 1>(zs, ldz, e, t);
        }
    }
};
template <class P>
__global__ __launch_bounds__(BLOCK) void k_inv_simul(const spint* xs, spint* zs, spint* cs, size_t n, size_t L, int rounds, Ld ldx, Ld ldz, Ld ldc) {
    const size_t j = (size_t)blockIdx.x * BLOCK + threadIdx.x;
    if (j < L) InvSimul<P>::run(xs, zs, cs, n, L, rounds, ldx, ldz, ldc, j);
}

// r[j] = sqrt(x[j]) / qr(x[j]) with caller-supplied progenitors h[j] (pseudo.py:815-874)
template <class P, bool QR>
__global__ __launch_bounds__(BLOCK) void k_sqrt_h(const spint* xs, const spint* hs, spint* rs, int* out, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], h[1][P::N], r[1][P::N];
        load_soa<P, 1>(xs, ld, t, x);
        load_soa<P, 1>(hs, ld, t, h);
        if constexpr (QR) {
            out[t] = Field<P>::modqr(h[0], x[0]);
        } else {
            Field<P>::modsqrt(x[0], h[0], r[0]);
            store_soa<P, 1>(rs, ld, t, r);
        }
    }
}
// constant-time conditional swap / move with a per-element selector d[j] in {0,1}: lane predication (v_cndmask), no branch on lane
// data (tests/test_ct_audit_w32.py)
template <class P, bool SWAP>
__global__ __launch_bounds__(BLOCK) void k_cond(const int* d, spint* g, spint* f, size_t n, Ld ldg, Ld ldf) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], y[1][P::N];
        load_soa<P, 1>(g, ldg, t, x);
        load_soa<P, 1>(f, ldf, t, y);
        const int b = d[t];
        if constexpr (SWAP) {
            Field<P>::modcsw(b, x[0], y[0]);
            store_soa<P, 1>(g, ldg, t, x);
        } else {
            Field<P>::modcmv(b, x[0], y[0]);
        }
        store_soa<P, 1>(f, ldf, t, y);
    }
}
// every limb below 2^(Radix+2): the limb budget modlimbs reports
template <class P> MA_DEV bool in_limb_budget(const spint* a) {
    spint m = 0;
    static_for<0, P::N>([&](auto I) { m |= a[I]; });
    return (m >> (P::RADIX + 2)) == 0;
}
// in-place normalisers / predicates; KIND selects the function, optional int result per element
enum { K_MODFSB = 0, K_FLATTEN, K_MODIS1, K_MODIS0, K_MODSIGN, K_MODHAF, K_MODQR, K_MODLIMBS, K_PROP };
template <class P, int KIND>
__global__ __launch_bounds__(BLOCK) void k_inplace(spint* a, int* out, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N];
        load_soa<P, 1>(a, ld, t, x);
        int r = 0;
        bool wr = false;
        if constexpr (KIND == K_MODFSB) { r = (int)Field<P>::modfsb(x[0]); wr = true; }
        if constexpr (KIND == K_FLATTEN) { r = (int)Field<P>::flatten(x[0]); wr = true; }
        if constexpr (KIND == K_PROP) { r = (int)Field<P>::prop(x[0]); wr = true; }        // the mask: -1 (all ones) or 0
        if constexpr (KIND == K_MODIS1) r = Field<P>::modis1(x[0]);
        if constexpr (KIND == K_MODIS0) r = Field<P>::modis0(x[0]);
        if constexpr (KIND == K_MODSIGN) r = Field<P>::modsign(x[0]);
        if constexpr (KIND == K_MODLIMBS) r = in_limb_budget<P>(x[0]) ? 1 : 0;
        if constexpr (KIND == K_MODHAF) { Field<P>::modhaf(x[0]); wr = true; }
        if constexpr (KIND == K_MODQR) r = Field<P>::modqr(nullptr, x[0]);
        if (wr) store_soa<P, 1>(a, ld, t, x);
        if (out) out[t] = r;
    }
}
template <class P>
__global__ __launch_bounds__(BLOCK) void k_cmp(const spint* a, const spint* b, int* out, size_t n, Ld lda, Ld ldb) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], y[1][P::N];
        load_soa<P, 1>(a, lda, t, x);
        load_soa<P, 1>(b, ldb, t, y);
        out[t] = Field<P>::modcmp(x[0], y[0]);
    }
}
// shifts by less than a word (modshl / modshr), in place; shr returns the shifted-out bits
template <class P, bool LEFT>
__global__ __launch_bounds__(BLOCK) void k_shift(unsigned k, spint* a, int* out, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N];
        load_soa<P, 1>(a, ld, t, x);
        int r = 0;
        if constexpr (LEFT) Field<P>::modshl(k, x[0]); else r = Field<P>::modshr(k, x[0]);
        store_soa<P, 1>(a, ld, t, x);
        if (out) out[t] = r;
    }
}
// fill with a constant element: modzer / modone / modint(x) / mod2r(r)
enum { K_INT = 0, K_2R };
template <class P, int KIND>
__global__ __launch_bounds__(BLOCK) void k_fill(int val, spint* a, size_t n, Ld ld) {
    spint x[1][P::N];
    if constexpr (KIND == K_INT) {
        if (val == 0) Field<P>::modzer(x[0]); else Field<P>::modint(val, x[0]);
    } else {
        Field<P>::mod2r((unsigned)val, x[0]);
    }
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK)
        store_soa<P, 1>(a, ld, t, x);
}

// bytes <-> limbs: AoS records of NBYTES big-endian bytes (what modimp / modexp take), one record per lane.  The integer travels
// as NW little-endian 64-bit words at either word length (field.h limbs_from_words); NBYTES is a multiple of 8 for the three primes
// of this form, so a record moves as 64-bit words (word k of the integer = the byte-swapped chunk NW-1-k).
template <class P>
__device__ __forceinline__ void load_be_record(const unsigned char* bytes, size_t t, word_t* w) {
    constexpr int NW = Field<P>::NW;
    static_assert(P::NBYTES % 8 == 0, "byte records of this form move as 64-bit words");
    const word_t* src = reinterpret_cast<const word_t*>(bytes) + t * NW;
    static_for<0, NW>([&](auto K) { w[K] = __builtin_bswap64(src[NW - 1 - K]); });
}
template <class P>
__device__ __forceinline__ void store_be_record(unsigned char* bytes, size_t t, const word_t* w) {
    constexpr int NW = Field<P>::NW;
    word_t* dst = reinterpret_cast<word_t*>(bytes) + t * NW;
    static_for<0, NW>([&](auto K) { dst[NW - 1 - K] = __builtin_bswap64(w[K]); });
}
template <class P>
__global__ __launch_bounds__(BLOCK) void k_imp(const unsigned char* bytes, spint* a, int* flag, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        word_t w[Field<P>::NW];
        load_be_record<P>(bytes, t, w);
        spint x[1][P::N];
        int r = Field<P>::modimp_words(w, x[0]);
        store_soa<P, 1>(a, ld, t, x);
        if (flag) flag[t] = r;
    }
}
template <class P>
__global__ __launch_bounds__(BLOCK) void k_exp(const spint* a, unsigned char* bytes, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N];
        load_soa<P, 1>(a, ld, t, x);
        word_t w[Field<P>::NW];
        Field<P>::modexp_words(x[0], w);
        store_be_record<P>(bytes, t, w);
    }
}

// Synthetic field elements: the splitmix64 stream and the reduction of kernels.h k_uniform -- element j takes the
// NWD = ceil(Nbits/64)+1 consecutive 64-bit outputs number j*NWD+1 .. j*NWD+NWD as a little-endian integer and reduces it mod p by
// Horner over the words with modmul by nres(2^64) and modadd, then modfsb -- so the SAME integers come out for the same
// (seed, array, first) at either word length, here as the canonical limbs of this form (plain, not nres'd).  plus_p: value + p,
// top limb unmasked.
MA_DEV uint64_t splitmix64_at(uint64_t s0, uint64_t t) {
    uint64_t z = s0 + (t + 1) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}
template <class P>
__global__ __launch_bounds__(BLOCK) void k_uniform(uint64_t s0, size_t first, int plus_p, spint* out, size_t n, Ld ld) {
    using F = Field<P>;
    constexpr int NWD = (P::NBITS + 63) / 64 + 1;
    static_assert(3 * P::RADIX >= 64 && P::N >= 3, "a 64-bit word spreads over three limbs");
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        const uint64_t base = (uint64_t)(first + t) * (uint64_t)NWD;
        spint c[P::N], e[P::N], acc[1][P::N];
        F::mod2r(64, c);
        auto word_elem = [&](int k, spint* x) {                     // one 64-bit word as plain limbs
            const uint64_t w = splitmix64_at(s0, base + (uint64_t)k);
            x[0] = (spint)w & F::MASK;
            x[1] = (spint)(w >> P::RADIX) & F::MASK;
            x[2] = (spint)(w >> (2 * P::RADIX));
            static_for<3, P::N>([&](auto I) { x[I] = 0; });
        };
        word_elem(NWD - 1, acc[0]);
#pragma unroll 1
        for (int k = NWD - 2; k >= 0; k--) {
            F::modmul(acc[0], c, acc[0]);
            word_elem(k, e);
            F::modadd(acc[0], e, acc[0]);
        }
        (void)F::modfsb(acc[0]);
        if (plus_p) {
            F::template addp<1>(acc[0], ~(spint)0);
            (void)F::prop(acc[0]);
        }
        store_soa<P, 1>(out, ld, t, acc);
    }
}

}  // namespace ma32
