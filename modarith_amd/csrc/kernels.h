// modarith_amd/csrc/kernels.h -- batched element-wise field kernels for gfx950, at either word length of csrc/field.h: this one text is
// compiled with MA_WL = 64 (namespace ma, spint = u64) or, through kernels32.h, with MA_WL = 32 (namespace ma32, spint = u32: the
// arithmetic `pseudo.py 32` / `monty.py 32` emit).  A translation unit holds one word length.  What the word length changes:
//   * the product policies.  At 64 bits the split products and the wave vote that guards them (OpMulAuto & co.); the 32-bit primes have
//     P::SPLIT = 0 -- a limb product IS one v_mad_u64_u32 into a 64-bit column, the reference's dpint arithmetic, for every limb pattern --
//     and every vote below folds away under `if constexpr (P::SPLIT > 0)`;
//   * the widest access of a lane, 16 bytes: two elements at 64 bits, four at 32 (EPT, load_soa);
//   * the workgroup of the streaming kernels: BLOCK at 64 bits, taken from the launch at 32 (stream_threads);
//   * the carrier of the two verdict bits of the shared inversion and its admission predicate (InvSimul).
// The templates that only the 64-bit C-ABI instantiates (the Auto functors, the lazy ops, k_mul_shared, k_time) are plain text at 32 bits.
//
// HBM layout: limb-interleaved SoA, buf[limb * ld + j] (spint), the n-lane generalisation of the
// reference's SIMD "batched form" (simd/pseudo_simd.py: a[i] holds limb i of every lane).  One field
// element per lane; lane j of a wave touches consecutive u64 of each limb row, so every limb load
// is one fully coalesced 512-byte (EPT=1) or 1-KiB (EPT=2, 16 B per lane) wave access.  All limbs of
// the operands are loaded before any arithmetic (independent loads in flight), results are stored
// limb row by limb row.  The kernels are HBM-bound streaming kernels: grid-stride over at most
// MA_MAX_BLOCKS workgroups of 256 threads.  No LDS is needed for per-lane data; the shared-multiplicand
// variant broadcasts its common operand from kernel arguments (SGPRs), which is cheaper than LDS.
#pragma once
#include "field.h"

namespace MA_NS {

constexpr int BLOCK = 256;
// The streaming kernels (k_binary, k_unary, k_mli) of the 32-bit form take their workgroup size from the launch: on tiles the rate
// depends on how many elements one workgroup covers (docs/kernels_field.md 4.5), and the C-ABI picks width and workgroup size
// together -- one element per lane may run 512 threads (95 VGPRs at most: no occupancy lost).  At 64 bits the workgroup is BLOCK.
constexpr int stream_block_max(int ept) { return MA_WL == 32 && ept == 1 ? 512 : BLOCK; }
__device__ __forceinline__ size_t stream_threads() { if constexpr (MA_WL == 32) return blockDim.x; else return BLOCK; }

// Batches are streamed once (640 MiB+ per array, far beyond L2 / Infinity Cache): loads and stores carry
// the non-temporal hint so they do not displace each other in the caches (measured +3..5 % on the
// 3-stream pattern, profiles/history/r01_membench.log).
template <int EPT> struct VecOf { typedef spint type __attribute__((ext_vector_type(EPT))); };
template <> struct VecOf<1> { typedef spint type; };
typedef VecOf<2>::type spint2;
#ifndef MA_NONTEMPORAL
#define MA_NONTEMPORAL 1
#endif
template <class T> __device__ __forceinline__ T ld_stream(const T* p) {
#if MA_NONTEMPORAL
    return __builtin_nontemporal_load(p);
#else
    return *p;
#endif
}
template <class T> __device__ __forceinline__ void st_stream(T* p, T v) {
#if MA_NONTEMPORAL
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

// Limb stride descriptor of a batch.  FLAT (ld >= n, the n-lane form of the reference's SIMD "batched form"): limb i of element
// j at buf[i * ld + j].  TILED (ld = 2^s < n): the batch is a sequence of tiles of ld elements, each tile limb-interleaved with
// stride ld, tiles N * ld words apart -- buf[((j >> s) * N + i) * ld + (j & (ld - 1))].  One formula serves both: the flat case
// carries s = 63, so that j >> s = 0 and j & (2^s - 1) = j.  Why tiles: with rows of 2^12 elements (32 KiB) the N limb rows a
// workgroup streams lie within one contiguous 160 KiB (5 limbs) / 256 KiB (8 limbs) stretch instead of N stretches 128 MiB
// apart, and the streaming rate no longer depends on where the driver placed the arrays (profiles/history/r03_tiled_exp_*).
struct Ld {
    size_t ld;
    unsigned s;
    __host__ __device__ Ld(size_t ld_ = 0) : ld(ld_), s(63) {}
    __host__ __device__ Ld(size_t ld_, unsigned s_) : ld(ld_), s(s_) {}
    template <int N>
    __host__ __device__ __forceinline__ size_t off(size_t j) const { return (((j >> s) * (size_t)N) << s) + (j & ((((size_t)1) << s) - 1)); }
};

// element index handled by (thread t, slot e): j = EPT*t + e  -> contiguous EPT words per lane, 16 bytes at the most
template <class P, int EPT>
__device__ __forceinline__ void load_soa(const spint* base, Ld L, size_t t, spint (*x)[P::N]) {
    static_assert(EPT == 1 || EPT == 2 || (EPT == 4 && MA_WL == 32), "one or two elements per lane, four of 32-bit limbs");
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
// The functors over a product carry the product policy at 64 bits (FAST: the split products of field.h).  The 32-bit form has one
// policy and its functors no such parameter: their names are part of the kernel symbols (ma32::k_unary<P, ma32::OpSqr<P>, 4>).
#if MA_WL == 64
#define MA_POLICY_OP template <class P, bool FAST = false>
#define MA_POLICY_FIELD Field<P, FAST>
#else
#define MA_POLICY_OP template <class P>
#define MA_POLICY_FIELD Field<P>
#endif
// the field on the split products where the prime has them (what a kernel runs after a vote in its favour), else the exact one
template <class P> using FieldVoted = Field<P, (P::SPLIT > 0)>;
MA_POLICY_OP struct OpMul { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { MA_POLICY_FIELD::modmul(a, b, c); } };
template <class P> struct OpAdd { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modadd(a, b, c); } };
template <class P> struct OpSub { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modsub(a, b, c); } };
template <class P> struct OpAddLazy { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modadd_lazy(a, b, c); } };
template <class P> struct OpSubLazy { static MA_DEV void apply(const spint* a, const spint* b, spint* c) { Field<P>::modsub_lazy(a, b, c); } };
// modmul / modsqr with a wave-uniform choice of product policy: the split products (Field<P,true>, fewer VALU
// instructions) when every active lane's operands are inside their limb contract (< 2^(Radix+2), field.h), the exact
// 128-bit products otherwise -- identical results either way, for every input
// (radix 62 and up: 2^(Radix+2) does not fit a word, every 64-bit limb is below it -- the predicate is vacuously true,
// and a shift by 64 would be undefined)
template <class P> MA_DEV bool in_split_contract(const spint* a) {
    if constexpr (P::RADIX + 2 >= 64) {
        return true;
    } else {
        spint m = 0;
        static_for<0, P::N>([&](auto I) { m |= a[I]; });
        return (m >> (P::RADIX + 2)) == 0;
    }
}
// the budget modlimbs / Curve.limbs_ok report: 2^(Radix+2) as above, except for the 5 x 52-bit pseudo-Mersenne primes whose curve
// kernels run the folded half-limb products (field.h FOLD52, 2^256-189): there the reference itself wraps mm * a_k at 64
// bits, and the two product forms agree only for limbs up to (2^64-1)/mm (2^52.4) -- which every field-function output keeps
template <class P> MA_DEV bool in_limb_budget(const spint* a) {
    constexpr bool fold52 = !P::MONTGOMERY && P::EPM && !P::OVERFLOW && P::RADIX == 52 && P::N == 5 && P::MM < (1ull << 16) && P::SPLIT == 0;
    if constexpr (fold52) {
        bool ok = true;
        static_for<0, P::N>([&](auto I) { ok = ok & (a[I] <= ~(spint)0 / (spint)P::MM); });      // (&: no short-circuit branch per limb)
        return ok;
    } else {
        return in_split_contract<P>(a);
    }
}
template <class P> struct OpMulAuto {
    static MA_DEV void apply(const spint* a, const spint* b, spint* c) {
        if constexpr (P::SPLIT > 0) {
            if (__all(in_split_contract<P>(a) && in_split_contract<P>(b))) { Field<P, true>::modmul(a, b, c); return; }
        }
        Field<P, false>::modmul(a, b, c);
    }
};
template <class P> struct OpSqrAuto {
    static MA_DEV void apply(const spint* a, spint* c) {
        if constexpr (P::SPLIT > 0) {
            if (__all(in_split_contract<P>(a))) { Field<P, true>::modsqr(a, c); return; }
        }
        Field<P, false>::modsqr(a, c);
    }
};
template <class P> struct OpNresAuto {
    static MA_DEV void apply(const spint* a, spint* c) {
        if constexpr (P::SPLIT > 0 && P::MONTGOMERY) {
            if (__all(in_split_contract<P>(a))) { Field<P, true>::nres(a, c); return; }
        }
        Field<P, false>::nres(a, c);
    }
};
template <class P> struct OpRedcAuto {
    static MA_DEV void apply(const spint* a, spint* c) {
        if constexpr (P::SPLIT > 0 && P::MONTGOMERY) {
            if (__all(in_split_contract<P>(a))) { Field<P, true>::redc(a, c); return; }
        }
        Field<P, false>::redc(a, c);
    }
};
// The 8-byte-per-lane kernels (EPT = 1: unaligned buffers, odd limb strides, the last element of an odd batch) run the exact
// products instead of the per-wave choice: compiled with EPT = 1 the two-path functors were allocated 217 (5 limbs) to 512
// (8 limbs: 256 VGPRs + 256 AGPRs, a v_accvgpr copy around every multiply-add) registers, and unaligned X448 batches
// streamed at 2.0 TB/s.  The exact path is right for every input, needs 66-100 VGPRs, and at 8 bytes per lane the kernel
// is not faster than its arithmetic anyway.
template <class Op> struct ScalarOp { using type = Op; };
template <class P> struct ScalarOp<OpMulAuto<P>> { using type = OpMul<P>; };
MA_POLICY_OP struct OpSqr { static MA_DEV void apply(const spint* a, spint* c) { MA_POLICY_FIELD::modsqr(a, c); } };
template <class P> struct ScalarOp<OpSqrAuto<P>> { using type = OpSqr<P>; };
template <class P> struct OpNeg { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modneg(a, c); } };
template <class P> struct OpNegLazy { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modneg_lazy(a, c); } };
MA_POLICY_OP struct OpNres { static MA_DEV void apply(const spint* a, spint* c) { MA_POLICY_FIELD::nres(a, c); } };
MA_POLICY_OP struct OpRedc { static MA_DEV void apply(const spint* a, spint* c) { MA_POLICY_FIELD::redc(a, c); } };
template <class P> struct ScalarOp<OpNresAuto<P>> { using type = OpNres<P>; };
template <class P> struct ScalarOp<OpRedcAuto<P>> { using type = OpRedc<P>; };
template <class P> struct OpCpy { static MA_DEV void apply(const spint* a, spint* c) { Field<P>::modcpy(a, c); } };
// modinv of the batched API returns the inverse in NORMALISED form nres(redc(1/a)): limbs that are a function of the value alone
// (canonical limbs for the pseudo-Mersenne fields, the Montgomery form of the canonical value otherwise).  The reference's
// modinv leaves whatever its addition chain leaves -- a chain this library does not share (the reference's comes from an
// external tool), so its limbs were never comparable before redc -- and normalising makes the per-element kernel, the
// progenitor form and the simultaneous-inversion kernel (k_inv_simul) return the same words for the same value.
template <class F> MA_DEV void inv_normalise(spint* z) {
    spint t[F::N];
    F::redc(z, t);
    F::nres(t, z);
}
MA_POLICY_OP struct OpInv {
    static MA_DEV void apply(const spint* a, spint* c) {
        MA_POLICY_FIELD::modinv(a, nullptr, c);
        inv_normalise<MA_POLICY_FIELD>(c);          // (1/a is a product of field-function outputs: inside the limb contract)
    }
};
MA_POLICY_OP struct OpSqrt { static MA_DEV void apply(const spint* a, spint* c) { MA_POLICY_FIELD::modsqrt(a, nullptr, c); } };
MA_POLICY_OP struct OpPro { static MA_DEV void apply(const spint* a, spint* c) { MA_POLICY_FIELD::modpro(a, c); } };
// the long chains (x^PE and what hangs on it: ~250-450 squarings + multiplications per element) with the same wave-uniform
// choice as OpMulAuto: split / half-limb products when every lane's input is inside the limb contract (the chain then stays
// inside it by closure), exact ones otherwise -- the same limbs either way
template <class P, template <class, bool> class Op> struct OpAutoUnary {
    static MA_DEV void apply(const spint* a, spint* c) {
        if constexpr (P::SPLIT > 0) {
            if (__all(in_split_contract<P>(a))) { Op<P, true>::apply(a, c); return; }
        }
        Op<P, false>::apply(a, c);
    }
};

// c[j] = op(a[j], b[j])
template <class P, class Op, int EPT>
__global__ __launch_bounds__(stream_block_max(EPT)) void k_binary(const spint* a, const spint* b,
                                                                  spint* c, size_t nthreads, Ld lda, Ld ldb, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * stream_threads() + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * stream_threads()) {
        spint x[EPT][P::N], y[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        load_soa<P, EPT>(b, ldb, t, y);
        // (the slots written out, not `#pragma unroll` or static_for: for the 8-limb two-path functors the optimizer declined to unroll
        // the loop -- "loop not unrolled" for ED448Q / SIDH434 -- which leaves x[e] indexed at run time, i.e. in scratch)
        Op::apply(x[0], y[0], z[0]);
        if constexpr (EPT >= 2) Op::apply(x[1], y[1], z[1]);
        if constexpr (EPT == 4) { Op::apply(x[2], y[2], z[2]); Op::apply(x[3], y[3], z[3]); }
        store_soa<P, EPT>(c, ldc, t, z);
    }
}

// c[j] = op(a[j]) for the long chains (modinv, modsqrt, modpro): same body as k_unary below, but compiled for at least
// three waves per SIMD on the small fields -- with only __launch_bounds__(256) the register allocator may take 512
// VGPRs, and it does (400 for the pinned half-limb products of modinv): one wave per SIMD on a latency-bound chain
template <class P> constexpr int heavy_waves() { return (MA_WL == 32 || P::N <= 5) ? 3 : 1; }
template <class P, class Op>
__global__ __launch_bounds__(BLOCK) __attribute__((amdgpu_waves_per_eu(heavy_waves<P>())))
void k_unary_heavy(const spint* a, spint* c, size_t nthreads, Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], z[1][P::N];
        load_soa<P, 1>(a, lda, t, x);
        Op::apply(x[0], z[0]);
        store_soa<P, 1>(c, ldc, t, z);
    }
}

// c[j] = op(a[j])
template <class P, class Op, int EPT>
__global__ __launch_bounds__(stream_block_max(EPT)) void k_unary(const spint* a, spint* c, size_t nthreads,
                                                                 Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * stream_threads() + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * stream_threads()) {
        spint x[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        Op::apply(x[0], z[0]);
        if constexpr (EPT >= 2) Op::apply(x[1], z[1]);
        if constexpr (EPT == 4) { Op::apply(x[2], z[2]); Op::apply(x[3], z[3]); }
        store_soa<P, EPT>(c, ldc, t, z);
    }
}

// shared multiplicand: c[j] = a[j] * b0, b0 passed by value (lands in SGPRs, broadcast to all lanes).
// AUTO: the per-wave product policy of OpMulAuto with the vote on a[] only -- the host has already checked b0 against
// the limb contract (capi_prime.inc modmuls), and everything the split / half-limb products derive from b0 alone (its halves,
// mm * half, the prepared Opd pairs) is wave-uniform: the compiler keeps it in SGPRs, computed once per kernel in
// scalar ALU, and every multiply-add reads ONE scalar and one vector source (the VOP3 constant-bus limit), so no
// v_mov / s_nop copies surround the products as they do around the exact 64 x 64 -> 128 ones.  Same limbs either way.
template <class P> struct Elem { spint l[P::N]; };
template <class P, bool AUTO>
MA_DEV void mul_shared_one(const spint* x, const spint* b, spint* z) {
    if constexpr (AUTO && P::SPLIT > 0) {
        if (__all(in_split_contract<P>(x))) { Field<P, true>::modmul(x, b, z); return; }
    }
    Field<P, false>::modmul(x, b, z);
}
template <class P, int EPT, bool AUTO>
__global__ __launch_bounds__(BLOCK) void k_mul_shared(const spint* a, Elem<P> b0, spint* c,
                                                      size_t nthreads, Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * BLOCK) {
        spint x[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        // one element at a time, each with its own vote (as OpMulAuto): voting once for both elements lets the scheduler
        // interleave two products and takes 136 VGPRs instead of 64
        static_assert(EPT == 1 || EPT == 2, "one or two elements per lane");
        mul_shared_one<P, AUTO>(x[0], b0.l, z[0]);
        if constexpr (EPT == 2) mul_shared_one<P, AUTO>(x[1], b0.l, z[1]);
        store_soa<P, EPT>(c, ldc, t, z);
    }
}

// c[j] = a[j] * b (small integer)
template <class P, int EPT>
__global__ __launch_bounds__(stream_block_max(EPT)) void k_mli(const spint* a, int b, spint* c, size_t nthreads,
                                                               Ld lda, Ld ldc) {
    for (size_t t = (size_t)blockIdx.x * stream_threads() + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * stream_threads()) {
        spint x[EPT][P::N], z[EPT][P::N];
        load_soa<P, EPT>(a, lda, t, x);
        Field<P>::modmli(x[0], b, z[0]);
        if constexpr (EPT >= 2) Field<P>::modmli(x[1], b, z[1]);
        if constexpr (EPT == 4) { Field<P>::modmli(x[2], b, z[2]); Field<P>::modmli(x[3], b, z[3]); }
        store_soa<P, EPT>(c, ldc, t, z);
    }
}

// a[j] = a[j]^(2^k)
template <class P>
__global__ __launch_bounds__(BLOCK) void k_nsqr(spint* a, int k, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N];
        load_soa<P, 1>(a, ld, t, x);
        // the vote is taken before EVERY squaring, not once on the input: the limb contract is not closed under squaring for every input
        // inside it.  A Montgomery product leaves its top limb unmasked, below (v(a)^2 / R + p) >> Radix (Nlimbs - 1); with 2^(Radix+2) - 1
        // in every limb the value is 4 * 2^(Radix Nlimbs) and the square's top limb reaches 2^(Radix+4) -- outside the contract of the
        // split products, which then returned other words than the reference from the second squaring on (tests/test_gpu_edge_products.py;
        // NIST256, k = 5, a = [1fffffffffffff x 5]: limb 4 = 55e30b312da0744, reference c660b78c46b68bd4)
        // (one policy at 32 bits, nothing to vote on: the field's own loop -- the loop below with `fast` folded away is allocated
        // other registers)
        if constexpr (MA_WL == 32) {
            Field<P>::modnsqr(x[0], k);
        } else {
#pragma unroll 1
            for (int i = 0; i < k; i++) {
                bool fast = false;
                if constexpr (P::SPLIT > 0) fast = __all(in_split_contract<P>(x[0]));
                if (fast) Field<P, true>::modsqr(x[0], x[0]); else Field<P, false>::modsqr(x[0], x[0]);
            }
        }
        store_soa<P, 1>(a, ld, t, x);
    }
}

// z[j] = 1/x[j] with caller-supplied progenitor h[j] (modinv(x,h,z), pseudo.py:788-812)
template <class P>
__global__ __launch_bounds__(BLOCK) void k_inv_h(const spint* xs, const spint* hs,
                                                 spint* zs, size_t n, Ld ldx, Ld ldh, Ld ldz) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], h[1][P::N], z[1][P::N];
        load_soa<P, 1>(xs, ldx, t, x);
        load_soa<P, 1>(hs, ldh, t, h);
        bool fast = false;
        if constexpr (P::SPLIT > 0) fast = __all(in_split_contract<P>(x[0]) && in_split_contract<P>(h[0]));
        if (fast) { FieldVoted<P>::modinv(x[0], h[0], z[0]); inv_normalise<FieldVoted<P>>(z[0]); }
        else { Field<P, false>::modinv(x[0], h[0], z[0]); inv_normalise<Field<P, false>>(z[0]); }
        store_soa<P, 1>(zs, ldz, t, z);
    }
}

// z[j] = 1/x[j] for a whole batch with ONE inversion per `rounds` elements (Montgomery's simultaneous inversion).  modinv is
// ~265 field multiplications (38 700 VALU instructions for 2^255-19); a batch does not owe one to every element.  Lane j of L
// takes the elements {r * L + j : r < rounds} (every access of a wave is one coalesced row): forward, it multiplies them up,
// leaving the prefix products c_r in cs (the output buffer itself, or scratch when the output aliases the input);
// then it inverts the last product; backward, 1/x_r = inv * c_{r-1} and inv *= x_r.
// No element may spoil the result of another, whatever its limbs.  Two kinds are kept out of the shared product by lane
// predication (c_r = c_{r-1}), their verdicts travelling to the backward pass in a carrier that depends on the word length
// (InvSimul::IN_LIMB below):
//   * zero values -- tested on the PRODUCT c_{r-1} * x_r, a field-function output, where modis0 is exact whatever the
//     representation of x_r (0, p, even 2p); their output is zero, as modinv(0) = 0 in the reference (pseudo.py:788-812) and as the
//     per-element kernel gives (every product of its chain is then 0 or p, and the normalisation makes that 0);
//   * elements outside the contract of the products (fabricated; the reference's behaviour on them is its wrap-around):
//     they get an inversion of their own on the exact products in the backward pass -- exactly what the per-element
//     kernel does for a wave that holds one -- paid by that wave only.
// Everything that enters a product is therefore inside the contract: all products run on the split forms where the prime has
// them.  Outputs in normalised form (inv_normalise): the same words as the per-element kernel for every input.
// The contract is in_split_contract at 64 bits, inv_in_contract at 32:
//
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

template <class P>
struct InvSimul {
    using F0 = Field<P, false>;
    using F1 = FieldVoted<P>;
    // where the two verdicts of a round travel.  64 bits: in bits 63 / 62 of the stored prefix's top limb (free: prefixes are inside
    // the limb contract and the path is taken for radix <= 60 only).  32 bits: in two per-lane 64-bit masks, bit r for round r (the
    // 29-bit limbs of that form have no spare bits once the top limb is unmasked, and rounds <= 64).
    static constexpr bool IN_LIMB = MA_WL == 64;
    static constexpr spint ZERO = (spint)1 << (MA_WL - 1), OOC = (spint)1 << (MA_WL - 2);
    static MA_DEV bool admitted(const spint* x) {
        if constexpr (MA_WL == 64) return in_split_contract<P>(x); else return inv_in_contract<P>(x);
    }
    static MA_DEV void run(const spint* xs, spint* zs, spint* cs, size_t n, size_t L, int rounds, Ld ldx, Ld ldz, Ld ldc, size_t j) {
        spint c[P::N], x[1][P::N], t[1][P::N];
        uint64_t zeros = 0, oocs = 0;
        F1::modone(c);
#pragma unroll 1
        for (int r = 0; r < rounds; r++) {
            const size_t e = (size_t)r * L + j;
            if (e >= n) break;                                  // (e grows with r)
            load_soa<P, 1>(xs, ldx, e, x);
            const bool ooc = !admitted(x[0]);
            F1::modmul(c, x[0], t[0]);                          // (discarded for an out-of-contract x)
            const bool zero = !ooc && F1::modis0(t[0]) != 0;
            const bool skip = ooc || zero;
            static_for<0, P::N>([&](auto I) { c[I] = skip ? c[I] : t[0][I]; });
            static_for<0, P::N>([&](auto I) { t[0][I] = c[I]; });
            if constexpr (IN_LIMB) {
                t[0][P::N - 1] |= (zero ? ZERO : (spint)0) | (ooc ? OOC : (spint)0);
            } else {
                zeros |= (uint64_t)zero << r;
                oocs |= (uint64_t)ooc << r;
            }
            store_soa<P, 1>(cs, ldc, e, t);
        }
        spint inv[P::N];
        F1::modinv(c, nullptr, inv);
#pragma unroll 1
        for (int r = rounds - 1; r >= 0; r--) {
            const size_t e = (size_t)r * L + j;
            if (e >= n) continue;
            load_soa<P, 1>(xs, ldx, e, x);
            bool zero, ooc;
            if constexpr (IN_LIMB) {
                const spint flags = cs[ldc.template off<P::N>(e) + (size_t)(P::N - 1) * ldc.ld];
                zero = (flags & ZERO) != 0, ooc = (flags & OOC) != 0;
            } else {
                zero = (zeros >> r) & 1, ooc = (oocs >> r) & 1;
            }
            spint zi[P::N];
            if (r > 0) {
                load_soa<P, 1>(cs, ldc, e - L, t);
                if constexpr (IN_LIMB) t[0][P::N - 1] &= ~(ZERO | OOC);
                F1::modmul(inv, t[0], zi);                      // inv * c_{r-1}
                F1::modmul(inv, x[0], t[0]);
                static_for<0, P::N>([&](auto I) { inv[I] = (zero || ooc) ? inv[I] : t[0][I]; });
            } else {
                static_for<0, P::N>([&](auto I) { zi[I] = inv[I]; });
            }
            inv_normalise<F1>(zi);
            static_for<0, P::N>([&](auto I) { zi[I] = zero ? (spint)0 : zi[I]; });
            if (__any(ooc)) {                                   // fabricated limbs somewhere in this wave: their own inversion, exact products
                spint w[P::N];
                F0::modinv(x[0], nullptr, w);
                inv_normalise<F0>(w);
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
        bool fast = false;
        if constexpr (P::SPLIT > 0) fast = __all(in_split_contract<P>(x[0]) && in_split_contract<P>(h[0]));
        if constexpr (QR) {
            out[t] = fast ? FieldVoted<P>::modqr(h[0], x[0]) : Field<P, false>::modqr(h[0], x[0]);
        } else {
            if (fast) FieldVoted<P>::modsqrt(x[0], h[0], r[0]); else Field<P, false>::modsqrt(x[0], h[0], r[0]);
            store_soa<P, 1>(rs, ld, t, r);
        }
    }
}

// constant-time conditional swap / move with a per-element selector d[j] in {0,1}
// (simd/pseudo_simd.py:1121-1162: selector widened to one value per lane)
template <class P, bool SWAP>
__global__ __launch_bounds__(BLOCK) void k_cond(const int* d, spint* g, spint* f, size_t n,
                                                Ld ldg, Ld ldf) {
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
        if constexpr (KIND == K_MODLIMBS) r = in_limb_budget<P>(x[0]) ? 1 : 0;      // every limb < 2^(Radix+2) (FOLD52 primes: <= (2^64-1)/mm)
        if constexpr (KIND == K_MODHAF) { Field<P>::modhaf(x[0]); wr = true; }
        if constexpr (KIND == K_MODQR) {
            bool fast = false;
            if constexpr (P::SPLIT > 0) fast = __all(in_split_contract<P>(x[0]));
            r = fast ? FieldVoted<P>::modqr(nullptr, x[0]) : Field<P, false>::modqr(nullptr, x[0]);
        }
        if (wr) store_soa<P, 1>(a, ld, t, x);
        if (out) out[t] = r;
    }
}

template <class P>
__global__ __launch_bounds__(BLOCK) void k_cmp(const spint* a, const spint* b, int* out,
                                               size_t n, Ld lda, Ld ldb) {
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

// bytes <-> limbs.  AoS records of NBYTES big-endian bytes (what modimp / modexp take), one record per
// lane.  The integer travels as NW little-endian 64-bit words at either word length (field.h limbs_from_words).  When
// NBYTES is a multiple of 8 the record moves as 64-bit words (word k of the integer = the
// byte-swapped chunk NW-1-k); otherwise (e.g. 66-byte NIST521 records) bytes are assembled one by one.
template <class P>
__device__ __forceinline__ void load_be_record(const unsigned char* bytes, size_t t, word_t* w) {
    constexpr int NW = Field<P>::NW, NB = P::NBYTES;
    if constexpr (NB % 8 == 0) {
        const word_t* src = reinterpret_cast<const word_t*>(bytes) + t * NW;
        static_for<0, NW>([&](auto K) { w[K] = __builtin_bswap64(src[NW - 1 - K]); });
    } else if constexpr (MA_WL == 32) {
        // The same, with every byte taken through a register the compiler knows nothing about.  For 30-byte records and 29-bit limbs
        // (GM240 at word length 32) hipcc folds the OR of the byte loads of limb 0 into one v_perm_b32 whose selector puts byte 28
        // into bits 24..31 as a filler, ORs byte 26 on top and masks with 2^29 - 1 only: bits 24..28 of the limb then hold
        // (byte 28 | byte 26) & 0x1f.  Seen in the disassembly and on the device (limb 0 off by 2^28 for one record in two); the
        // host build of the same text is right.  Opaque bytes keep the fold from forming; the built-in primes of this word length
        // have records of 32 and 56 bytes and never come here.
        const unsigned char* src = bytes + t * NB;
        static_for<0, NW>([&](auto K) { w[K] = 0; });
        static_for<0, NB>([&](auto B) {
            constexpr int pos = NB - 1 - B;                 // byte significance (0 = least)
            uint32_t by = src[B];
            asm volatile("" : "+v"(by));
            w[pos / 8] |= (word_t)by << (8 * (pos % 8));
        });
    } else {
        // (64-bit words keep the plain form, whose code the change above must not touch.  The same source pattern could fold the same
        // way: the 30-byte GM240 unit has no v_perm_b32 in k_imp at all, the 66-byte NIST521 unit has seven that nobody has traced
        // byte by byte.  What guards them is tests/test_gpu_parity.py test_golden_bytes -- the reference's modimp on fixed and random
        // records for every prime, on the device -- so a compiler that folds them wrongly fails that test; re-inspect the
        // disassembly of k_imp for the primes whose NBYTES is no multiple of 8 when the compiler changes.)
        const unsigned char* src = bytes + t * NB;
        static_for<0, NW>([&](auto K) { w[K] = 0; });
        static_for<0, NB>([&](auto B) {
            constexpr int pos = NB - 1 - B;                 // byte significance (0 = least)
            w[pos / 8] |= (word_t)src[B] << (8 * (pos % 8));
        });
    }
}
template <class P>
__device__ __forceinline__ void store_be_record(unsigned char* bytes, size_t t, const word_t* w) {
    constexpr int NW = Field<P>::NW, NB = P::NBYTES;
    if constexpr (NB % 8 == 0) {
        word_t* dst = reinterpret_cast<word_t*>(bytes) + t * NW;
        static_for<0, NW>([&](auto K) { dst[NW - 1 - K] = __builtin_bswap64(w[K]); });
    } else {
        unsigned char* dst = bytes + t * NB;
        static_for<0, NB>([&](auto B) {
            constexpr int pos = NB - 1 - B;
            dst[B] = (unsigned char)(w[pos / 8] >> (8 * (pos % 8)));
        });
    }
}
// What a fused call hands back of the affine point (xw, yw) of record t (ecnXXXget): the x record if asked for, the y record if asked
// for, and the sign: the parity of the coordinate that is NOT written (of y first), 0 when both are
template <class P>
__device__ __forceinline__ void store_affine_be(unsigned char* xb, unsigned char* yb, int* sign, size_t t, const word_t* xw, const word_t* yw) {
    if (xb) store_be_record<P>(xb, t, xw);
    if (yb) store_be_record<P>(yb, t, yw);
    if (sign) sign[t] = !yb ? (int)(yw[0] & 1) : (!xb ? (int)(xw[0] & 1) : 0);
}
// The three coordinates of record first + t of a batch of projective points: limb rows ld apart, X's N rows, then Y's, then Z's.  t: the
// index, or a callable that yields it and is called afresh for every limb -- the kernels that keep a 64-bit index out of their loops that
// way (one index held across the fifteen loads spilled two more scalar registers in k_ed448_mul2_straus)
template <int N, class T>
__device__ __forceinline__ void load_xyz(const spint* B, size_t ld, size_t first, T t, spint* X, spint* Y, spint* Z) {
    auto at = [&]() -> size_t {
        if constexpr (std::is_invocable_v<T>) return t();
        else return t;
    };
    static_for<0, N>([&](auto I) {
        X[I] = B[(size_t)I * ld + first + at()];
        Y[I] = B[(size_t)(N + I) * ld + first + at()];
        Z[I] = B[(size_t)(2 * N + I) * ld + first + at()];
    });
}
// The same records least significant byte first (the RFC 7748 / RFC 8032 wire formats; what the reference's reverse() makes of them
// before modimp): word k of the integer is chunk k as it lies in memory, no swap and no reversal of the word order; bytes are
// assembled one by one where NBYTES is no multiple of 8, at word length 32 through the opaque form of load_be_record -- the same
// source pattern, open to the same fold.  Used by the fused chains (csrc/chain.inc)
template <class P>
__device__ __forceinline__ void load_le_record(const unsigned char* bytes, size_t t, word_t* w) {
    constexpr int NW = Field<P>::NW, NB = P::NBYTES;
    if constexpr (NB % 8 == 0) {
        const word_t* src = reinterpret_cast<const word_t*>(bytes) + t * NW;
        static_for<0, NW>([&](auto K) { w[K] = src[K]; });
    } else {
        const unsigned char* src = bytes + t * NB;
        static_for<0, NW>([&](auto K) { w[K] = 0; });
        static_for<0, NB>([&](auto B) {
            constexpr int pos = B;                          // byte significance (0 = least)
            uint32_t by = src[B];
            if constexpr (MA_WL == 32) asm volatile("" : "+v"(by));
            w[pos / 8] |= (word_t)by << (8 * (pos % 8));
        });
    }
}
template <class P>
__device__ __forceinline__ void store_le_record(unsigned char* bytes, size_t t, const word_t* w) {
    constexpr int NW = Field<P>::NW, NB = P::NBYTES;
    if constexpr (NB % 8 == 0) {
        word_t* dst = reinterpret_cast<word_t*>(bytes) + t * NW;
        static_for<0, NW>([&](auto K) { dst[K] = w[K]; });
    } else {
        unsigned char* dst = bytes + t * NB;
        static_for<0, NB>([&](auto B) { dst[B] = (unsigned char)(w[B / 8] >> (8 * (B % 8))); });
    }
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

// Synthetic field elements for benchmarks and full-size tests (SURVEY 8(d) input recipe): a splitmix64 stream keyed by
// (seed, array id); element j takes the NWD = ceil(Nbits/64)+1 consecutive outputs number j*NWD+1 .. j*NWD+NWD as a
// little-endian integer (bias below 2^-64) and reduces it mod p with field calls only -- Horner over the words with
// modmul by nres(2^64) (keeps plain values plain) and modadd, then modfsb -- leaving the CANONICAL limbs of a value
// uniform in [0,p) (plain, not nres'd).  plus_p: the same value + p, top limb unmasked: a representative in [p,2p).
// Regenerable on the host from (seed, array, j) alone (tests/util.py uniform_model).  The stream is one of 64-bit words at either word
// length, so the SAME integers come out for the same (seed, array, first), in the limbs of the form.
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
    constexpr int NLW = (64 + P::RADIX - 1) / P::RADIX;             // limbs a 64-bit word spreads over: two at 64 bits, three at 32
    static_assert(P::N >= NLW, "a 64-bit word fits the element");
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        const uint64_t base = (uint64_t)(first + t) * (uint64_t)NWD;
        spint c[P::N], e[P::N], acc[1][P::N];
        F::mod2r(64, c);
        auto word_elem = [&](int k, spint* x) {                     // one 64-bit word as plain limbs
            const uint64_t w = splitmix64_at(s0, base + (uint64_t)k);
            static_for<0, NLW - 1>([&](auto I) { x[I] = (spint)(w >> (I * P::RADIX)) & F::MASK; });
            x[NLW - 1] = (spint)(w >> ((NLW - 1) * P::RADIX));
            static_for<NLW, P::N>([&](auto I) { x[I] = 0; });
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

// The reference's timing protocol on the GPU (time.c: pseudo.py:1177-1386; its CUDA form
// simd/pseudo_cuda.py:1163-1231 runs the same dependent chains inside one thread): every lane runs the
// serially dependent chain on its own operands, entirely in registers, and leaves redc(z).
// KIND 0: `outer` x 200 x 5 modmul;  1: `outer` x 500 x 2 modsqr;  2: `outer` x 2 modinv.
template <class F, class P, int KIND>
MA_DEV void time_chain(spint* x, spint* y, spint* z, long outer) {
    // long fields: one out-of-line copy of the product / squaring (field.h chain_mul, chain_nsqr) instead of five / two inlined ones per
    // policy -- k_time<SIDH610, 0, 2> stood at 329 registers with both policies' chains inlined
    constexpr bool OOL = P::N >= 9;
    auto mul = [](const spint* a, const spint* b, spint* c) { if constexpr (OOL) F::chain_mul(a, b, c); else F::modmul(a, b, c); };
    F::nres(x, x);
    if constexpr (KIND == 0) {
        F::nres(y, y);
#pragma unroll 1
        for (long i = 0; i < outer * 200; i++) {
            mul(x, y, z);
            mul(z, x, y);
            mul(y, z, x);
            mul(x, y, z);
            mul(z, x, y);
        }
    } else if constexpr (KIND == 1) {
#pragma unroll 1
        for (long i = 0; i < outer * 500; i++) {
            if constexpr (OOL) {
                F::modcpy(x, z);
                F::chain_nsqr(z, 1);
                F::modcpy(z, x);
                F::chain_nsqr(x, 1);
            } else {
                F::modsqr(x, z);
                F::modsqr(z, x);
            }
        }
    } else {
#pragma unroll 1
        for (long i = 0; i < outer; i++) {
            F::modinv(x, nullptr, z);
            F::modinv(z, nullptr, x);
        }
    }
    F::redc(z, z);
}
// POLICY 0: exact products; 1: split products, unguarded (MA_FORCE_FAST); 2: the wave vote of OpMulAuto, taken once on the
// operands -- the chain then stays inside the limb contract by closure (every link is a field-function output)
template <class P, int KIND, int POLICY = 0>
__global__ __launch_bounds__(BLOCK) void k_time(const spint* xs, const spint* ys, spint* zs, long outer, size_t n, Ld ld) {
    for (size_t t = (size_t)blockIdx.x * BLOCK + threadIdx.x; t < n; t += (size_t)gridDim.x * BLOCK) {
        spint x[1][P::N], y[1][P::N], z[1][P::N];
        load_soa<P, 1>(xs, ld, t, x);
        if constexpr (KIND == 0) load_soa<P, 1>(ys, ld, t, y);
        else static_for<0, P::N>([&](auto I) { y[0][I] = 0; });
        bool fast = POLICY == 1;
        if constexpr (POLICY == 2 && P::SPLIT > 0) fast = __all(in_split_contract<P>(x[0]) && in_split_contract<P>(y[0]));
        if constexpr (POLICY != 0 && P::SPLIT > 0) {
            if (fast) { time_chain<Field<P, true>, P, KIND>(x[0], y[0], z[0], outer); store_soa<P, 1>(zs, ld, t, z); continue; }
        }
        time_chain<Field<P, false>, P, KIND>(x[0], y[0], z[0], outer);
        store_soa<P, 1>(zs, ld, t, z);
    }
}

}  // namespace MA_NS
