// tools/field_fast_host.hip -- both product arithmetics of csrc/field.h, ma::Field<P, false> (exact: 128-bit columns) and
// ma::Field<P, true> (FAST: operands cut at P::SPLIT, 64-bit accumulators, column chain, half-limb forms), compiled for the HOST
// into a shared library for a LIST of primes, so that tests/test_fast_products_host.py can drive every prime's forms with limbs at
// the edge of the limb budget (every limb 2^(Radix+2) - 1: the one input the overflow proofs of emit.split_point / chain_ok /
// sparse_terms are about) and compare limb for limb with the CPU oracle.  Test tooling, not product code.
//
// The list of primes is not kept here: the translation unit is compiled with -DFFH_LIST='"<file>"', a file of
//     #include "params_<PRIME>.h"      (one line per prime)
//     #define FFH_PRIMES(X) X(<PRIME>) X(<PRIME>) ...
// which the test writes from emit.BUILT_PRIMES and generate.EXAMPLES; several such units keep the build time of one unit down.
//   hipcc -O1 -std=c++17 -w -shared -fPIC --offload-host-only -I modarith_amd/csrc/generated -I modarith_amd/csrc \
//         -DFFH_LIST='"/tmp/list_0.inc"' tools/field_fast_host.hip -o /tmp/libfield_fast_host_0.so
//
// Batches are limb-major, as everywhere in the library and the oracle: limb i of element j at a[i * n + j].
#define MA_DEV __host__ __device__ inline
#include <hip/hip_runtime.h>
// field.h's out-of-line chain primitives (chain_nsqr, chain_mul) and the generated progenitor chains (P::modpro_chain) are declared
// __device__ only; for this host-only build they become host functions as well
#undef __device__
#define __device__ __attribute__((host)) __attribute__((device))
#include "../modarith_amd/csrc/field.h"
#ifndef FFH_LIST
#error "compile with -DFFH_LIST='\"<list file>\"' (see the head of this file)"
#endif
#include FFH_LIST
#include <stddef.h>
#include <string.h>

namespace {

enum { OP_MODMUL, OP_MODSQR, OP_NRES, OP_REDC, OP_MODNSQR, OP_MODINV, OP_MODSQRT, OP_MODQR, OP_MODMLI };

// c = op(a, b) for n elements; k: the count of modnsqr, the multiplier of modmli.  modqr writes its answer (0 / 1) into limb 0 and zeroes
// the other limbs.
template <class P, bool FAST>
void run_op(int op, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t n, int k) {
    using F = ma::Field<P, FAST>;
    constexpr int N = P::N;
    for (size_t j = 0; j < n; j++) {
        uint64_t x[N], y[N], z[N];
        for (int i = 0; i < N; i++) { x[i] = a[(size_t)i * n + j]; y[i] = b ? b[(size_t)i * n + j] : 0; z[i] = 0; }
        switch (op) {
            case OP_MODMUL: F::modmul(x, y, z); break;
            case OP_MODSQR: F::modsqr(x, z); break;
            case OP_NRES: F::nres(x, z); break;
            case OP_REDC: F::redc(x, z); break;
            case OP_MODNSQR: F::modnsqr(x, k); F::modcpy(x, z); break;
            case OP_MODINV: F::modinv(x, nullptr, z); break;
            case OP_MODSQRT: F::modsqrt(x, nullptr, z); break;
            case OP_MODQR: z[0] = (uint64_t)F::modqr(nullptr, x); break;
            case OP_MODMLI: F::modmli(x, k, z); break;
            default: break;
        }
        for (int i = 0; i < N; i++) c[(size_t)i * n + j] = z[i];
    }
}

template <bool FAST>
int dispatch(const char* prime, int op, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t n, int k) {
#define FFH_X(T) if (strcmp(prime, #T) == 0) { run_op<ma::P_##T, FAST>(op, a, b, c, n, k); return 0; }
    FFH_PRIMES(FFH_X)
#undef FFH_X
    return -1;                                  // not a prime of this unit
}

template <class P>
void facts(int* out) {
    using F = ma::Field<P, true>;
    const int v[] = {F::FAST, F::CHAINED, F::SPLIT4, F::HALF, F::HALF_OV, F::MHALF, F::MHALF_TRI, F::SPLIT_SPARSE, F::FOLD52,
                     P::SPLIT, P::N, P::RADIX, P::MONTGOMERY, ma::Field<P, false>::FAST};
    for (size_t i = 0; i < sizeof v / sizeof v[0]; i++) out[i] = v[i];
}

}  // namespace

// one entry point per (policy, operation): 0 = done, -1 = the prime is not in this unit
#define FFH_BIN(NAME, OP)                                                                                                             \
    extern "C" int ffh_exact_##NAME(const char* prime, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t n) {                 \
        return dispatch<false>(prime, OP, a, b, c, n, 0);                                                                             \
    }                                                                                                                                 \
    extern "C" int ffh_fast_##NAME(const char* prime, const uint64_t* a, const uint64_t* b, uint64_t* c, size_t n) {                  \
        return dispatch<true>(prime, OP, a, b, c, n, 0);                                                                              \
    }
#define FFH_UN(NAME, OP)                                                                                                              \
    extern "C" int ffh_exact_##NAME(const char* prime, const uint64_t* a, uint64_t* c, size_t n) {                                    \
        return dispatch<false>(prime, OP, a, nullptr, c, n, 0);                                                                       \
    }                                                                                                                                 \
    extern "C" int ffh_fast_##NAME(const char* prime, const uint64_t* a, uint64_t* c, size_t n) {                                     \
        return dispatch<true>(prime, OP, a, nullptr, c, n, 0);                                                                        \
    }
#define FFH_UNK(NAME, OP)                                                                                                             \
    extern "C" int ffh_exact_##NAME(const char* prime, const uint64_t* a, int k, uint64_t* c, size_t n) {                             \
        return dispatch<false>(prime, OP, a, nullptr, c, n, k);                                                                       \
    }                                                                                                                                 \
    extern "C" int ffh_fast_##NAME(const char* prime, const uint64_t* a, int k, uint64_t* c, size_t n) {                              \
        return dispatch<true>(prime, OP, a, nullptr, c, n, k);                                                                        \
    }
FFH_BIN(modmul, OP_MODMUL)
FFH_UN(modsqr, OP_MODSQR)
FFH_UN(nres, OP_NRES)
FFH_UN(redc, OP_REDC)
FFH_UNK(modnsqr, OP_MODNSQR)
FFH_UN(modinv, OP_MODINV)
FFH_UN(modsqrt, OP_MODSQRT)
FFH_UN(modqr, OP_MODQR)
FFH_UNK(modmli, OP_MODMLI)

// compile-time facts of Field<P, true>, in the order of FFH_FACTS in tests/test_fast_products_host.py:
// FAST, CHAINED, SPLIT4, HALF, HALF_OV, MHALF, MHALF_TRI, SPLIT_SPARSE, FOLD52, P::SPLIT, N, RADIX, MONTGOMERY, Field<P, false>::FAST
extern "C" int ffh_facts(const char* prime, int* out) {
#define FFH_X(T) if (strcmp(prime, #T) == 0) { facts<ma::P_##T>(out); return 0; }
    FFH_PRIMES(FFH_X)
#undef FFH_X
    return -1;
}
