// modarith_amd/csrc/capi_hash.hip -- the entry points of include/modarith_amd_hash.h: hash.c's SHA-2, SHA-3 and SHAKE as batches, one
// record per lane over the per-lane functions of hash.h.  The parts of the record travel by value in the kernel arguments; no memory
// is taken and nothing synchronises, so every call works on a stream under capture.
#include "../../include/modarith_amd_hash.h"
#include "capi_common.h"
#include "hash.h"

namespace ma {
namespace hash {

constexpr int HASH_BLOCK = 256;

static_assert(sizeof(Part) == sizeof(ma_hash_part) && offsetof(Part, ptr) == offsetof(ma_hash_part, ptr) && offsetof(Part, stride) == offsetof(ma_hash_part, stride) &&
              offsetof(Part, lens) == offsetof(ma_hash_part, lens) && offsetof(Part, len) == offsetof(ma_hash_part, len), "Part is ma_hash_part");

// one record per lane, grid-stride; lanes of a wave that need fewer blocks wait for the longest
template <class A, int DIGEST>
__global__ __launch_bounds__(HASH_BLOCK) void k_sha2(Parts P, unsigned char* digest, size_t dstride, size_t n) {
    for (size_t j = (size_t)blockIdx.x * HASH_BLOCK + threadIdx.x; j < n; j += (size_t)gridDim.x * HASH_BLOCK)
        sha2_record<A, DIGEST>(P, j, digest + j * dstride);
}
template <int RATE, int DOM>
__global__ __launch_bounds__(HASH_BLOCK) void k_keccak(Parts P, unsigned char* digest, size_t dstride, size_t olen, size_t n) {
    for (size_t j = (size_t)blockIdx.x * HASH_BLOCK + threadIdx.x; j < n; j += (size_t)gridDim.x * HASH_BLOCK)
        keccak_record<RATE, DOM>(P, j, digest + j * dstride, olen);
}

}  // namespace hash
}  // namespace ma

namespace {
using namespace ma::hash;

// the host preamble of every entry point: 0 and *go = false for an empty batch, a refusal (nothing launched) or *go = true with P filled
int prepare(const char* what, const ma_hash_part* parts, int nparts, const void* digest, size_t dstride, size_t dlen, size_t n, Parts* P, bool* go) {
    *go = false;
    if (n == 0) return 0;
    const std::string w(what);
    if (nparts < 1 || nparts > MAX_PARTS) return ma::reject(w + ": need 1 <= nparts <= 8");
    if (!parts || !digest) return ma::reject(w + ": parts and digest must not be null");
    if (dlen == 0) return ma::reject(w + ": olen must not be 0");
    if (dstride < dlen) return ma::reject(w + ": dstride is below the digest length");
    *P = Parts{};
    P->n = nparts;
    for (int k = 0; k < nparts; k++) {
        if (!parts[k].ptr && parts[k].len != 0) return ma::reject(w + ": a part with len > 0 has a null ptr");
        P->p[k].ptr = static_cast<const unsigned char*>(parts[k].ptr);
        P->p[k].stride = parts[k].stride;
        P->p[k].lens = parts[k].lens;
        P->p[k].len = parts[k].len;
    }
    *go = true;
    return 0;
}

template <class A, int DIGEST>
int sha2_batch(const char* what, const ma_hash_part* parts, int nparts, void* digest, size_t dstride, size_t n, void* stream) {
    Parts P;
    bool go;
    if (int rc = prepare(what, parts, nparts, digest, dstride, DIGEST, n, &P, &go); rc || !go) return rc;
    k_sha2<A, DIGEST><<<ma::grid_for(n, HASH_BLOCK), HASH_BLOCK, 0, (hipStream_t)stream>>>(P, static_cast<unsigned char*>(digest), dstride, n);
    return ma::check_launch(what);
}
template <int RATE, int DOM>
int keccak_batch(const char* what, const Parts& P, void* digest, size_t dstride, size_t olen, size_t n, void* stream) {
    k_keccak<RATE, DOM><<<ma::grid_for(n, HASH_BLOCK), HASH_BLOCK, 0, (hipStream_t)stream>>>(P, static_cast<unsigned char*>(digest), dstride, olen, n);
    return ma::check_launch(what);
}
}  // namespace

extern "C" {

int HASH256_batch(const ma_hash_part* parts, int nparts, void* digest, size_t dstride, size_t n, void* stream) {
    return sha2_batch<Sha256, 32>("hash sha256", parts, nparts, digest, dstride, n, stream);
}
int HASH384_batch(const ma_hash_part* parts, int nparts, void* digest, size_t dstride, size_t n, void* stream) {
    return sha2_batch<Sha512, 48>("hash sha384", parts, nparts, digest, dstride, n, stream);
}
int HASH512_batch(const ma_hash_part* parts, int nparts, void* digest, size_t dstride, size_t n, void* stream) {
    return sha2_batch<Sha512, 64>("hash sha512", parts, nparts, digest, dstride, n, stream);
}

int SHA3_hash_batch(int t, const ma_hash_part* parts, int nparts, void* digest, size_t dstride, size_t n, void* stream) {
    if (n == 0) return 0;
    if (t != 28 && t != 32 && t != 48 && t != 64) return ma::reject("SHA3_hash_batch: t must be 28, 32, 48 or 64");
    Parts P;
    bool go;
    if (int rc = prepare("SHA3_hash_batch", parts, nparts, digest, dstride, (size_t)t, n, &P, &go); rc || !go) return rc;
    switch (t) {
    case 28: return keccak_batch<144, 0x06>("hash sha3-224", P, digest, dstride, 28, n, stream);
    case 32: return keccak_batch<136, 0x06>("hash sha3-256", P, digest, dstride, 32, n, stream);
    case 48: return keccak_batch<104, 0x06>("hash sha3-384", P, digest, dstride, 48, n, stream);
    default: return keccak_batch<72, 0x06>("hash sha3-512", P, digest, dstride, 64, n, stream);
    }
}

int SHA3_shake_batch(int t, const ma_hash_part* parts, int nparts, void* digest, size_t dstride, size_t olen, size_t n, void* stream) {
    if (n == 0) return 0;
    if (t != 16 && t != 32) return ma::reject("SHA3_shake_batch: t must be 16 (SHAKE128) or 32 (SHAKE256)");
    Parts P;
    bool go;
    if (int rc = prepare("SHA3_shake_batch", parts, nparts, digest, dstride, olen, n, &P, &go); rc || !go) return rc;
    if (t == 16) return keccak_batch<168, 0x1f>("hash shake128", P, digest, dstride, olen, n, stream);
    return keccak_batch<136, 0x1f>("hash shake256", P, digest, dstride, olen, n, stream);
}

}  // extern "C"
