/* include/modarith_amd_hash.h -- the reference's hash.c as batches on the device: SHA-256, SHA-384, SHA-512, SHA-3 and SHAKE over
 * byte records, one record per lane.  The entry points keep hash.h's names with _batch added.
 *
 * A record is the concatenation of up to eight PARTS, each an array of byte rows of its own (or one row shared by the whole batch).
 * The loops of SHA3_process calls in ed448.c:219-225, 236-244, 289-298 (dom4, then R, then Q, then M) become the `parts` array; no
 * concatenation pass is needed.
 *
 *   digest j = H(part0[j] || part1[j] || ...), written to (char *)digest + j * dstride
 *
 * Parts:         1 <= nparts <= 8.  `parts` is a HOST array; it is copied by value into the kernel arguments, so it may be a
 *                temporary.  The pointers inside it are DEVICE pointers.  Rows may start at any byte address (rows of 57 bytes are
 *                the normal case).  A part with len == 0 may have a null ptr.
 * Lengths:       record j takes min(lens[j], len) bytes of a part; lens == NULL: len bytes.  The clamp is deliberate: a bad length
 *                array cannot take a lane outside the row the caller described.  The total of a record must stay below 2^32 bytes.
 * No allocation: the calls take no memory, no workspace and no host synchronisation: they work on a stream under capture.
 * Empty batch:   n == 0 returns 0 and launches nothing (checked first, as everywhere in the library).
 * Refusals:      nparts out of range, an unknown t, olen == 0, dstride below the digest length, null pointers (parts, digest, the
 *                ptr of a part with len > 0): hipErrorInvalidValue, the text in modarith_amd_last_error(), nothing launched.
 * Aliasing:      the digest array must NOT overlap any part (a lane writes its digest while its neighbours still read).
 * Launch shape:  one record per lane, the grid sized as for the element-wise field kernels.  Lanes of a wave may need different block
 *                counts; the wave runs to its longest.  modarith_amd_last_launch() names the launch: "hash sha256", "hash sha384",
 *                "hash sha512", "hash sha3-224" ... "hash sha3-512", "hash shake128", "hash shake256".
 * Timing:        the time of a launch depends on the LENGTHS only.  The kernels index no table by message data and take no branch on
 *                message data: the round constants are indexed by the round counter, the part cursor branches on lengths and
 *                offsets, and the state and schedule live in registers under compile-time indices (csrc/hash.h).
 * Status:        return values, errors, streams and threading as in modarith_amd.h (0 on success, a hipError_t value otherwise).
 *                MODARITH_AMD_ABI is unchanged by this header: nothing existing changed.
 *
 * Out of scope: the streaming init / process / hash API and the continuing_* forms (a batch has the whole record; a caller that
 * streams keeps hash.c); HMAC (two calls of the above plus an XOR pass -- and the reference's SHA-3 branch of it does not terminate,
 * hash.c:599-600); scalar host-pointer forms.
 */
#ifndef MODARITH_AMD_HASH_H
#define MODARITH_AMD_HASH_H

#include <stddef.h>
#include <stdint.h>

#include "modarith_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    const void *ptr;      /* device; record j starts at (const char *)ptr + j * stride; any alignment */
    size_t stride;        /* bytes between records; 0: one record shared by the whole batch (dom4, a prefix) */
    const uint32_t *lens; /* device, n entries, or NULL.  Record j contributes min(lens[j], len) bytes; NULL: len bytes */
    uint32_t len;         /* the part's length, or the upper bound of lens[j] (what the caller allocated per row) */
} ma_hash_part;

/* SHA-2 (FIPS 180-4): digests of 32 / 48 / 64 bytes */
int HASH256_batch(const ma_hash_part *parts, int nparts, void *digest, size_t dstride, size_t n, void *stream);
int HASH384_batch(const ma_hash_part *parts, int nparts, void *digest, size_t dstride, size_t n, void *stream);
int HASH512_batch(const ma_hash_part *parts, int nparts, void *digest, size_t dstride, size_t n, void *stream);
/* SHA-3 (FIPS 202): t = digest bytes, 28, 32, 48 or 64 (hash.h SHA3_HASH224 ... SHA3_HASH512) */
int SHA3_hash_batch(int t, const ma_hash_part *parts, int nparts, void *digest, size_t dstride, size_t n, void *stream);
/* SHAKE: t = 16 (SHAKE128) or 32 (SHAKE256), as SHA3_init takes them; olen output bytes per record */
int SHA3_shake_batch(int t, const ma_hash_part *parts, int nparts, void *digest, size_t dstride, size_t olen, size_t n, void *stream);

#ifdef __cplusplus
}
#endif
#endif
