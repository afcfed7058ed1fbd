/* examples/hash_batch.c -- the batched hashes of include/modarith_amd_hash.h from plain C.
 *
 *   gcc -O2 examples/hash_batch.c -I include -L modarith_amd -l:libmodarith_amd.so -Wl,-rpath,$PWD/modarith_amd -o hash_batch
 *   ./hash_batch [n]
 *
 * 1. HASH256 of one shared record "abc" (stride 0) in every lane: the FIPS 180-4 value.
 * 2. The hash of ED448_VERIFY (ed448.c:289-298) for n records: SHAKE256(dom4 || R || A || M) to 114 bytes, the four SHA3_process loops
 *    as four parts -- dom4 shared by the batch, R the first 57 bytes of each 114-byte signature row (stride 114), A 57-byte rows, M
 *    rows of 120 bytes of which record j uses j % 121.  The digests go to rows of 128 bytes.  Every digest is printed as
 *    "<j> <hex>"; tests/test_gpu_hash.py rebuilds the inputs (the generator below) and compares with hashlib.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "modarith_amd_hash.h"

#define CHECK(call)                                                                                    \
    do {                                                                                               \
        int rc_ = (call);                                                                              \
        if (rc_ != 0) {                                                                                \
            fprintf(stderr, "%s failed (%d): %s\n", #call, rc_, modarith_amd_last_error());           \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

static uint32_t lcg_state;
static unsigned char lcg_byte(void) {
    lcg_state = lcg_state * 1103515245u + 12345u;
    return (unsigned char)(lcg_state >> 16);
}
static void fill(unsigned char *p, size_t bytes, uint32_t seed) {
    lcg_state = seed;
    for (size_t i = 0; i < bytes; i++) p[i] = lcg_byte();
}

int main(int argc, char **argv) {
    const size_t n = argc > 1 ? (size_t)strtoul(argv[1], NULL, 10) : 200;
    enum { B = 57, LMAX = 120, OLEN = 114, DSTRIDE = 128 };
    static const unsigned char dom4[10] = {'S', 'i', 'g', 'E', 'd', '4', '4', '8', 0, 0};
    if (n == 0) return 0;

    unsigned char *sig = malloc(n * 2 * B), *pub = malloc(n * B), *msg = malloc(n * LMAX), *out = malloc(n * DSTRIDE);
    uint32_t *mlen = malloc(n * sizeof(uint32_t));
    if (!sig || !pub || !msg || !out || !mlen) return 1;
    fill(sig, n * 2 * B, 1);
    fill(pub, n * B, 2);
    fill(msg, n * LMAX, 3);
    for (size_t j = 0; j < n; j++) mlen[j] = (uint32_t)(j % (LMAX + 1));

    void *d_dom, *d_sig, *d_pub, *d_msg, *d_len, *d_out;
    CHECK(modarith_amd_malloc(&d_dom, sizeof dom4));
    CHECK(modarith_amd_malloc(&d_sig, n * 2 * B));
    CHECK(modarith_amd_malloc(&d_pub, n * B));
    CHECK(modarith_amd_malloc(&d_msg, n * LMAX));
    CHECK(modarith_amd_malloc(&d_len, n * sizeof(uint32_t)));
    CHECK(modarith_amd_malloc(&d_out, n * DSTRIDE));
    CHECK(modarith_amd_memcpy_h2d(d_dom, dom4, sizeof dom4, NULL));
    CHECK(modarith_amd_memcpy_h2d(d_sig, sig, n * 2 * B, NULL));
    CHECK(modarith_amd_memcpy_h2d(d_pub, pub, n * B, NULL));
    CHECK(modarith_amd_memcpy_h2d(d_msg, msg, n * LMAX, NULL));
    CHECK(modarith_amd_memcpy_h2d(d_len, mlen, n * sizeof(uint32_t), NULL));

    /* 1. one shared record in every lane */
    {
        static const unsigned char want[32] = {0xba, 0x78, 0x16, 0xbf, 0x8f, 0x01, 0xcf, 0xea, 0x41, 0x41, 0x40, 0xde, 0x5d, 0xae, 0x22, 0x23,
                                               0xb0, 0x03, 0x61, 0xa3, 0x96, 0x17, 0x7a, 0x9c, 0xb4, 0x10, 0xff, 0x61, 0xf2, 0x00, 0x15, 0xad};
        ma_hash_part abc = {d_dom, 0, NULL, 3};
        CHECK(modarith_amd_memcpy_h2d(d_dom, "abc", 3, NULL));
        CHECK(HASH256_batch(&abc, 1, d_out, DSTRIDE, n, NULL));
        CHECK(modarith_amd_memcpy_d2h(out, d_out, n * DSTRIDE, NULL));
        CHECK(modarith_amd_sync(NULL));
        for (size_t j = 0; j < n; j++)
            if (memcmp(out + j * DSTRIDE, want, 32) != 0) { fprintf(stderr, "HASH256(\"abc\") differs in lane %zu\n", j); return 1; }
        printf("HASH256(\"abc\") in %zu lanes: the FIPS 180-4 value (%s)\n", n, modarith_amd_last_launch());
        CHECK(modarith_amd_memcpy_h2d(d_dom, dom4, sizeof dom4, NULL));
    }

    /* 2. SHAKE256(dom4 || R || A || M), 114 bytes out: ed448.c:289-298 for the whole batch */
    {
        ma_hash_part parts[4] = {
            {d_dom, 0, NULL, sizeof dom4},          /* shared by the batch */
            {d_sig, 2 * B, NULL, B},                /* R: the first half of each signature row */
            {d_pub, B, NULL, B},
            {d_msg, LMAX, (const uint32_t *)d_len, LMAX},
        };
        CHECK(SHA3_shake_batch(32, parts, 4, d_out, DSTRIDE, OLEN, n, NULL));
        CHECK(modarith_amd_memcpy_d2h(out, d_out, n * DSTRIDE, NULL));
        CHECK(modarith_amd_sync(NULL));
        for (size_t j = 0; j < n; j++) {
            printf("%zu ", j);
            for (int i = 0; i < OLEN; i++) printf("%02x", out[j * DSTRIDE + i]);
            printf("\n");
        }
        printf("%zu records hashed (%s)\n", n, modarith_amd_last_launch());
    }
    modarith_amd_free(d_dom); modarith_amd_free(d_sig); modarith_amd_free(d_pub); modarith_amd_free(d_msg); modarith_amd_free(d_len); modarith_amd_free(d_out);
    free(sig); free(pub); free(msg); free(out); free(mlen);
    return 0;
}
