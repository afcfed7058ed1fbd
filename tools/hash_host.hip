// tools/hash_host.hip -- the per-lane hash functions of csrc/hash.h compiled for the HOST: the very record functions the kernels of
// capi_hash.hip wrap (ma::hash::sha2_record, keccak_record over the part cursor), so that tests/test_hash_host.py can run every padding
// edge and every split of a message into parts against hashlib before any GPU is involved.  Test tooling, not product code.
//   hipcc -O1 -std=c++17 -w --offload-host-only -I modarith_amd/csrc tools/hash_host.hip -o hash_host
// A stand-alone program: it reads one request per line on standard input --
//   <algorithm> <olen> <part> [<part> ...]
// algorithm: sha256 sha384 sha512 sha3-224 sha3-256 sha3-384 sha3-512 shake128 shake256; olen: output bytes (SHAKE; ignored otherwise);
// a part: hex bytes, "-" for an empty part, and "<hex>:<L>" to give the part a lens[] entry L (the cursor clamps it to the part's length)
// -- and answers each with one line: the digest in hex.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "hash.h"

using namespace ma::hash;

static int hexval(int c) { return c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : c >= 'A' && c <= 'F' ? c - 'A' + 10 : -1; }

int main() {
    static char line[1 << 16];
    while (fgets(line, sizeof line, stdin)) {
        char* save = nullptr;
        const char* algo = strtok_r(line, " \n", &save);
        const char* ol = strtok_r(nullptr, " \n", &save);
        if (!algo || !ol) { printf("error parse\n"); return 2; }
        size_t olen = (size_t)strtoul(ol, nullptr, 10);
        // every part in an exact-size heap block of its own: a read past a part's end is a heap overflow the sanitizer build reports
        std::vector<std::vector<unsigned char>> bytes;
        std::vector<uint32_t> lens(MAX_PARTS, 0);
        bool has_len[MAX_PARTS] = {};
        for (char* tok; (tok = strtok_r(nullptr, " \n", &save));) {
            if ((int)bytes.size() == MAX_PARTS) { printf("error parts\n"); return 2; }
            const int k = (int)bytes.size();
            if (char* colon = strchr(tok, ':')) { *colon = 0; lens[k] = (uint32_t)strtoul(colon + 1, nullptr, 10); has_len[k] = true; }
            std::vector<unsigned char> b;
            if (strcmp(tok, "-") != 0) {
                const size_t L = strlen(tok);
                if (L % 2) { printf("error hex\n"); return 2; }
                for (size_t i = 0; i < L; i += 2) {
                    const int hi = hexval(tok[i]), lo = hexval(tok[i + 1]);
                    if (hi < 0 || lo < 0) { printf("error hex\n"); return 2; }
                    b.push_back((unsigned char)(hi * 16 + lo));
                }
            }
            bytes.push_back(b);
        }
        if (bytes.empty()) { printf("error parts\n"); return 2; }
        Parts P = {};
        P.n = (int)bytes.size();
        for (int k = 0; k < P.n; k++) {
            P.p[k].ptr = bytes[k].data();
            P.p[k].stride = 0;
            P.p[k].len = (uint32_t)bytes[k].size();
            P.p[k].lens = has_len[k] ? &lens[k] : nullptr;
        }
        size_t dl = 0;
        if (!strcmp(algo, "sha256")) dl = 32;
        else if (!strcmp(algo, "sha384")) dl = 48;
        else if (!strcmp(algo, "sha512")) dl = 64;
        else if (!strcmp(algo, "sha3-224")) dl = 28;
        else if (!strcmp(algo, "sha3-256")) dl = 32;
        else if (!strcmp(algo, "sha3-384")) dl = 48;
        else if (!strcmp(algo, "sha3-512")) dl = 64;
        else if (!strcmp(algo, "shake128") || !strcmp(algo, "shake256")) dl = olen;
        if (dl == 0) { printf("error algorithm\n"); return 2; }
        std::vector<unsigned char> out(dl);                 // exact size: a write past the digest is reported too
        unsigned char* o = out.data();
        if (!strcmp(algo, "sha256")) sha2_record<Sha256, 32>(P, 0, o);
        else if (!strcmp(algo, "sha384")) sha2_record<Sha512, 48>(P, 0, o);
        else if (!strcmp(algo, "sha512")) sha2_record<Sha512, 64>(P, 0, o);
        else if (!strcmp(algo, "sha3-224")) keccak_record<144, 0x06>(P, 0, o, dl);
        else if (!strcmp(algo, "sha3-256")) keccak_record<136, 0x06>(P, 0, o, dl);
        else if (!strcmp(algo, "sha3-384")) keccak_record<104, 0x06>(P, 0, o, dl);
        else if (!strcmp(algo, "sha3-512")) keccak_record<72, 0x06>(P, 0, o, dl);
        else if (!strcmp(algo, "shake128")) keccak_record<168, 0x1f>(P, 0, o, dl);
        else keccak_record<136, 0x1f>(P, 0, o, dl);
        for (size_t i = 0; i < dl; i++) printf("%02x", o[i]);
        printf("\n");
    }
    return 0;
}
