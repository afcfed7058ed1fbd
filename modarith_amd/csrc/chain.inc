// modarith_amd/csrc/chain.inc -- what every fused chain (modarith_amd/fuse.py) has in common: the kernels around the chain and the bodies
// of its C entry points, at either word length (MA_WL: kernels.h / kernels32.h).  The generated unit includes this file ONCE, inside its
// own anonymous namespace, after the pieces that depend on the chain:
//   #define CHAIN_SYMBOL "chain_<name>_<TAG>"                             what the entry points are called, without _batch / _aos
//   using namespace ma | ma32;  using P = ...;
//   constexpr int NIN, NOUT, NSEL;  constexpr bool HEAVY;                 arrays in and out, selectors; a chain at one element per lane
//   constexpr int EPT_CAP, CBLOCK;                                        word length 32 only: widest width of the build, workgroup size
//   #define CHAIN_AOS_IMAGES k                                            word length 64 only: LDS images of the element-major kernel
//   #define CHAIN_KERNEL_ATTR __attribute__((...))                        optional: an occupancy hint on k_chain
//   #define CHAIN_NSHARED k                                               optional: batch-wide element operands (ch.shared()), 1 .. 8
//   #define CHAIN_NPRED k                                                 optional: int32 results (ch.output() of a Pred), one entry per element
//   #define CHAIN_NBIN k, CHAIN_NBOUT k                                   optional: byte-record inputs (ch.input_bytes()) and outputs (ch.output_bytes())
//   #define CHAIN_BYTES_STAGED 0 | 1                                      with either of them: the default way to the bytes (section "byte records")
//   #define CHAIN_BIN_LE m, CHAIN_BOUT_LE m                               optional: bit j set = byte array j of that side is little-endian
//   #define CHAIN_BIN_SIGN m, CHAIN_BOUT_SIGN m                           optional: bit j set = the top bit of array j's records is a sign:
//                                                                         io.imp(j, v, s, sign) takes it out, io.exp(k, v, sign) puts it in
//   template <class F> MA_DEV void body(v0, ..., s0, ...);                the chain on one element's registers
//   template <int EPT, class IO> MA_DEV void chain_step(IO io);           EPT elements of a lane: io.load(i, v_i) per input, io.shared(j)
//                                                                         per shared operand, io.sel(k, s_k) per selector, the vote,
//                                                                         body, io.store(k, v_o) per output, io.pred(k, s_j) per int output;
//                                                                         io.imp(j, v, s) per byte input, io.exp(k, v) per byte output
// and then defines its `extern "C"` symbols over chain_batch() and chain_aos().  Editing this file rebuilds every chain (generate.key_of
// hashes all of csrc/).
//
// THE ARRAYS OF A CALL, in this order (the one statement of it on this side; fuse.Chain.layout() is the same list for the Python side):
//   in[]   NIN element batches | CHAIN_NBIN arrays of n byte records | CHAIN_NSHARED HOST pointers, Nlimbs words each | NSEL int32 device
//          arrays, one entry per element
//   out[]  NOUT element batches | CHAIN_NBOUT arrays of n byte records | CHAIN_NPRED int32 device arrays of n entries
// (_aos takes the same with element-major arrays for the batches; it has no byte records.)  The constants IN_* / OUT_* below are the first
// slot of each kind: every entry body goes through them.
#if MA_WL == 32
using ma::check_launch;         // (the host helpers of capi_common.h; the 64-bit unit has all of namespace ma in scope)
using ma::grid_for;
using ma::set_error;
#endif
#if MA_WL == 64
constexpr int EPT_CAP = HEAVY ? 1 : 2;   // widest access of a call in elements per lane (2 = 16 bytes, 1 = 8)
constexpr int EPT_BUILT = 2;             // (both widths are compiled for every 64-bit chain, a HEAVY one included: as the units always were)
constexpr int CBLOCK = BLOCK;            // workgroup size
#else
constexpr int EPT_BUILT = EPT_CAP;       // wider kernels are not instantiated
#endif
static_assert(EPT_CAP == 1 || EPT_CAP == 2 || (EPT_CAP == 4 && MA_WL == 32), "one or two elements per lane, four of 32-bit limbs");
static_assert(!HEAVY || EPT_CAP == 1, "the long chains run one element per lane");
#ifndef CHAIN_KERNEL_ATTR
#define CHAIN_KERNEL_ATTR
#endif
// Shared operands (CHAIN_NSHARED > 0): one field element each, the same for every element of the batch.  They travel BY VALUE in the
// kernel arguments, as the Elem<P> of k_mul_shared (kernels.h) does: wave-uniform, so the compiler may keep them and what it derives
// from them alone in SGPRs.  The entry points read them from HOST memory, once, before they return (Nlimbs words each, as modmuls reads
// b0_host): no device buffer, no copy to order on the stream, and a call under stream capture bakes the value in.  Without them Args and
// the kernels' signatures are what they were.
#ifndef CHAIN_NSHARED
#define CHAIN_NSHARED 0
#endif
static_assert(CHAIN_NSHARED >= 0 && CHAIN_NSHARED <= 8, "a chain takes at most 8 shared operands");
// Int results (CHAIN_NPRED > 0): the ints a chain computes (modis0 / modis1 / modsign / modcmp / modqr and the 0/1 expressions on them) that
// it declares outputs.  One int32 device array of n contiguous entries each, indexed BY ELEMENT as the selectors are, whatever the layout
// of the element batches.  A chain may have nothing else to return (NOUT == 0).  An int result may be the array of a selector input: a
// lane reads its entries (io.sel) before it stores them (io.pred), and no other lane touches them.  Args::pred is a zero-length array
// without int results: it adds nothing to the kernel arguments.
#ifndef CHAIN_NPRED
#define CHAIN_NPRED 0
#endif
// Byte records (CHAIN_NBIN + CHAIN_NBOUT > 0): arrays of n big-endian records of P::NBYTES bytes, rec[j * NBYTES + i], what modimp reads and
// modexp writes (little-endian, or with the top bit a sign, where the unit says so per array: below); record index = element index.
// The kernels of such a chain are in the section "byte records" below; with both 0 none of them is compiled, BArgs stays on the host
// and k_chain is launched as it always was.
#ifndef CHAIN_NBIN
#define CHAIN_NBIN 0
#endif
#ifndef CHAIN_NBOUT
#define CHAIN_NBOUT 0
#endif
static_assert(CHAIN_NBIN >= 0 && CHAIN_NBOUT >= 0 && NIN + CHAIN_NBIN > 0, "a chain reads at least one array");
static_assert(CHAIN_NPRED >= 0 && NOUT + CHAIN_NPRED + CHAIN_NBOUT > 0, "a chain returns at least one array");
#define CHAIN_BYTES (CHAIN_NBIN + CHAIN_NBOUT > 0)
// the first slot of each kind of array in in[] and out[] (the order: the head of this file); the element batches start at 0
constexpr int IN_BYTES = NIN, IN_SHARED = IN_BYTES + CHAIN_NBIN, IN_SEL = IN_SHARED + CHAIN_NSHARED;
constexpr int OUT_BYTES = NOUT, OUT_PRED = OUT_BYTES + CHAIN_NBOUT;
#if CHAIN_NSHARED > 0
struct Args { const spint* in[NIN]; spint* out[NOUT > 0 ? NOUT : 1]; const int* sel[NSEL > 0 ? NSEL : 1]; int* pred[CHAIN_NPRED]; Elem<P> sh[CHAIN_NSHARED]; };
MA_DEV const spint* shared_of(const Args& A, int j) { return A.sh[j].l; }
#else
struct Args { const spint* in[NIN]; spint* out[NOUT > 0 ? NOUT : 1]; const int* sel[NSEL > 0 ? NSEL : 1]; int* pred[CHAIN_NPRED]; };
MA_DEV const spint* shared_of(const Args&, int) { return nullptr; }
#endif
struct BArgs { const unsigned char* bin[CHAIN_NBIN > 0 ? CHAIN_NBIN : 1]; unsigned char* bout[CHAIN_NBOUT > 0 ? CHAIN_NBOUT : 1]; };    // (a kernel argument of the byte-record kernels only)
constexpr int NB = P::NBYTES;

// ---- limb-interleaved batches: load_soa / store_soa at lane t, EPT consecutive elements.  (The int side -- shared, sel, pred -- is
// spelt out in each of the three lane I/Os of this file: written once over "the lane's first element" and "is entry E live" it
// compiled to other code in the kernels of chains with selectors or int results, profiles/chain_one_entry.json)
template <int EPT> struct SoaIO {
    const Args& A; Ld L; size_t t;
    MA_DEV void load(int i, spint (*v)[P::N]) const { load_soa<P, EPT>(A.in[i], L, t, v); }
    MA_DEV const spint* shared(int j) const { return shared_of(A, j); }
    MA_DEV void sel(int k, int* s) const { static_for<0, EPT>([&](auto E) { s[E] = A.sel[k][(size_t)EPT * t + E]; }); }
    MA_DEV void store(int k, spint (*v)[P::N]) const { store_soa<P, EPT>(A.out[k], L, t, v); }
    MA_DEV void pred(int k, const int* s) const { static_for<0, EPT>([&](auto E) { A.pred[k][(size_t)EPT * t + E] = s[E]; }); }   // (one 4-byte store per element: no alignment asked of the array)
};
template <int EPT>
__global__ __launch_bounds__(CBLOCK) CHAIN_KERNEL_ATTR void k_chain(Args A, size_t nthreads, Ld L) {
    for (size_t t = (size_t)blockIdx.x * CBLOCK + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * CBLOCK) chain_step<EPT>(SoaIO<EPT>{A, L, t});
}

#if CHAIN_BYTES
// ---- byte records: modimp at the head of the chain and modexp at its tail, inside the kernel.  io.imp(j, v, s) leaves in v the CANONICAL
// limbs of the integer that record j spells (limbs_from_words, then modfsb: inside the limb contract, so an imported value joins the
// vote as any input does) and in s modimp's return value; the chain's body starts with F::nres of it, under the policy the wave voted
// for.  The body ends with F::redc of what io.exp(k, v) then turns into bytes (words_from_limbs and the store).  Two ways to the bytes:
//   direct   every lane reads and writes its own records in HBM, as k_imp / k_exp do (load_be_record / store_be_record of kernels.h).
//            Always legal: the remainder launch and any call whose record arrays are not 16-byte aligned take it;
//   staged   a workgroup moves the records of the CBLOCK * EPT consecutive elements it is about to process -- one linear stretch,
//            16-byte aligned since 64 * NBYTES is a multiple of 16 -- with 16-byte-per-lane coalesced non-temporal accesses into an
//            LDS image, and after a barrier every lane takes its own records out of the image (the same load_be_record, on LDS);
//            output is the mirror image.  A record's pitch in the image is an odd number of 8-byte words where NBYTES is a
//            multiple of 8 and of 4-byte words otherwise: a wave's accesses conflict two ways at the most (the idea of SP = N | 1
//            below).  One image per byte input while they fit 64 KB together, else one image that the arrays take in turn between
//            barriers (the CHAIN_AOS_IMAGES rule); the outputs go through the first image.
// Which of the two a call on aligned arrays takes is BYTES_STAGED below (measured: tools/chain_bytes_rate.py, docs/fused_chains.md);
// the environment variable MA_CHAIN_BYTES=staged|direct, read at every call, overrides it (tests, the rate tool).
// Byte order and sign are properties of each byte array, fixed when the unit is emitted: CHAIN_BIN_LE / CHAIN_BOUT_LE name the arrays
// whose records are least significant byte first (load_le_record / store_le_record: no bswap, word order kept); CHAIN_BIN_SIGN /
// CHAIN_BOUT_SIGN those whose most significant bit -- bit 8 NBYTES - 1 of the integer, the top bit of the record's last byte where it is
// little-endian and of its first where it is big-endian -- is not part of the value (RFC 8032's x_0, the bit rfc7748.c:172 masks).  The
// bit is taken out of, or OR-ed into, the words in registers, between the load and limbs_from_words and between words_from_limbs and
// the store.  The array index reaches these helpers as a literal of chain_step: the tests fold.  A unit that defines none of the four
// compiles the text it always did.
constexpr int NW = Field<P>::NW;
constexpr int TOPW = (8 * NB - 1) / 64, TOPB = (8 * NB - 1) % 64;     // where a record's most significant bit lies in its words
MA_DEV void load_record(int j, const unsigned char* bytes, size_t t, word_t* w) {
#ifdef CHAIN_BIN_LE
    if ((CHAIN_BIN_LE >> j) & 1) { load_le_record<P>(bytes, t, w); return; }
#endif
    load_be_record<P>(bytes, t, w);
}
MA_DEV void store_record(int k, unsigned char* bytes, size_t t, const word_t* w) {
#ifdef CHAIN_BOUT_LE
    if ((CHAIN_BOUT_LE >> k) & 1) { store_le_record<P>(bytes, t, w); return; }
#endif
    store_be_record<P>(bytes, t, w);
}
MA_DEV int take_sign(word_t* w) {
    const int s = (int)((w[TOPW] >> TOPB) & 1);
    w[TOPW] &= ~((word_t)1 << TOPB);
    return s;
}
MA_DEV void put_sign(word_t* w, int d) { w[TOPW] |= (word_t)(unsigned)d << TOPB; }       // (defined for d = 0 / 1)
constexpr bool BYTES_STAGED = CHAIN_BYTES_STAGED; // the path of a call on 16-byte aligned record arrays: the unit says (fuse.BYTES_IO_DEFAULT)
MA_DEV int imp_words(const word_t* w, spint* v) {
    Field<P>::limbs_from_words(w, v);
    return (int)Field<P>::modfsb(v);
}

template <int EPT> struct ByteIO : SoaIO<EPT> {       // direct: records EPT t .. EPT t + EPT - 1 of lane t, at their place in HBM
    const BArgs& B;
    MA_DEV void imp(int j, spint (*v)[P::N], int* s) const {
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            load_record(j, B.bin[j], (size_t)EPT * this->t + E, w);
            s[E] = imp_words(w, v[E]);
        });
    }
#ifdef CHAIN_BIN_SIGN
    MA_DEV void imp(int j, spint (*v)[P::N], int* s, int* sign) const {
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            load_record(j, B.bin[j], (size_t)EPT * this->t + E, w);
            sign[E] = take_sign(w);
            s[E] = imp_words(w, v[E]);
        });
    }
#endif
    MA_DEV void exp(int k, spint (*v)[P::N]) const {
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            Field<P>::words_from_limbs(v[E], w);
            store_record(k, B.bout[k], (size_t)EPT * this->t + E, w);
        });
    }
#ifdef CHAIN_BOUT_SIGN
    MA_DEV void exp(int k, spint (*v)[P::N], const int* sign) const {
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            Field<P>::words_from_limbs(v[E], w);
            put_sign(w, sign[E]);
            store_record(k, B.bout[k], (size_t)EPT * this->t + E, w);
        });
    }
#endif
};
template <int EPT>
__global__ __launch_bounds__(CBLOCK) CHAIN_KERNEL_ATTR void k_chain_direct(Args A, BArgs B, size_t nthreads, Ld L) {
    for (size_t t = (size_t)blockIdx.x * CBLOCK + threadIdx.x; t < nthreads; t += (size_t)gridDim.x * CBLOCK) chain_step<EPT>(ByteIO<EPT>{{A, L, t}, B});
}

// the LDS image of a stretch of records: UNIT bytes are what is moved in one piece (a record's 8-byte words, or its bytes), PITCH the
// bytes from one record to the next
constexpr int UNIT = NB % 8 == 0 ? 8 : 1, UPR = NB / UNIT;
constexpr int PITCH = UNIT == 8 ? (UPR | 1) * 8 : (((NB + 3) / 4) | 1) * 4;
constexpr int image_bytes(int ept) { return CBLOCK * ept * PITCH; }
constexpr int images(int ept) { return CHAIN_NBIN > 1 && CHAIN_NBIN * image_bytes(ept) <= 65536 ? CHAIN_NBIN : 1; }
constexpr bool STAGED_BUILT = image_bytes(EPT_BUILT) <= 65536;        // (a record too long for one image: the direct path only)
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
// `total` bytes at src (16-byte aligned) into the image: 16 bytes a lane and step, what is left of the last 16 byte by byte
MA_DEV void stage_in(const unsigned char* src, unsigned total, unsigned char* img) {
    for (unsigned o = 16u * threadIdx.x; o + 16 <= total; o += 16u * CBLOCK) {
        const u32x4 x = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(src + o));
        unsigned r = (o / UNIT) / UPR, i = (o / UNIT) % UPR;
        static_for<0, 16 / UNIT>([&](auto U) {
            constexpr int u = U;
            if constexpr (UNIT == 8) *reinterpret_cast<word_t*>(img + r * PITCH + i * 8) = (word_t)x[2 * u] | (word_t)x[2 * u + 1] << 32;
            else img[r * PITCH + i] = (unsigned char)(x[u / 4] >> (8 * (u % 4)));
            if (++i == UPR) { i = 0; r++; }
        });
    }
    for (unsigned o = (total & ~15u) + threadIdx.x; o < total; o += CBLOCK) img[(o / NB) * PITCH + o % NB] = src[o];
}
MA_DEV void stage_out(unsigned char* dst, unsigned total, const unsigned char* img) {
    for (unsigned o = 16u * threadIdx.x; o + 16 <= total; o += 16u * CBLOCK) {
        u32x4 x = {0, 0, 0, 0};
        unsigned r = (o / UNIT) / UPR, i = (o / UNIT) % UPR;
        static_for<0, 16 / UNIT>([&](auto U) {
            constexpr int u = U;
            if constexpr (UNIT == 8) {
                const word_t w = *reinterpret_cast<const word_t*>(img + r * PITCH + i * 8);
                x[2 * u] = (uint32_t)w; x[2 * u + 1] = (uint32_t)(w >> 32);
            } else {
                x[u / 4] |= (uint32_t)img[r * PITCH + i] << (8 * (u % 4));
            }
            if (++i == UPR) { i = 0; r++; }
        });
        __builtin_nontemporal_store(x, reinterpret_cast<u32x4*>(dst + o));
    }
    for (unsigned o = (total & ~15u) + threadIdx.x; o < total; o += CBLOCK) dst[o] = img[(o / NB) * PITCH + o % NB];
}
template <int... I> MA_DEV void stage_in_all(const BArgs& B, size_t first, unsigned total, unsigned char* sh, int image, std::integer_sequence<int, I...>) {
    (stage_in(B.bin[I] + first, total, sh + I * image), ...);
}
// staged: the workgroup's lanes are t0 .. t0 + CBLOCK - 1, the first cnt of them have elements.  The others take every barrier, compute
// on zeros (inside the limb contract: they vote with the wave) and store nothing, as the lanes beyond cnt of AosIO
template <int EPT> struct StagedIO {
    const Args& A; const BArgs& B; Ld L; size_t t0; unsigned cnt; unsigned char* sh;
    MA_DEV bool live() const { return threadIdx.x < cnt; }
    MA_DEV size_t t() const { return t0 + threadIdx.x; }
    MA_DEV size_t first() const { return t0 * EPT * NB; }                                  // the stretch of this workgroup in a record array
    MA_DEV unsigned char* mine(unsigned char* img, int e) const { return img + (threadIdx.x * EPT + e) * PITCH; }
    MA_DEV void load(int i, spint (*v)[P::N]) const {
        if (live()) load_soa<P, EPT>(A.in[i], L, t(), v);
        else static_for<0, EPT>([&](auto E) { static_for<0, P::N>([&](auto I) { v[E][I] = 0; }); });
    }
    MA_DEV const spint* shared(int j) const { return shared_of(A, j); }
    MA_DEV void sel(int k, int* s) const { static_for<0, EPT>([&](auto E) { s[E] = live() ? A.sel[k][(size_t)EPT * t() + E] : 0; }); }
    MA_DEV void store(int k, spint (*v)[P::N]) const { if (live()) store_soa<P, EPT>(A.out[k], L, t(), v); }
    MA_DEV void pred(int k, const int* s) const { static_for<0, EPT>([&](auto E) { if (live()) A.pred[k][(size_t)EPT * t() + E] = s[E]; }); }
    MA_DEV unsigned char* image_in(int j) const {         // the image that holds this workgroup's records of byte input j
        unsigned char* img = sh;
        if constexpr (images(EPT) == CHAIN_NBIN) {
            img += j * image_bytes(EPT);                  // (k_chain_staged has filled the images)
        } else {
            __syncthreads();                              // the previous user of the image is done
            stage_in(B.bin[j] + first(), cnt * EPT * NB, img);
            __syncthreads();
        }
        return img;
    }
    MA_DEV void imp(int j, spint (*v)[P::N], int* s) const {
        unsigned char* img = image_in(j);
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            if (live()) load_record(j, mine(img, E), 0, w);
            else static_for<0, NW>([&](auto K) { w[K] = 0; });
            s[E] = imp_words(w, v[E]);
        });
    }
#ifdef CHAIN_BIN_SIGN
    MA_DEV void imp(int j, spint (*v)[P::N], int* s, int* sign) const {
        unsigned char* img = image_in(j);
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            if (live()) load_record(j, mine(img, E), 0, w);
            else static_for<0, NW>([&](auto K) { w[K] = 0; });
            sign[E] = take_sign(w);
            s[E] = imp_words(w, v[E]);
        });
    }
#endif
    MA_DEV void exp(int k, spint (*v)[P::N]) const {
        __syncthreads();
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            Field<P>::words_from_limbs(v[E], w);
            if (live()) store_record(k, mine(sh, E), 0, w);
        });
        __syncthreads();
        stage_out(B.bout[k] + first(), cnt * EPT * NB, sh);
    }
#ifdef CHAIN_BOUT_SIGN
    MA_DEV void exp(int k, spint (*v)[P::N], const int* sign) const {
        __syncthreads();
        static_for<0, EPT>([&](auto E) {
            word_t w[NW];
            Field<P>::words_from_limbs(v[E], w);
            put_sign(w, sign[E]);
            if (live()) store_record(k, mine(sh, E), 0, w);
        });
        __syncthreads();
        stage_out(B.bout[k] + first(), cnt * EPT * NB, sh);
    }
#endif
};
// the loop is on the workgroup's base lane: block-uniform, since barriers sit inside it
template <int EPT>
__global__ __launch_bounds__(CBLOCK) CHAIN_KERNEL_ATTR void k_chain_staged(Args A, BArgs B, size_t nthreads, Ld L) {
    __shared__ __attribute__((aligned(16))) unsigned char sh[images(EPT) * image_bytes(EPT)];
    for (size_t t0 = (size_t)blockIdx.x * CBLOCK; t0 < nthreads; t0 += (size_t)gridDim.x * CBLOCK) {
        const unsigned cnt = nthreads - t0 < (size_t)CBLOCK ? (unsigned)(nthreads - t0) : (unsigned)CBLOCK;
        if constexpr (CHAIN_NBIN > 0 && images(EPT) == CHAIN_NBIN) {
            __syncthreads();
            stage_in_all(B, t0 * EPT * NB, cnt * EPT * NB, sh, image_bytes(EPT), std::make_integer_sequence<int, CHAIN_NBIN>());
            __syncthreads();
        }
        chain_step<EPT>(StagedIO<EPT>{A, B, L, t0, cnt, sh});
    }
}
#endif  // byte records

// ---- the host side of both entries.  A call's arrays as the kernels take them (the shared operands are read from the host here, once);
// addr / baddr: the OR of the addresses of the element arrays / of the record arrays
struct Call { Args A; BArgs B; uintptr_t addr = 0, baddr = 0; };
Call call_of(const void* const* in, void* const* out) {
    Call c;
    for (int i = 0; i < NIN; i++) { c.A.in[i] = (const spint*)in[i]; c.addr |= reinterpret_cast<uintptr_t>(in[i]); }
    for (int i = 0; i < NOUT; i++) { c.A.out[i] = (spint*)out[i]; c.addr |= reinterpret_cast<uintptr_t>(out[i]); }
    for (int i = 0; i < CHAIN_NBIN; i++) { c.B.bin[i] = (const unsigned char*)in[IN_BYTES + i]; c.baddr |= reinterpret_cast<uintptr_t>(in[IN_BYTES + i]); }
    for (int i = 0; i < CHAIN_NBOUT; i++) { c.B.bout[i] = (unsigned char*)out[OUT_BYTES + i]; c.baddr |= reinterpret_cast<uintptr_t>(out[OUT_BYTES + i]); }
    for (int i = 0; i < NSEL; i++) c.A.sel[i] = (const int*)in[IN_SEL + i];
    for (int i = 0; i < CHAIN_NPRED; i++) c.A.pred[i] = (int*)out[OUT_PRED + i];
#if CHAIN_NSHARED > 0
    for (int j = 0; j < CHAIN_NSHARED; j++)
        for (int i = 0; i < P::N; i++) c.A.sh[j].l[i] = static_cast<const spint*>(in[IN_SHARED + j])[i];
#endif
    return c;
}
// the same call from element `done` on; o: that element's offset in an element array.  (A copy: the shared operands are those already read)
Call rest_of(Call c, size_t done, size_t o) {
    for (int i = 0; i < NIN; i++) c.A.in[i] += o;
    for (int i = 0; i < NOUT; i++) c.A.out[i] += o;
    for (int i = 0; i < CHAIN_NBIN; i++) c.B.bin[i] += done * NB;
    for (int i = 0; i < CHAIN_NBOUT; i++) c.B.bout[i] += done * NB;
    for (int i = 0; i < NSEL; i++) c.A.sel[i] += done;
    for (int i = 0; i < CHAIN_NPRED; i++) c.A.pred[i] += done;
    return c;
}
// nt lanes of EPT elements each: k_chain, or with byte records one of their two kernels
template <int EPT> void launch(bool staged, const Call& c, size_t nt, Ld L, unsigned grid, hipStream_t s) {
#if CHAIN_BYTES
    if constexpr (STAGED_BUILT) if (staged) { k_chain_staged<EPT><<<grid, CBLOCK, 0, s>>>(c.A, c.B, nt, L); return; }
    k_chain_direct<EPT><<<grid, CBLOCK, 0, s>>>(c.A, c.B, nt, L);
#else
    k_chain<EPT><<<grid, CBLOCK, 0, s>>>(c.A, nt, L);
#endif
}

// Element batches are flat (ld >= n) or tiled (ld < n: the tile); without element arrays on either side ld is ignored.  Record arrays are
// 8-byte aligned where NBYTES is a multiple of 8 (the rule of modimp_<P>_batch) and may be anywhere otherwise; a byte output may be the
// array of a byte input
int chain_batch(const void* const* in, void* const* out, size_t n, size_t ld, void* stream) {
    if (n == 0) return 0;
    constexpr bool elems = NIN + NOUT > 0;
    Ld L(elems ? ld : n);
    if (elems && ld < n) {
        if (ld < 128 || (ld & (ld - 1)) != 0) { set_error(CHAIN_SYMBOL "_batch: a limb stride below n selects the tiled layout and must be a power of two >= 128"); return (int)hipErrorInvalidValue; }
        L = Ld(ld, (unsigned)__builtin_ctzll((unsigned long long)ld));
    }
    const Call c = call_of(in, out);
    bool staged = false;
#if CHAIN_BYTES
    if (NB % 8 == 0 && (c.baddr & 7u)) { set_error(CHAIN_SYMBOL "_batch: byte records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    staged = BYTES_STAGED;
    if (const char* v = getenv("MA_CHAIN_BYTES")) {
        const std::string m(v);
        if (m == "staged") staged = true;
        else if (m == "direct") staged = false;
        else { set_error(CHAIN_SYMBOL "_batch: MA_CHAIN_BYTES is staged or direct"); return (int)hipErrorInvalidValue; }
    }
    staged = staged && (c.baddr & 15u) == 0;
#endif
    hipStream_t s = (hipStream_t)stream;
    // elements per lane (the rules of the library's pick_ept, capi_field.inc, on the element arrays: a record array asks nothing of the
    // width): e elements need n >= e, a stride that is a multiple of e and rows aligned to e words; what is left over (fewer than e
    // elements) runs one element per lane at its own address, flat stride, records read and written directly
    size_t e = EPT_CAP;
    while (e > 1 && !(n >= e && (!elems || ld % e == 0) && (c.addr & (e * sizeof(spint) - 1)) == 0)) e /= 2;
    const size_t nt = n / e, done = nt * e;
    const unsigned grid = grid_for(nt, CBLOCK, L.s != 63);
    if constexpr (EPT_BUILT >= 4) if (e == 4) launch<4>(staged, c, nt, L, grid, s);
    if constexpr (EPT_BUILT >= 2) if (e == 2) launch<2>(staged, c, nt, L, grid, s);
    if (e == 1) launch<1>(staged, c, nt, L, grid, s);
    if (done < n) launch<1>(false, rest_of(c, done, L.off<P::N>(done)), n - done, Ld(L.ld), 1, s);
    return check_launch(CHAIN_SYMBOL "_batch");
}

#if defined(CHAIN_AOS_IMAGES) && CHAIN_AOS_IMAGES > 0
// ---- element-major I/O: x[n][N] in, x[n][N] out (how the scalar callers of field.c hold their elements).  A workgroup of 256 lanes
// takes a chunk of 512 elements; each array's chunk is one linear stretch of 512 N words, moved with 16-byte-per-lane coalesced accesses
// and transposed through LDS (pitch N | 1 words: two-way bank conflicts at most; the pattern of capi_common.hip k_convert_lds, which is
// why 64 KB hold fields of up to 14 limbs) into the lanes' registers -- elements 2t, 2t+1 -- and back.  The layout conversions on either
// side of a chain (160 bytes of HBM traffic per element and array) disappear into the kernel.
// CHAIN_AOS_IMAGES = NIN: one LDS image per input array while they fit 64 KB, so that every array's loads are issued before the first
// barrier (measured against one shared image: X25519 0.577 -> 0.517 ms, X448 1.089 -> 1.038 ms); = 1 < NIN: one image, array by array.
static_assert(CHAIN_AOS_IMAGES == 1 || CHAIN_AOS_IMAGES == NIN, "one image for all input arrays or one each");
constexpr int CH = 512, SP = P::N | 1;
MA_DEV void aos_load(const spint* aos, size_t cnt, spint* sh) {
    const int t = threadIdx.x;
    const size_t total = cnt * (size_t)P::N;
    int e = (2 * t) / P::N, i = (2 * t) % P::N;
    constexpr int de = CH / P::N, di = CH % P::N;
    for (size_t w = 2 * (size_t)t; w < total; w += CH) {
        int e1 = e, i1 = i + 1;
        if (i1 == P::N) { i1 = 0; e1++; }
        if (w + 1 < total) {
            const spint2 x = __builtin_nontemporal_load(reinterpret_cast<const spint2*>(aos + w));
            sh[e * SP + i] = x.x; sh[e1 * SP + i1] = x.y;
        } else {
            sh[e * SP + i] = aos[w];
        }
        e += de; i += di;
        if (i >= P::N) { i -= P::N; e++; }
    }
}
// every input array's chunk into its own image (a fold over the indices, not a static_for: a lambda around A costs the kernel registers)
template <int... I> MA_DEV void aos_load_all(const Args& A, size_t c0, size_t cnt, spint* sh, std::integer_sequence<int, I...>) {
    (aos_load(A.in[I] + c0 * (size_t)P::N, cnt, sh + I * CH * SP), ...);
}
MA_DEV void aos_regs(size_t cnt, const spint* sh, spint (*v)[P::N]) {
    const int t = threadIdx.x;
    static_for<0, 2>([&](auto E) {
        const bool live = 2 * (size_t)t + E < cnt;         // lanes beyond the chunk's end compute on zeros (inside the limb contract)
        static_for<0, P::N>([&](auto I) { v[E][I] = live ? sh[(2 * t + E) * SP + I] : 0; });
    });
}
MA_DEV void aos_in(const spint* aos, size_t cnt, spint* sh, spint (*v)[P::N]) {
    __syncthreads();                                  // the previous user of sh is done
    aos_load(aos, cnt, sh);
    __syncthreads();
    aos_regs(cnt, sh, v);
}
MA_DEV void aos_out(spint* aos, size_t cnt, spint* sh, spint (*v)[P::N]) {
    const int t = threadIdx.x;
    const size_t total = cnt * (size_t)P::N;
    __syncthreads();
    static_for<0, 2>([&](auto E) { static_for<0, P::N>([&](auto I) { sh[(2 * t + E) * SP + I] = v[E][I]; }); });
    __syncthreads();
    int e = (2 * t) / P::N, i = (2 * t) % P::N;
    constexpr int de = CH / P::N, di = CH % P::N;
    for (size_t w = 2 * (size_t)t; w < total; w += CH) {
        int e1 = e, i1 = i + 1;
        if (i1 == P::N) { i1 = 0; e1++; }
        if (w + 1 < total) {
            spint2 x; x.x = sh[e * SP + i]; x.y = sh[e1 * SP + i1];
            __builtin_nontemporal_store(x, reinterpret_cast<spint2*>(aos + w));
        } else {
            aos[w] = sh[e * SP + i];
        }
        e += de; i += di;
        if (i >= P::N) { i -= P::N; e++; }
    }
}
struct AosIO {                                        // two elements per lane: 2t, 2t + 1 of the chunk of cnt elements at c0
    const Args& A; spint* sh; size_t c0, cnt, off;
    MA_DEV void load(int i, spint (*v)[P::N]) const {
        if constexpr (CHAIN_AOS_IMAGES == NIN) aos_regs(cnt, sh + i * CH * SP, v);        // (k_chain_aos has filled the images)
        else aos_in(A.in[i] + off, cnt, sh, v);
    }
    MA_DEV const spint* shared(int j) const { return shared_of(A, j); }       // (straight from the kernel arguments: not through LDS)
    MA_DEV void sel(int k, int* s) const {
        const int t = threadIdx.x;
        const int* d = A.sel[k] + c0;
        static_for<0, 2>([&](auto E) { s[E] = (2 * (size_t)t + E < cnt) ? d[2 * (size_t)t + E] : 0; });
    }
    MA_DEV void store(int k, spint (*v)[P::N]) const { aos_out(A.out[k] + off, cnt, sh, v); }
    MA_DEV void pred(int k, const int* s) const {
        const int t = threadIdx.x;
        int* d = A.pred[k] + c0;
        static_for<0, 2>([&](auto E) { if (2 * (size_t)t + E < cnt) d[2 * (size_t)t + E] = s[E]; });
    }
};
__global__ __launch_bounds__(BLOCK) void k_chain_aos(Args A, size_t n) {
    __shared__ spint sh[CHAIN_AOS_IMAGES * CH * SP];
    for (size_t c0 = (size_t)blockIdx.x * CH; c0 < n; c0 += (size_t)gridDim.x * CH) {
        const size_t cnt = (n - c0 < (size_t)CH) ? n - c0 : (size_t)CH;
        if constexpr (CHAIN_AOS_IMAGES == NIN) {
            __syncthreads();
            aos_load_all(A, c0, cnt, sh, std::make_integer_sequence<int, NIN>());
            __syncthreads();
        }
        chain_step<2>(AosIO{A, sh, c0, cnt, c0 * (size_t)P::N});
    }
}

// element-major arrays spint x[n][Nlimbs], 16-byte aligned; nothing is asked of the int32 arrays
int chain_aos(const void* const* in, void* const* out, size_t n, void* stream) {
    if (n == 0) return 0;
    const Call c = call_of(in, out);
    if (c.addr & 15u) { set_error(CHAIN_SYMBOL "_aos: element-major arrays must be 16-byte aligned"); return (int)hipErrorInvalidValue; }
    const size_t chunks = (n + CH - 1) / CH;
    const size_t cap = (size_t)max_blocks_tiled();
    k_chain_aos<<<(unsigned)(chunks < cap ? chunks : cap), BLOCK, 0, (hipStream_t)stream>>>(c.A, n);
    return check_launch(CHAIN_SYMBOL "_aos");
}
#elif MA_WL == 64
int chain_aos(const void* const*, void* const*, size_t, void*) {        // no kernel: byte records have no layout, more than 14 limbs no image
    set_error(CHAIN_BYTES ? CHAIN_SYMBOL "_aos: a chain with byte records has no element-major entry; call " CHAIN_SYMBOL "_batch"
                          : CHAIN_SYMBOL "_aos: element-major I/O is built for fields of up to 14 limbs; convert with modarith_amd_aos_to_soa");
    return (int)hipErrorInvalidValue;
}
#endif
