// modarith_amd/csrc/capi_field.inc -- the part of the per-prime C-ABI shim that is the same text at either word length: launch
// geometry, the launchers of the streaming kernels, every batched entry point without a product-policy choice, the modinv dispatch
// and the whole scalar (_ct) form.  Included by capi_prime.inc (64-bit words, namespace ma) and capi_w32.inc (32-bit words, namespace
// ma32) after kernels.h, with the namespace of the word length and ma's host helpers (capi_common.h) in scope and these defined:
//   P, NL, NB                    the prime's parameter struct, its limb and byte counts
//   BATCH(fn), SCALAR(fn)        the names of the entry points
//   MA_WHAT(fn), MA_WHAT2(fn, how)   the launch names modarith_amd_last_launch() reports: "modinv" / "modinv(h)" at 64 bits,
//                                "modinv(w32)" / "modinv(w32, h)" at 32
//   int ept_cap(), int stream_block()   widest access (elements per lane) and workgroup size the streaming kernels may take now
//   INV_SIMUL                    constexpr bool: modinv of this prime shares inversions on large batches
// The including file defines, after this one, what depends on its product policies: modmul, modsqr, nres, redc, modpro, modsqrt,
// modqr and the two functions declared below.  The limbs are spint (ma_spint / ma_spint32 of the public headers: the same types, and
// for the built-in primes the headers' prototypes are in scope, so a mismatch does not compile).

namespace {
// The limb stride argument of every batched entry point (include/modarith_amd.h): ld >= n is the flat layout, ld < n the tiled
// one (tiles of ld elements, ld a power of two >= 128) -> kernels.h Ld.  false (and the error text) for an unusable stride.
bool make_ld(size_t n, size_t ld, Ld* L, const char* what) {
    if (ld >= n) { *L = Ld(ld); return true; }
    if (ld < 128 || (ld & (ld - 1)) != 0) {
        set_error(std::string(what) + ": a limb stride below n selects the tiled layout and must be a power of two >= 128");
        return false;
    }
    *L = Ld(ld, (unsigned)__builtin_ctzll((unsigned long long)ld));
    return true;
}
#define GRID(x) grid_for((x), BLOCK, L.s != 63)       /* launch geometry of a kernel over the batch described by L */
#define MA_LD(what)                                                  \
    Ld L;                                                            \
    if (!make_ld(n, ld, &L, what)) return (int)hipErrorInvalidValue;

// Launch of a streaming kernel (k_binary, k_unary, k_mli) over a batch of n elements at limb stride ld whose buffers all sit at the
// addresses or-ed into `addr`.  EPT elements per lane need n >= EPT, a stride that is a multiple of EPT and rows aligned to the
// EPT * sizeof(spint) bytes of the access; the widest such EPT up to ept_cap() runs the body of the batch.  What is left over (fewer
// than EPT elements: they share a tile with their predecessors, tiles hold a multiple of four elements) runs one element per lane at
// its own address with the flat stride.  go(Width<E>, grid, block, o, cnt, l) launches the kernel of width E over cnt lanes from word o on.
uintptr_t U(const void* p) { return reinterpret_cast<uintptr_t>(p); }
int pick_ept(size_t n, size_t ld, uintptr_t addr) {
    for (int e = ept_cap(); e > 1; e >>= 1)
        if (n >= (size_t)e && ld % e == 0 && (addr & (e * sizeof(spint) - 1)) == 0) return e;
    return 1;
}
template <int E> using Width = std::integral_constant<int, E>;
// widest streaming kernel this unit COMPILES: a generated 32-bit unit names it (MA_W32_EPT_MAX = 1 | 2 | 4, chosen by the driver from
// the limb count so that no width it builds leaves the register budget: modarith_amd/emit.py w32_ept_max); its ept_cap() clamps to
// the same figure, so a width that is not compiled is never picked.  Undefined: every width of the word length, as before.
#ifdef MA_W32_EPT_MAX
constexpr int EPT_COMPILED = MA_W32_EPT_MAX;
#else
constexpr int EPT_COMPILED = 4;
#endif
template <class Go>
int launch_stream(size_t n, size_t ld, uintptr_t addr, const char* what, Go go) {
    if (n == 0) return 0;
    MA_LD(what)
    const int ept = pick_ept(n, ld, addr), sb = std::min(stream_block(), stream_block_max(ept));
    const size_t nt = n / ept, done = nt * ept;
    const unsigned grid = grid_for(nt, sb, L.s != 63);
    if (ept == 4) { if constexpr (MA_WL == 32 && EPT_COMPILED >= 4) go(Width<4>{}, grid, sb, 0, nt, L); }
    else if (ept == 2) { if constexpr (EPT_COMPILED >= 2) go(Width<2>{}, grid, sb, 0, nt, L); }
    else go(Width<1>{}, grid, sb, 0, nt, L);
    if (done < n) go(Width<1>{}, 1u, BLOCK, L.off<NL>(done), n - done, Ld(L.ld));
    return check_launch(what);
}
// (the one-element kernels of the voted functors run the exact products: kernels.h ScalarOp, the identity at 32 bits)
template <class Op, int E> using OpAt = typename std::conditional<E == 1, typename ScalarOp<Op>::type, Op>::type;
template <class Op>
int launch_binary(const spint* a, const spint* b, spint* c, size_t n, size_t ld, void* stream, const char* what) {
    return launch_stream(n, ld, U(a) | U(b) | U(c), what, [=](auto W, unsigned grid, int block, size_t o, size_t cnt, Ld l) {
        constexpr int E = decltype(W)::value;
        k_binary<P, OpAt<Op, E>, E><<<grid, block, 0, (hipStream_t)stream>>>(a + o, b + o, c + o, cnt, l, l, l);
    });
}
template <class Op>
int launch_unary(const spint* a, spint* c, size_t n, size_t ld, void* stream, const char* what) {
    return launch_stream(n, ld, U(a) | U(c), what, [=](auto W, unsigned grid, int block, size_t o, size_t cnt, Ld l) {
        constexpr int E = decltype(W)::value;
        k_unary<P, OpAt<Op, E>, E><<<grid, block, 0, (hipStream_t)stream>>>(a + o, c + o, cnt, l, l);
    });
}
// long-running per-element kernels (inversion, square root, progenitor): one element per lane
template <class Op>
int launch_unary_heavy(const spint* a, spint* c, size_t n, size_t ld, void* stream, const char* what) {
    if (n == 0) return 0;
    MA_LD(what)
    k_unary_heavy<P, Op><<<GRID(n), BLOCK, 0, (hipStream_t)stream>>>(a, c, n, L, L);
    return check_launch(what);
}
// the including file's: one inversion per element under its product policy, and whether its testing knobs leave inversions shared
int modinv_each(const spint* x, spint* z, size_t n, size_t ld, void* st);
bool inv_may_share();

// ---- scalar staging: run a batched call on one element held in host memory
struct Stage : StageBase {
    template <class T>
    T* put(const T* host, size_t count) {
        T* d = reinterpret_cast<T*>(take(count * sizeof(T)));
        if (host) h2d(d, host, count * sizeof(T));
        return d;
    }
    template <class T>
    void get(T* host, const T* dev, size_t count) { d2h(host, dev, count * sizeof(T)); }
};
}  // namespace

extern "C" {

// ------------------------------------------------------------------ batched form
int BATCH(modadd)(const spint* a, const spint* b, spint* c, size_t n, size_t ld, void* st) { return launch_binary<OpAdd<P>>(a, b, c, n, ld, st, MA_WHAT("modadd")); }
int BATCH(modsub)(const spint* a, const spint* b, spint* c, size_t n, size_t ld, void* st) { return launch_binary<OpSub<P>>(a, b, c, n, ld, st, MA_WHAT("modsub")); }
int BATCH(modneg)(const spint* b, spint* c, size_t n, size_t ld, void* st) { return launch_unary<OpNeg<P>>(b, c, n, ld, st, MA_WHAT("modneg")); }
int BATCH(modcpy)(const spint* a, spint* c, size_t n, size_t ld, void* st) { return launch_unary<OpCpy<P>>(a, c, n, ld, st, MA_WHAT("modcpy")); }
int BATCH(modmli)(const spint* a, int b, spint* c, size_t n, size_t ld, void* st) {
    return launch_stream(n, ld, U(a) | U(c), MA_WHAT("modmli"), [=](auto W, unsigned grid, int block, size_t o, size_t cnt, Ld l) {
        k_mli<P, decltype(W)::value><<<grid, block, 0, (hipStream_t)st>>>(a + o, b, c + o, cnt, l, l);
    });
}

// Large batches without a caller-supplied progenitor: simultaneous inversion (kernels.h k_inv_simul), one modinv per up to 64
// elements.  The prefix products go to the output buffer, or -- when the output IS the input -- to stream-ordered scratch of the
// library's own (not during stream capture; without scratch the per-element kernel runs).  MA_INV_SIMUL=0 keeps one modinv per
// element.  Same words either way (normalised outputs).
constexpr size_t INV_SIMUL_LANES = 16384;      // lanes kept busy before elements start sharing an inversion
constexpr size_t INV_SIMUL_MIN = 32768;        // batches from this size on share inversions
int BATCH(modinv)(const spint* x, const spint* h, spint* z, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modinv"))
    if constexpr (INV_SIMUL)
    if (h == nullptr && n >= INV_SIMUL_MIN && inv_simul() && inv_may_share()) {
        hipStream_t s = (hipStream_t)st;
        // elements per inversion: up to 64, fewer only for batches too small to leave 16 384 lanes busy (measured at 2^22
        // elements: 64 per inversion on 65 536 lanes 1.17e10/s, 32 per inversion on 131 072 lanes 1.11e10/s)
        size_t rounds = (n + INV_SIMUL_LANES - 1) / INV_SIMUL_LANES;
        if (rounds > 64) rounds = 64;
        const size_t lanes = (n + rounds - 1) / rounds;
        const unsigned grid = (unsigned)((lanes + BLOCK - 1) / BLOCK);
        if (x != z) {
            k_inv_simul<P><<<grid, BLOCK, 0, s>>>(x, z, z, n, lanes, (int)rounds, L, L, L);
            return check_launch(MA_WHAT2("modinv", "simultaneous"));
        }
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        if (s == nullptr || (hipStreamIsCapturing(s, &cs) == hipSuccess && cs == hipStreamCaptureStatusNone)) {
            if (spint* ws = static_cast<spint*>(scratch_alloc(n * NL * sizeof(spint), s))) {
                k_inv_simul<P><<<grid, BLOCK, 0, s>>>(x, z, ws, n, lanes, (int)rounds, L, L, Ld(n));
                scratch_free(ws, s);
                return check_launch(MA_WHAT2("modinv", "simultaneous, in place"));
            }
        }
        (void)hipGetLastError();
    }
    if (h == nullptr) return modinv_each(x, z, n, ld, st);
    k_inv_h<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, h, z, n, L, L, L);
    return check_launch(MA_WHAT2("modinv", "h"));
}

int BATCH(modnsqr)(spint* a, int k, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modnsqr"))
    k_nsqr<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, k, n, L);
    return check_launch(MA_WHAT("modnsqr"));
}

#define MA_INPLACE(fn, KIND)                                                                  \
    int BATCH(fn)(spint * a, int* out, size_t n, size_t ld, void* st) {                       \
        if (n == 0) return 0;                                                                 \
        MA_LD(MA_WHAT(#fn))                                                                   \
        k_inplace<P, KIND><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, out, n, L);             \
        return check_launch(MA_WHAT(#fn));                                                    \
    }
MA_INPLACE(modfsb, K_MODFSB)
MA_INPLACE(flatten, K_FLATTEN)
MA_INPLACE(prop, K_PROP)        /* flag[j] = -1 where the top limb went negative (the mask prop returns), else 0 */
int BATCH(modhaf)(spint* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modhaf"))
    k_inplace<P, K_MODHAF><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, nullptr, n, L);
    return check_launch(MA_WHAT("modhaf"));
}
#define MA_PRED(fn, KIND)                                                                     \
    int BATCH(fn)(const spint* a, int* out, size_t n, size_t ld, void* st) {                  \
        if (n == 0) return 0;                                                                 \
        MA_LD(MA_WHAT(#fn))                                                                   \
        k_inplace<P, KIND><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(const_cast<spint*>(a), out, n, L);\
        return check_launch(MA_WHAT(#fn));                                                    \
    }
MA_PRED(modis1, K_MODIS1)
MA_PRED(modis0, K_MODIS0)
MA_PRED(modsign, K_MODSIGN)
MA_PRED(modlimbs, K_MODLIMBS)
int BATCH(modcmp)(const spint* a, const spint* b, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modcmp"))
    k_cmp<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, b, out, n, L, L);
    return check_launch(MA_WHAT("modcmp"));
}
int BATCH(modshl)(unsigned int k, spint* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modshl"))
    k_shift<P, true><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(k, a, nullptr, n, L);
    return check_launch(MA_WHAT("modshl"));
}
int BATCH(modshr)(unsigned int k, spint* a, int* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modshr"))
    k_shift<P, false><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(k, a, out, n, L);
    return check_launch(MA_WHAT("modshr"));
}
int BATCH(modint)(int x, spint* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modint"))
    k_fill<P, K_INT><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(x, a, n, L);
    return check_launch(MA_WHAT("modint"));
}
int BATCH(modzer)(spint* a, size_t n, size_t ld, void* st) { return BATCH(modint)(0, a, n, ld, st); }
int BATCH(modone)(spint* a, size_t n, size_t ld, void* st) { return BATCH(modint)(1, a, n, ld, st); }
int BATCH(mod2r)(unsigned int r, spint* a, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("mod2r"))
    k_fill<P, K_2R><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>((int)r, a, n, L);
    return check_launch(MA_WHAT("mod2r"));
}
int BATCH(modcmv)(const int* d, const spint* g, spint* f, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modcmv"))
    k_cond<P, false><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(d, const_cast<spint*>(g), f, n, L, L);
    return check_launch(MA_WHAT("modcmv"));
}
int BATCH(modcsw)(const int* d, spint* g, spint* f, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modcsw"))
    k_cond<P, true><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(d, g, f, n, L, L);
    return check_launch(MA_WHAT("modcsw"));
}
int BATCH(modimp)(const char* b, spint* a, int* flag, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modimp"))
    if (NB % 8 == 0 && (reinterpret_cast<uintptr_t>(b) & 7u)) { set_error("modimp: byte records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    k_imp<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(reinterpret_cast<const unsigned char*>(b), a, flag, n, L);
    return check_launch(MA_WHAT("modimp"));
}
int BATCH(modexp)(const spint* a, char* b, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("modexp"))
    if (NB % 8 == 0 && (reinterpret_cast<uintptr_t>(b) & 7u)) { set_error("modexp: byte records must be 8-byte aligned"); return (int)hipErrorInvalidValue; }
    k_exp<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(a, reinterpret_cast<unsigned char*>(b), n, L);
    return check_launch(MA_WHAT("modexp"));
}

// synthetic inputs (kernels.h k_uniform): out[j] = canonical limbs of the (seed, array, first + j) element, uniform mod p
int BATCH(moduniform)(unsigned long long seed, unsigned long long array, size_t first, int plus_p, spint* out, size_t n, size_t ld, void* st) {
    if (n == 0) return 0;
    MA_LD(MA_WHAT("moduniform"))
    const uint64_t s0 = (uint64_t)seed * 0x9E3779B97F4A7C15ull + (uint64_t)array * 0xD1342543DE82EF95ull;
    k_uniform<P><<<GRID(n), BLOCK, 0, (hipStream_t)st>>>(s0, first, plus_p, out, n, L);
    return check_launch(MA_WHAT("moduniform"));
}

// ------------------------------------------------------------------ scalar form (n = 1 through the device)
// (the entry points the including file defines after this text; a generated field's unit has no header that declares them)
int BATCH(modmul)(const spint* a, const spint* b, spint* c, size_t n, size_t ld, void* st);
int BATCH(modsqr)(const spint* a, spint* c, size_t n, size_t ld, void* st);
int BATCH(modpro)(const spint* a, spint* c, size_t n, size_t ld, void* st);
int BATCH(nres)(const spint* a, spint* c, size_t n, size_t ld, void* st);
int BATCH(redc)(const spint* a, spint* c, size_t n, size_t ld, void* st);
int BATCH(modsqrt)(const spint* x, const spint* h, spint* r, size_t n, size_t ld, void* st);
int BATCH(modqr)(const spint* h, const spint* x, int* out, size_t n, size_t ld, void* st);
#define MA_SC_BIN(fn)                                                                         \
    void SCALAR(fn)(const spint* a, const spint* b, spint* c) {                               \
        Stage s;                                                                              \
        spint *da = s.put(a, NL), *db = s.put(b, NL), *dc = s.put<spint>(nullptr, NL);        \
        if (!s.bad) s.check(BATCH(fn)(da, db, dc, 1, 1, nullptr), #fn);                       \
        s.get(c, dc, NL);                                                                     \
    }
#define MA_SC_UN(fn)                                                                          \
    void SCALAR(fn)(const spint* a, spint* c) {                                               \
        Stage s;                                                                              \
        spint *da = s.put(a, NL), *dc = s.put<spint>(nullptr, NL);                            \
        if (!s.bad) s.check(BATCH(fn)(da, dc, 1, 1, nullptr), #fn);                           \
        s.get(c, dc, NL);                                                                     \
    }
MA_SC_BIN(modadd)
MA_SC_BIN(modsub)
MA_SC_BIN(modmul)
MA_SC_UN(modneg)
MA_SC_UN(modsqr)
MA_SC_UN(modcpy)
MA_SC_UN(modpro)
MA_SC_UN(nres)
MA_SC_UN(redc)

void SCALAR(modmli)(const spint* a, int b, spint* c) {
    Stage s;
    spint *da = s.put(a, NL), *dc = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modmli)(da, b, dc, 1, 1, nullptr), "modmli");
    s.get(c, dc, NL);
}
void SCALAR(modnsqr)(spint* a, int n) {
    Stage s;
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modnsqr)(da, n, 1, 1, nullptr), "modnsqr");
    s.get(a, da, NL);
}
void SCALAR(modinv)(const spint* x, const spint* h, spint* z) {
    Stage s;
    spint *dx = s.put(x, NL), *dh = h ? s.put(h, NL) : nullptr, *dz = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modinv)(dx, dh, dz, 1, 1, nullptr), "modinv");
    s.get(z, dz, NL);
}
void SCALAR(modsqrt)(const spint* x, const spint* h, spint* r) {
    Stage s;
    spint *dx = s.put(x, NL), *dh = h ? s.put(h, NL) : nullptr, *dr = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modsqrt)(dx, dh, dr, 1, 1, nullptr), "modsqrt");
    s.get(r, dr, NL);
}
int SCALAR(modqr)(const spint* h, const spint* x) {
    Stage s;
    spint *dx = s.put(x, NL), *dh = h ? s.put(h, NL) : nullptr;
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modqr)(dh, dx, dr, 1, 1, nullptr), "modqr");
    int r;
    s.get(&r, dr, 1);
    return s.answer(r);
}
#define MA_SC_INPLACE_RET(fn, rtype)                                                          \
    rtype SCALAR(fn)(spint* a) {                                                              \
        Stage s;                                                                              \
        spint* da = s.put(a, NL);                                                             \
        int* dr = s.put<int>(nullptr, 1);                                                     \
        if (!s.bad) s.check(BATCH(fn)(da, dr, 1, 1, nullptr), #fn);                           \
        int r;                                                                                \
        s.get(&r, dr, 1);                                                                     \
        s.get(a, da, NL);                                                                     \
        return (rtype)r;                                                                      \
    }
MA_SC_INPLACE_RET(modfsb, spint)
MA_SC_INPLACE_RET(flatten, spint)
MA_SC_INPLACE_RET(prop, spint)   /* (spint)(int)-1 = all ones, as pseudo.py:251 returns */
#define MA_SC_PRED(fn)                                                                        \
    int SCALAR(fn)(const spint* a) {                                                          \
        Stage s;                                                                              \
        spint* da = s.put(a, NL);                                                             \
        int* dr = s.put<int>(nullptr, 1);                                                     \
        if (!s.bad) s.check(BATCH(fn)(da, dr, 1, 1, nullptr), #fn);                           \
        int r;                                                                                \
        s.get(&r, dr, 1);                                                                     \
        return s.answer(r);                                                                   \
    }
MA_SC_PRED(modis1)
MA_SC_PRED(modis0)
MA_SC_PRED(modsign)
int SCALAR(modcmp)(const spint* a, const spint* b) {
    Stage s;
    spint *da = s.put(a, NL), *db = s.put(b, NL);
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modcmp)(da, db, dr, 1, 1, nullptr), "modcmp");
    int r;
    s.get(&r, dr, 1);
    return s.answer(r);
}
void SCALAR(modzer)(spint* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modzer)(da, 1, 1, nullptr), "modzer");
    s.get(a, da, NL);
}
void SCALAR(modone)(spint* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modone)(da, 1, 1, nullptr), "modone");
    s.get(a, da, NL);
}
void SCALAR(modint)(int x, spint* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(modint)(x, da, 1, 1, nullptr), "modint");
    s.get(a, da, NL);
}
void SCALAR(mod2r)(unsigned int r, spint* a) {
    Stage s;
    spint* da = s.put<spint>(nullptr, NL);
    if (!s.bad) s.check(BATCH(mod2r)(r, da, 1, 1, nullptr), "mod2r");
    s.get(a, da, NL);
}
void SCALAR(modcmv)(int b, const spint* g, volatile spint* f) {
    Stage s;
    int bb = b;
    int* dd = s.put(&bb, 1);
    spint *dg = s.put(g, NL), *df = s.put(const_cast<const spint*>(f), NL);
    if (!s.bad) s.check(BATCH(modcmv)(dd, dg, df, 1, 1, nullptr), "modcmv");
    s.get(const_cast<spint*>(f), df, NL);
}
void SCALAR(modcsw)(int b, volatile spint* g, volatile spint* f) {
    Stage s;
    int bb = b;
    int* dd = s.put(&bb, 1);
    spint *dg = s.put(const_cast<const spint*>(g), NL), *df = s.put(const_cast<const spint*>(f), NL);
    if (!s.bad) s.check(BATCH(modcsw)(dd, dg, df, 1, 1, nullptr), "modcsw");
    s.get(const_cast<spint*>(g), dg, NL);
    s.get(const_cast<spint*>(f), df, NL);
}
void SCALAR(modshl)(unsigned int n, spint* a) {
    Stage s;
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modshl)(n, da, 1, 1, nullptr), "modshl");
    s.get(a, da, NL);
}
int SCALAR(modshr)(unsigned int n, spint* a) {
    Stage s;
    spint* da = s.put(a, NL);
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modshr)(n, da, dr, 1, 1, nullptr), "modshr");
    int r;
    s.get(&r, dr, 1);
    s.get(a, da, NL);
    return r;
}
void SCALAR(modhaf)(spint* a) {
    Stage s;
    spint* da = s.put(a, NL);
    if (!s.bad) s.check(BATCH(modhaf)(da, 1, 1, nullptr), "modhaf");
    s.get(a, da, NL);
}
void SCALAR(modexp)(const spint* a, char* b) {
    Stage s;
    spint* da = s.put(a, NL);
    char* db = s.put<char>(nullptr, NB);
    if (!s.bad) s.check(BATCH(modexp)(da, db, 1, 1, nullptr), "modexp");
    s.get(b, db, NB);
}
int SCALAR(modimp)(const char* b, spint* a) {
    Stage s;
    char* db = s.put(b, NB);
    spint* da = s.put<spint>(nullptr, NL);
    int* dr = s.put<int>(nullptr, 1);
    if (!s.bad) s.check(BATCH(modimp)(db, da, dr, 1, 1, nullptr), "modimp");
    int r;
    s.get(&r, dr, 1);
    s.get(a, da, NL);
    return s.answer(r);
}

}  // extern "C"
