/* examples/field_consumer_w32.c -- a consumer of a GENERATED 32-bit field through its paste-marker shim.
 *
 * The reference's templates say "paste field.c here"; here that is  #include "field_<TAG>_w32.h"  (emitted next to the plug-in by
 * `python -m modarith_amd.generate w32 <prime>`), given as -DFIELD_HEADER='"field_BP256_w32.h"'.  Only the undecorated names and
 * macros of a generated field.c are used below (spint, Nlimbs, Nbytes, modint, modmul, ...): the same text compiles against the
 * reference's own field.c of that prime at word length 32.  Link libmodarith_amd.so and the field's plug-in.
 *
 *   gcc -O2 examples/field_consumer_w32.c -DFIELD_HEADER='"field_BP256_w32.h"' -Iinclude -Imodarith_amd/plugins \
 *       -Lmodarith_amd -l:libmodarith_amd.so -Lmodarith_amd/plugins -l:libmodarith_amd_BP256_w32.so -o consumer
 *
 * Prints the macro block and, as big-endian hex, 39081 / ((x y)^2 + x - y) for x = 1234567, y = 7654321, its square root flag and
 * whether the round trip through modexp / modimp gives the element back.
 */
#include FIELD_HEADER

int main(void) {
    spint x[Nlimbs], y[Nlimbs], z[Nlimbs], w[Nlimbs];
    char b[Nbytes];
    int i;
    printf("field Wordlength %d Nlimbs %d Radix %d Nbits %d Nbytes %d sizeof(spint) %d\n", Wordlength, Nlimbs, Radix, Nbits, Nbytes, (int)sizeof(spint));
    modint(1234567, x);
    modint(7654321, y);
    modmul(x, y, z);
    modsqr(z, z);
    modadd(z, x, z);
    modsub(z, y, z);
    modinv(z, NULL, z);
    modmli(z, 39081, z);
    modexp(z, b);
    printf("value ");
    for (i = 0; i < Nbytes; i++) printf("%02x", (unsigned char)b[i]);
    printf("\n");
    printf("qr %d\n", modqr(NULL, z));
    i = modimp(b, w);                 /* (its own statement: the order in which a call's arguments are evaluated is not fixed) */
    printf("import %d same %d\n", i, modcmp(w, z));
    modcpy(z, w);
    modneg(w, w);
    modadd(w, z, w);
    printf("zero %d one %d\n", modis0(w), modis1(w));
    return 0;
}
