// modarith_amd/csrc/shared_inv.h -- Montgomery's simultaneous inversion down one lane's column of items: the ONE walk behind k_fe_finish,
// k_fe_batch_div (fe_finish.h, on fe26.h / fe28.h), k_wn_export (wn_export.h) and k_wn_table_affine (wn_affine.h, on fm26.h / fk26.h):
// prefix products up the column, one inversion, two multiplications per item on the way back.  Host too (tools/shared_inv_host.hip).
//
// A denominator that is zero counts as ONE and its item leaves as its caller's answer for zero; every other item of the column gets
// exactly the inverse it would get alone.  What counts as one is decided by the policy's load_den() alone, and the walk calls that same
// function in both passes.  (Round 5, with two loops per caller: the table kernel's way down took it from the record's flag, not from the
// entry's Z.  An input off the curve, (x, 0, Z != 0), has Z = 0 in its entries 2P, 4P, 6P, 8P alone; that went into `inv` and zeroed the
// tables of every record EARLIER in the lane's column -- one unvalidated public key spoiled up to three other records of its batch.)
//
// The item policy POL, per lane:
//   valid(i)               item i exists.  PRECONDITION: it depends on the lane's index and uniform values only, and the valid items
//                          are a PREFIX of 0 .. count - 1 (r L + j < n is monotone in r).  The others are skipped by this index guard.
//   load_den(i, z) -> zero the denominator; where it is zero, z = 1 by a SELECT, never a branch.  The zero test is the caller's.
//   store_prefix(i, c), load_prefix(i, c)      the product of the denominators 0 .. i, in the caller's workspace
//   emit(i, zinv, zero)    multiply the numerators by zinv = 1 / z and write them out.  The answer for zero goes in through field.h's
//                          lane_mask(), not as `zero ? 0 : w`: that invites an EXEC region headed by a branch on lane data (ct_audit.py)
#pragma once
#include "field.h"

namespace ma {

template <class F, class POL>
MA_DEV void shared_inv_walk(int count, const POL& pol) {
    typename F::limb c[F::NLIMB], z[F::NLIMB], inv[F::NLIMB], zinv[F::NLIMB];
    F::set_one(c);
#pragma unroll 1
    for (int i = 0; i < count; i++) {
        if (!pol.valid(i)) continue;
        (void)pol.load_den(i, z);
        F::mul(z, c, c);            // (z first: its limb bounds are in sight, c's are lost behind the guard -- fe26.h then keeps 38 f g to one product)
        pol.store_prefix(i, c);
    }
    F::invert(c, inv);
#pragma unroll 1
    for (int i = count - 1; i >= 0; i--) {
        if (!pol.valid(i)) continue;                                // (never entered the product: nothing to undo)
        const bool zero = pol.load_den(i, z);                       // the SAME test as on the way up
        if (i > 0) {
            pol.load_prefix(i - 1, c);
            F::mul(inv, c, zinv);
            F::mul(inv, z, inv);
        } else {
            F::copy(inv, zinv);
        }
        pol.emit(i, zinv, zero);
    }
}

// load_den() for the redundant limbs of fm26.h / fk26.h: z = 1 where z is zero mod p; returns the flag
template <class F>
MA_DEV bool den_or_one(typename F::limb* z) {
    typename F::limb one[F::NLIMB];
    uint64_t zw[4];
    F::set_one(one);
    F::to_words(z, zw);
    const bool zero = (zw[0] | zw[1] | zw[2] | zw[3]) == 0;
    F::select(zero, z, one, z);
    return zero;
}

}  // namespace ma
