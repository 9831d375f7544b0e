// g1_lincomb.cuh -- one term k * P of a short G1 linear combination, written once for the device kernel (g1_lincomb.hip, one
// term per lane) and for the host (its test hook, over Fq64Field).
//
// k is 256 raw bits, never reduced (the subgroup test multiplies by r itself).  Fixed 4-bit windows with signed digits:
//   k + 0x888...8 = sum n_w 16^w (65 nibbles, the top one is the carry: 0 or 1)   =>   k = c 16^64 + sum (n_w - 8) 16^w
// so every digit but the top is in [-8, 7] and the table holds 1 P .. 8 P.  Every lane of a wave is scheduled the same sequence --
// the table, then per window four doublings and ONE complete addition -- whatever its scalar is: the digit only selects the operand
// (table entry by address, sign and "zero digit" by field selects), never whether or how often an addition is issued.  No
// endomorphism: the points may be outside the subgroup.  The additions are ec.cuh's complete xyzz_add, so a point at infinity,
// P + P and P - P inside the chain are all handled -- by branches INSIDE it: a lane whose operand is infinity (a zero digit), whose
// accumulator still is (the leading zero windows) or whose operands meet at equal x leaves the addition early or takes its
// doubling arm, and sits masked while its neighbours run the general formulas.  The wave pays one full addition per window
// either way (plus the doubling arm in the windows where some lane needs it), which is the cost the fixed schedule was chosen for.
#pragma once
#include "ec.cuh"

namespace zk {

constexpr int LINCOMB_TAB = 8;           // table entries per term: e holds (e + 1) P
constexpr int LINCOMB_MAX_TERMS = 64;    // terms of a segment: one wave

// Tab: void put(int e, const XYZZ<F>&), XYZZ<F> get(int e) for e < LINCOMB_TAB -- the device keeps it in LDS (an entry chosen by a
// per-lane digit is an address there, not an index into a register array), the host in a local array.
// NW: 32-bit words of k (8: the 256 raw bits above; 4: a 128-bit coefficient, half the windows -- groth16_verify.hip)
template <class F, class Tab, int NW = 8>
ZK_HD XYZZ<F> lincomb_term(const Affine<F>& p, const uint32_t k[NW], Tab& tab) {
    uint32_t kk[NW], carry = 0;
#pragma unroll
    for (int i = 0; i < NW; i++) {
        const uint64_t t = (uint64_t)k[i] + 0x88888888u + carry;
        kk[i] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
    const XYZZ<F> P = xyzz_from_affine<F>(p);
    XYZZ<F> e = P;
    tab.put(0, e);
#pragma unroll 1
    for (int i = 1; i < LINCOMB_TAB; i++) {
        e = xyzz_add<F>(e, P);
        tab.put(i, e);
    }
    XYZZ<F> acc = carry ? P : xyzz_inf<F>();
#pragma unroll 1
    for (int w = 8 * NW - 1; w >= 0; w--) {
#pragma unroll 1
        for (int j = 0; j < 4; j++) acc = xyzz_dbl<F>(acc);
        const int d = (int)(kk[NW - 1] >> 28) - 8;
#pragma unroll
        for (int i = NW - 1; i > 0; i--) kk[i] = (kk[i] << 4) | (kk[i - 1] >> 28);
        kk[0] <<= 4;
        const int m = d < 0 ? -d : d;
        XYZZ<F> t = tab.get(m ? m - 1 : 0);
        t.y = F::select(d < 0, F::neg(t.y), t.y);
        t.zz = F::select(m == 0, F::zero(), t.zz);          // a zero digit adds infinity
        acc = xyzz_add<F>(acc, t);
    }
    return acc;
}

}  // namespace zk
