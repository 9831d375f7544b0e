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
// lincomb_term_glv (below) is the same schedule at half the windows for points KNOWN to be in the subgroup (g1_term_fold.hip's GLV mode).
#pragma once
#include "ec.cuh"
#include "hostfield64.hpp"

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
    // the carry digit: P or infinity, by a field select (a ?: between two points cost the kernels a 108-byte stack object per lane)
    XYZZ<F> acc = P;
    acc.zz = F::select(carry != 0, acc.zz, F::zero());
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

// ---- one term through the endomorphism --------------------------------------------------------------------------------------------
// (k1 + k2 lambda) P = k1 P + k2 phi(P) for P in the prime-order subgroup, phi(x, y) = (beta x, y) (hostfield64.hpp:
// host64_scalar_mul_glv has the curve facts; host64_glv_split makes the halves, below 2^127 each for k < r).  The halves are 128 raw
// bits each and any value up to 2^128 - 1 gives the right point: both are recoded as above (k + 0x88...8, 32 digits in [-8, 7] and a
// carry digit), and the carries enter before the first window.  ONE table 1 P .. 8 P serves both: phi of an entry (X, Y, ZZ, ZZZ) is
// (beta X, Y, ZZ, ZZZ), one product at the select.  The schedule is the same for every scalar -- seven table additions, the carry
// addition, then 32 windows of four doublings and two complete additions, the second one's operand through phi -- against 64 windows
// of four doublings and one addition for the plain term: about 200 group operations instead of 327.  On a point outside the subgroup
// phi is not lambda and the result means nothing, but the arithmetic is the same complete formulas and ends.
// Written in the form a one-term-per-lane kernel takes (digits select operands, never the control flow; GlvBeta<F> gives beta in
// F's form): instantiated over the host field (zk_diag_g1_glv_sum_host) and over G1Field by g1_term_fold.hip's k_g1_term_fold.
template <class F> struct GlvBeta;
template <> struct GlvBeta<Fq64Field> {
    static Fq64 get() { return Fq64Field::from_dev(fp_const<FqParams>(FqParams::BETA)); }
};

template <class F, class Tab>
ZK_HD XYZZ<F> lincomb_term_glv(const Affine<F>& p, const uint32_t k1[4], const uint32_t k2[4], Tab& tab) {
    uint32_t a[4], b[4], ca = 0, cb = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const uint64_t ta = (uint64_t)k1[i] + 0x88888888u + ca, tb = (uint64_t)k2[i] + 0x88888888u + cb;
        a[i] = (uint32_t)ta;
        ca = (uint32_t)(ta >> 32);
        b[i] = (uint32_t)tb;
        cb = (uint32_t)(tb >> 32);
    }
    const typename F::T beta = GlvBeta<F>::get();
    const XYZZ<F> P = xyzz_from_affine<F>(p);
    XYZZ<F> e = P;
    tab.put(0, e);
#pragma unroll 1
    for (int i = 1; i < LINCOMB_TAB; i++) {
        e = xyzz_add<F>(e, P);
        tab.put(i, e);
    }
    // the carry digits: ca P + cb phi(P)
    XYZZ<F> acc = P, t = P;
    acc.zz = F::select(ca != 0, acc.zz, F::zero());
    t.x = F::mul(t.x, beta);
    t.zz = F::select(cb != 0, t.zz, F::zero());
    acc = xyzz_add<F>(acc, t);
#pragma unroll 1
    for (int w = 31; w >= 0; w--) {
#pragma unroll 1
        for (int j = 0; j < 4; j++) acc = xyzz_dbl<F>(acc);
        const int da = (int)(a[3] >> 28) - 8, db = (int)(b[3] >> 28) - 8;
#pragma unroll
        for (int i = 3; i > 0; i--) {
            a[i] = (a[i] << 4) | (a[i - 1] >> 28);
            b[i] = (b[i] << 4) | (b[i - 1] >> 28);
        }
        a[0] <<= 4;
        b[0] <<= 4;
#pragma unroll 1
        for (int h = 0; h < 2; h++) {
            const int d = h ? db : da, m = d < 0 ? -d : d;
            t = tab.get(m ? m - 1 : 0);
            if (h) t.x = F::mul(t.x, beta);
            t.y = F::select(d < 0, F::neg(t.y), t.y);
            t.zz = F::select(m == 0, F::zero(), t.zz);      // a zero digit adds infinity
            acc = xyzz_add<F>(acc, t);
        }
    }
    return acc;
}

}  // namespace zk
