// subgroup.cuh -- membership in the prime-order subgroups of BLS12-377's G1 and G2, written once over a field policy (the interface
// ec.cuh uses): G1Field / G2Field of fp29.cuh for the device kernel (subgroup.hip, one point per lane), Fq64Field / Fq264Field of
// hostfield64.hpp for the host forms.
//
// Replaces (reference): GroupAffine::is_in_correct_subgroup_assuming_on_curve, ec/src/models/short_weierstrass_jacobian.rs:146-149
// (r P == O by the plain 253-bit chain), which GroupAffine::deserialize / deserialize_uncompressed (:888-940) call on every point.
//
// Both tests are exact -- the verdict is that of r P == O for EVERY point of the curve -- and run seed chains instead of the chain
// by r.  z = BLS12_X (64 bits, seven of them set): a chain [z] is 63 doublings and 6 additions.
//
//   G1.  phi(x, y) = (beta x, y) has phi^2 + phi + 1 = 0 on the whole curve, and lambda = z^2 - 1 has lambda^2 + lambda + 1 = r.
//        On the subgroup phi = lambda (gen_consts.py asserts it on the generator), so [z^2] P = P + phi(P) = -phi^2(P) =
//        (beta^2 x, -y).  Conversely [z^2] P = -phi^2(P) says phi(P) = lambda P, and then r P = (lambda^2 + lambda + 1) P =
//        (phi^2 + phi + 1)(P) = O.  The test is [z]([z] P) == (beta^2 x, -y): two chains, no final addition.
//   G2.  psi(x, y) = (conj(x) u^((q-1)/3), conj(y) u^((q-1)/2)) satisfies psi^2 - t psi + q = 0 with t = z + 1, and acts on G2 as
//        q = z (mod r).  psi(Q) = z Q gives (z^2 - (z + 1) z + q) Q = (q - z) Q = h1 r Q = O with h1 = (z - 1)^2 / 3; the order of Q
//        also divides #E'(Fq2) = h2 r, and gcd(h1, h2) = 1 (asserted by gen_consts.py), so r Q = O.  The test is [z] Q == psi(Q):
//        one chain; the two coefficients of psi lie in Fq (u^2 = -5, 12 | q - 1).
//
// The chains use ec.cuh's complete xyzz_dbl / xyzz_madd / xyzz_add: a point of order 2 or 3 reaches infinity INSIDE a chain and
// goes on from there.  The bits of z are the same on every lane, so lanes of a wave part only inside those rare arms.  The final
// comparison is projective (X == x' ZZ, Y == y' ZZZ, ZZ != 0): no inversion.  Infinity (all-zero words) is in the subgroup, as
// in the reference, where zero passes.  The point is taken to be on its curve.
#pragma once
#include "hostfield64.hpp"

namespace zk {

// the image the chain's result is compared with, per policy: -phi^2(P) on G1, psi(Q) on G2; CHAINS seed chains lead to it
template <class F> struct SubgroupEndo;
template <> struct SubgroupEndo<G1Field> {
    static constexpr int CHAINS = 2;
    static ZK_HD Affine<G1Field> image(const Affine<G1Field>& p) {
        return Affine<G1Field>{FqField::mul(p.x, fp_const<FqParams>(FqParams::BETA2)), FqField::neg(p.y)};
    }
};
template <> struct SubgroupEndo<G2Field> {
    static constexpr int CHAINS = 1;
    static ZK_HD Affine<G2Field> image(const Affine<G2Field>& p) {
        const Fq cx = fp_const<FqParams>(FqParams::PSI_CX), cy = fp_const<FqParams>(FqParams::PSI_CY);
        return Affine<G2Field>{Fq2{FqField::mul(p.x.c0, cx), FqField::neg(FqField::mul(p.x.c1, cx))},
                               Fq2{FqField::mul(p.y.c0, cy), FqField::neg(FqField::mul(p.y.c1, cy))}};
    }
};
template <> struct SubgroupEndo<Fq64Field> {
    static constexpr int CHAINS = 2;
    static Affine<Fq64Field> image(const Affine<Fq64Field>& p) {
        return Affine<Fq64Field>{Fq64Field::mul(p.x, Fq64Field::from_dev(fp_const<FqParams>(FqParams::BETA2))), Fq64Field::neg(p.y)};
    }
};
template <> struct SubgroupEndo<Fq264Field> {
    static constexpr int CHAINS = 1;
    static Affine<Fq264Field> image(const Affine<Fq264Field>& p) {
        using B = Fq64Field;
        const Fq64 cx = B::from_dev(fp_const<FqParams>(FqParams::PSI_CX)), cy = B::from_dev(fp_const<FqParams>(FqParams::PSI_CY));
        return Affine<Fq264Field>{Fq264{B::mul(p.x.c0, cx), B::neg(B::mul(p.x.c1, cx))}, Fq264{B::mul(p.y.c0, cy), B::neg(B::mul(p.y.c1, cy))}};
    }
};

template <class F> ZK_HD XYZZ<F> seed_add(const XYZZ<F>& acc, const Affine<F>& p) { return xyzz_madd<F>(acc, p); }
template <class F> ZK_HD XYZZ<F> seed_add(const XYZZ<F>& acc, const XYZZ<F>& p) { return xyzz_add<F>(acc, p); }

// [z] P from the top bit down; P affine (the table's point) or XYZZ (the first chain's result).  One copy of the doubling and one
// of the addition in the code: the loop is not unrolled, its branch is on a constant every lane shares.
template <class F, class P>
ZK_HD XYZZ<F> seed_mul(const XYZZ<F>& start, const P& p) {
    XYZZ<F> acc = start;
#pragma unroll 1
    for (int i = 62; i >= 0; i--) {
        acc = xyzz_dbl<F>(acc);
        if ((BLS12_X >> i) & 1) acc = seed_add<F>(acc, p);
    }
    return acc;
}

template <class F>
ZK_HD bool in_subgroup(const Affine<F>& p) {
    const bool inf = aff_is_inf<F>(p);
    XYZZ<F> w = seed_mul<F>(xyzz_from_affine<F>(p), p);
    if (SubgroupEndo<F>::CHAINS == 2) {
        const XYZZ<F> zp = w;
        w = seed_mul<F>(zp, zp);
    }
    const Affine<F> e = SubgroupEndo<F>::image(p);
    const bool same = F::eq(w.x, F::mul(e.x, w.zz)) & F::eq(w.y, F::mul(e.y, w.zzz)) & !F::is_zero(w.zz);
    return inf | same;
}

}  // namespace zk
