// pairing.cuh -- the BLS12-377 pairing: the tower Fq12 over Fq2, the Miller loop and the final exponentiation, written ONCE over
// an Fq2 policy (the interface ec.cuh uses): Fq2Field of fp29.cuh on the device, Fq264Field of hostfield64.hpp on the host.
//
// Replaces (reference):
//   arkworks/algebra/ff/src/fields/models/{fp6_3over2,fp12_2over3over2}.rs          the tower, Frobenius maps, cyclotomic squaring
//   arkworks/algebra/ec/src/models/bls12/{mod.rs,g2.rs}                              miller_loop / final_exponentiation, line steps
//   arkworks/curves/bls12_377/src/curves/mod.rs:16-19                                x, D-type twist
//
// Tower (the reference's Fq12Parameters, fields/fq12.rs): Fq2 = Fq[u]/(u^2 + 5), Fq6 = Fq2[v]/(v^3 - u), Fq12 = Fq6[w]/(w^2 - v).  An element is
// c[i].c[j] (i < 2, j < 3), the Fq2 coefficient of w^(2 j + i); as one polynomial in w over Fq (w^12 = -5) the Fq component h of
// c[i].c[j] is the coefficient of w^(2 j + i + 6 h).  Every value is fully reduced (the exact domain of the policy): equality of
// elements is equality of words, which is what the verdicts compare.  The lazy domain of fp29.cuh is not used: Fq2Field's fused
// products take fully reduced operands.
//
// The GT value.  pairing(P, Q) = miller(P, Q)^(3 (q^12 - 1) / r): the hard part is the chain of Hayashida, Hayasaka and Teruya,
// "Efficient final exponentiation via cyclotomic structure for pairings over families of elliptic curves" (eprint 2020/875, the
// BLS12 case): 3 (q^4 - q^2 + 1) / r = (x - 1)^2 (x + q) (x^2 + q^2 - 1) + 3 (gen_consts.py asserts the identity), five
// exponentiations by x in cyclotomic squarings (Granger, Scott: "Faster squaring in the cyclotomic subgroup of sixth degree
// extensions", eprint 2009/565).  3 is coprime to r, so "is one" and "are equal" mean what they mean for the plain power.
#define ZK_GT_EXPONENT_MULTIPLE 3
//
// Miller loop: over the bits of x below the top one, Q walked in homogeneous projective coordinates on the twist y^2 = x^3 + 1/u
// (Costello, Lange, Naehrig: "Faster pairing computations on curves with high-degree twists", eprint 2009/615: no inversion), each
// line evaluated at P and folded in by the sparse product (coefficients of w^0, w^1, w^3).  Lines are scaled by Fq2 factors, which
// the final exponentiation removes.  P or Q at infinity: the loop runs on the words as they are (there is no inversion to trip
// over) and the result is replaced by 1 at the end -- lanes of a wave never part on data.
//
// Shape on the device: every Fq12-level function and the Fq2 product itself are real calls (noinline), values are passed by
// address.  One Fq2 product is ~2 200 instructions; a Miller loop and a final exponentiation hold ~120 textual products, and
// inlined they would be a megabyte of code.  Temporaries therefore live in scratch (pairing.hip reports the figures).
#pragma once
#include "hostfield64.hpp"

namespace zk {

constexpr int FQ12_WORDS = 144;     // 32-bit words of an Fq12, packed or in the ABI's form (zk_gt)

#define ZK_PAIR_FN __host__ __device__ __attribute__((noinline))

// what the tower needs beyond the policy interface
template <class F2> struct PairingField;
template <> struct PairingField<Fq2Field> {
    using B = FqField;
    static ZK_HD Fq base_const(const uint32_t (&c)[13]) { return fp_const<FqParams>(c); }
    static ZK_HD Fq2 from_ext(const uint32_t* w24) { return Fq2Field::ext_to_int(Fq2Field::load(w24)); }
    static ZK_HD void to_ext(uint32_t* w24, const Fq2& a) { Fq2Field::store(w24, Fq2Field::int_to_ext(a)); }
};
template <> struct PairingField<Fq264Field> {
    using B = Fq64Field;
    static Fq64 base_const(const uint32_t (&c)[13]) { return Fq64Field::from_dev(fp_const<FqParams>(c)); }
    static Fq264 from_ext(const uint32_t* w24) { return Fq264Field::load(w24); }
    static void to_ext(uint32_t* w24, const Fq264& a) { Fq264Field::store(w24, a); }
};

template <class F2> struct Fq6 { typename F2::T c[3]; };
template <class F2> struct Fq12 { Fq6<F2> c[2]; };
template <class F2> struct Line { typename F2::T l0, l3, l4; };     // l0 + l3 w + l4 w^3

// ---- Fq2 helpers ------------------------------------------------------------------------------------------------------------------
template <class F2> ZK_PAIR_FN typename F2::T pf_mul(const typename F2::T& a, const typename F2::T& b) { return F2::mul(a, b); }
template <class F2> ZK_PAIR_FN typename F2::T pf_sqr(const typename F2::T& a) { return F2::sqr(a); }
template <class F2> ZK_HD typename F2::T pf_mul_base(const typename F2::T& a, const typename F2::B::T& k) {
    return typename F2::T{F2::B::mul(a.c0, k), F2::B::mul(a.c1, k)};
}
template <class F2> ZK_HD typename F2::T pf_mul_u(const typename F2::T& a) {      // (c0 + c1 u) u = -5 c1 + c0 u
    return typename F2::T{F2::B::neg(F2::mul5(a.c1)), a.c0};
}
template <class F2> ZK_HD typename F2::T pf_conj(const typename F2::T& a) { return typename F2::T{a.c0, F2::B::neg(a.c1)}; }
template <class F2> ZK_HD typename F2::T pf_triple(const typename F2::T& a) { return F2::add(F2::dbl(a), a); }

// ---- Fq6 ----------------------------------------------------------------------------------------------------------------------------
template <class F2> ZK_HD Fq6<F2> fq6_add(const Fq6<F2>& a, const Fq6<F2>& b) {
    return Fq6<F2>{{F2::add(a.c[0], b.c[0]), F2::add(a.c[1], b.c[1]), F2::add(a.c[2], b.c[2])}};
}
template <class F2> ZK_HD Fq6<F2> fq6_sub(const Fq6<F2>& a, const Fq6<F2>& b) {
    return Fq6<F2>{{F2::sub(a.c[0], b.c[0]), F2::sub(a.c[1], b.c[1]), F2::sub(a.c[2], b.c[2])}};
}
template <class F2> ZK_HD Fq6<F2> fq6_neg(const Fq6<F2>& a) { return Fq6<F2>{{F2::neg(a.c[0]), F2::neg(a.c[1]), F2::neg(a.c[2])}}; }
template <class F2> ZK_HD Fq6<F2> fq6_mul_v(const Fq6<F2>& a) { return Fq6<F2>{{pf_mul_u<F2>(a.c[2]), a.c[0], a.c[1]}}; }   // v^3 = u
// Karatsuba over three terms: six Fq2 products
template <class F2> ZK_PAIR_FN void fq6_mul(Fq6<F2>& r, const Fq6<F2>& a, const Fq6<F2>& b) {
    using T = typename F2::T;
    const T v0 = pf_mul<F2>(a.c[0], b.c[0]), v1 = pf_mul<F2>(a.c[1], b.c[1]), v2 = pf_mul<F2>(a.c[2], b.c[2]);
    const T t12 = F2::sub(F2::sub(pf_mul<F2>(F2::add(a.c[1], a.c[2]), F2::add(b.c[1], b.c[2])), v1), v2);
    const T t01 = F2::sub(F2::sub(pf_mul<F2>(F2::add(a.c[0], a.c[1]), F2::add(b.c[0], b.c[1])), v0), v1);
    const T t02 = F2::sub(F2::sub(pf_mul<F2>(F2::add(a.c[0], a.c[2]), F2::add(b.c[0], b.c[2])), v0), v2);
    r.c[0] = F2::add(v0, pf_mul_u<F2>(t12));
    r.c[1] = F2::add(t01, pf_mul_u<F2>(v2));
    r.c[2] = F2::add(t02, v1);
}
// a (d0 + d1 v): five products
template <class F2> ZK_PAIR_FN void fq6_mul_by_01(Fq6<F2>& r, const Fq6<F2>& a, const typename F2::T& d0, const typename F2::T& d1) {
    using T = typename F2::T;
    const T v0 = pf_mul<F2>(a.c[0], d0), v1 = pf_mul<F2>(a.c[1], d1);
    const T t01 = F2::sub(F2::sub(pf_mul<F2>(F2::add(a.c[0], a.c[1]), F2::add(d0, d1)), v0), v1);
    const T a2d1 = pf_mul<F2>(a.c[2], d1), a2d0 = pf_mul<F2>(a.c[2], d0);
    r.c[0] = F2::add(v0, pf_mul_u<F2>(a2d1));
    r.c[1] = t01;
    r.c[2] = F2::add(a2d0, v1);
}
template <class F2> ZK_PAIR_FN void fq6_inv(Fq6<F2>& r, const Fq6<F2>& a) {
    using T = typename F2::T;
    const T c0 = F2::sub(pf_sqr<F2>(a.c[0]), pf_mul_u<F2>(pf_mul<F2>(a.c[1], a.c[2])));
    const T c1 = F2::sub(pf_mul_u<F2>(pf_sqr<F2>(a.c[2])), pf_mul<F2>(a.c[0], a.c[1]));
    const T c2 = F2::sub(pf_sqr<F2>(a.c[1]), pf_mul<F2>(a.c[0], a.c[2]));
    const T n = F2::add(pf_mul<F2>(a.c[0], c0), pf_mul_u<F2>(F2::add(pf_mul<F2>(a.c[2], c1), pf_mul<F2>(a.c[1], c2))));
    const T ni = F2::inv(n);          // the inverse of zero is zero (Fermat), on both policies
    r.c[0] = pf_mul<F2>(c0, ni);
    r.c[1] = pf_mul<F2>(c1, ni);
    r.c[2] = pf_mul<F2>(c2, ni);
}

// ---- Fq12 ---------------------------------------------------------------------------------------------------------------------------
template <class F2> ZK_HD Fq12<F2> fq12_one() {
    Fq12<F2> r;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) r.c[i].c[j] = F2::zero();
    r.c[0].c[0] = F2::one();
    return r;
}
template <class F2> ZK_HD bool fq12_eq(const Fq12<F2>& a, const Fq12<F2>& b) {
    bool e = true;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) e = e & F2::eq(a.c[i].c[j], b.c[i].c[j]);
    return e;
}
template <class F2> ZK_HD Fq12<F2> fq12_add(const Fq12<F2>& a, const Fq12<F2>& b) { return Fq12<F2>{{fq6_add<F2>(a.c[0], b.c[0]), fq6_add<F2>(a.c[1], b.c[1])}}; }
template <class F2> ZK_HD Fq12<F2> fq12_sub(const Fq12<F2>& a, const Fq12<F2>& b) { return Fq12<F2>{{fq6_sub<F2>(a.c[0], b.c[0]), fq6_sub<F2>(a.c[1], b.c[1])}}; }
template <class F2> ZK_HD Fq12<F2> fq12_conj(const Fq12<F2>& a) { return Fq12<F2>{{a.c[0], fq6_neg<F2>(a.c[1])}}; }      // the q^6-power map
// r may alias a or b
template <class F2> ZK_PAIR_FN void fq12_mul(Fq12<F2>& r, const Fq12<F2>& a, const Fq12<F2>& b) {
    Fq6<F2> v0, v1, s;
    fq6_mul<F2>(v0, a.c[0], b.c[0]);
    fq6_mul<F2>(v1, a.c[1], b.c[1]);
    fq6_mul<F2>(s, fq6_add<F2>(a.c[0], a.c[1]), fq6_add<F2>(b.c[0], b.c[1]));
    r.c[1] = fq6_sub<F2>(fq6_sub<F2>(s, v0), v1);
    r.c[0] = fq6_add<F2>(v0, fq6_mul_v<F2>(v1));
}
// complex squaring: (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1 + 2 a0 a1 w
template <class F2> ZK_PAIR_FN void fq12_sqr(Fq12<F2>& r, const Fq12<F2>& a) {
    Fq6<F2> m, s;
    fq6_mul<F2>(m, a.c[0], a.c[1]);
    fq6_mul<F2>(s, fq6_add<F2>(a.c[0], a.c[1]), fq6_add<F2>(a.c[0], fq6_mul_v<F2>(a.c[1])));
    r.c[0] = fq6_sub<F2>(fq6_sub<F2>(s, m), fq6_mul_v<F2>(m));
    r.c[1] = fq6_add<F2>(m, m);
}
// the sparse product by a line l0 + l3 w + l4 w^3 = l0 + (l3 + l4 v) w: 13 Fq2 products
template <class F2> ZK_PAIR_FN void fq12_mul_line(Fq12<F2>& r, const Fq12<F2>& a, const Line<F2>& l) {
    Fq6<F2> v0, v1, s;
    for (int j = 0; j < 3; j++) v0.c[j] = pf_mul<F2>(a.c[0].c[j], l.l0);
    fq6_mul_by_01<F2>(v1, a.c[1], l.l3, l.l4);
    fq6_mul_by_01<F2>(s, fq6_add<F2>(a.c[0], a.c[1]), F2::add(l.l0, l.l3), l.l4);
    r.c[1] = fq6_sub<F2>(fq6_sub<F2>(s, v0), v1);
    r.c[0] = fq6_add<F2>(v0, fq6_mul_v<F2>(v1));
}
template <class F2> ZK_PAIR_FN void fq12_inv(Fq12<F2>& r, const Fq12<F2>& a) {      // (a0 - a1 w) / (a0^2 - v a1^2)
    Fq6<F2> t0, t1, ni;
    fq6_mul<F2>(t0, a.c[0], a.c[0]);
    fq6_mul<F2>(t1, a.c[1], a.c[1]);
    fq6_inv<F2>(ni, fq6_sub<F2>(t0, fq6_mul_v<F2>(t1)));
    fq6_mul<F2>(t0, a.c[0], ni);
    fq6_mul<F2>(t1, a.c[1], ni);
    r.c[0] = t0;
    r.c[1] = fq6_neg<F2>(t1);
}
// the q^J-power map, J = 1, 2, 3: the coefficient of w^k is conjugated J times and scaled by FQ12_FROB[J - 1][k], an Fq element
template <class F2, int J> ZK_PAIR_FN void fq12_frobenius(Fq12<F2>& r, const Fq12<F2>& a) {
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) {
            const typename F2::T t = (J & 1) ? pf_conj<F2>(a.c[i].c[j]) : a.c[i].c[j];
            r.c[i].c[j] = pf_mul_base<F2>(t, PairingField<F2>::base_const(i ? FQ12_FROB[J - 1][2 * j + 1] : FQ12_FROB[J - 1][2 * j]));
        }
}
// the square of an element of the cyclotomic subgroup (a^(q^6 + 1) = 1 and a^(q^4 - q^2 + 1) = 1; anything else: not its
// square), Granger-Scott: three squarings in Fq4 = Fq2[s]/(s^2 - u), six Fq2 products.  The Fq4 pairs are (c00, c11), (c10, c02),
// (c01, c12) with c_ij = c[i].c[j].
template <class F2> ZK_PAIR_FN void fq12_cyclotomic_sqr(Fq12<F2>& r, const Fq12<F2>& a) {
    using T = typename F2::T;
    // (x + y s)^2 = (x^2 + u y^2) + 2 x y s, as (x + y)(x + u y) - xy - u xy
    auto sq4 = [](const T& x, const T& y, T& lo, T& hi) {
        const T m = pf_mul<F2>(x, y);
        lo = F2::sub(F2::sub(pf_mul<F2>(F2::add(x, y), F2::add(x, pf_mul_u<F2>(y))), m), pf_mul_u<F2>(m));
        hi = F2::dbl(m);
    };
    T t0, t1, t2, t3, t4, t5;
    sq4(a.c[0].c[0], a.c[1].c[1], t0, t1);
    sq4(a.c[1].c[0], a.c[0].c[2], t2, t3);
    sq4(a.c[0].c[1], a.c[1].c[2], t4, t5);
    auto m3s2 = [](const T& t, const T& z) { return F2::add(F2::dbl(F2::sub(t, z)), t); };      // 3 t - 2 z
    auto m3a2 = [](const T& t, const T& z) { return F2::add(F2::dbl(F2::add(t, z)), t); };      // 3 t + 2 z
    const T z00 = m3s2(t0, a.c[0].c[0]), z11 = m3a2(t1, a.c[1].c[1]);
    const T z10 = m3a2(pf_mul_u<F2>(t5), a.c[1].c[0]), z02 = m3s2(t4, a.c[0].c[2]);
    const T z01 = m3s2(t2, a.c[0].c[1]), z12 = m3a2(t3, a.c[1].c[2]);
    r.c[0].c[0] = z00; r.c[0].c[1] = z01; r.c[0].c[2] = z02;
    r.c[1].c[0] = z10; r.c[1].c[1] = z11; r.c[1].c[2] = z12;
}

// a^x for a in the cyclotomic subgroup (x = BLS12_X: 64 bits, seven of them set)
template <class F2> ZK_PAIR_FN void fq12_cyclotomic_exp_x(Fq12<F2>& r, const Fq12<F2>& a) {
    Fq12<F2> t = a;
    for (int i = 62; i >= 0; i--) {
        fq12_cyclotomic_sqr<F2>(t, t);
        if ((BLS12_X >> i) & 1) fq12_mul<F2>(t, t, a);
    }
    r = t;
}

// ---- ABI form: 12 Fq in the reference's Montgomery words, tower order (c[i].c[j].c0, .c1 at words 24 (3 i + j)) -----------------------
template <class F2> ZK_HD Fq12<F2> fq12_from_ext(const uint32_t* w144) {
    Fq12<F2> r;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) r.c[i].c[j] = PairingField<F2>::from_ext(w144 + 24 * (3 * i + j));
    return r;
}
template <class F2> ZK_HD void fq12_to_ext(uint32_t* w144, const Fq12<F2>& a) {
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) PairingField<F2>::to_ext(w144 + 24 * (3 * i + j), a.c[i].c[j]);
}

// ---- Miller loop --------------------------------------------------------------------------------------------------------------------
template <class F2> struct TwistPoint { typename F2::T x, y, z; };      // homogeneous projective: (X / Z, Y / Z)

// T <- 2 T; the tangent at T evaluated at P = (xp, yp), scaled by -2 Y Z
template <class F2> ZK_PAIR_FN void miller_double(TwistPoint<F2>& t, Line<F2>& l, const typename F2::B::T& xp, const typename F2::B::T& yp) {
    using T = typename F2::T;
    using PF = PairingField<F2>;
    const typename F2::B::T inv2 = PF::base_const(FqParams::INV2);
    const T b3 = pf_triple<F2>(T{F2::B::zero(), PF::base_const(FqParams::G2_B_C1)});      // 3 b', b' = 1 / u (curves/g2.rs:28-35)
    const T a = pf_mul_base<F2>(pf_mul<F2>(t.x, t.y), inv2);
    const T b = pf_sqr<F2>(t.y), c = pf_sqr<F2>(t.z);
    const T e = pf_mul<F2>(b3, c);
    const T f = pf_triple<F2>(e);
    const T g = pf_mul_base<F2>(F2::add(b, f), inv2);
    const T h = F2::sub(pf_sqr<F2>(F2::add(t.y, t.z)), F2::add(b, c));      // 2 Y Z
    const T j = pf_sqr<F2>(t.x);
    const T ee = pf_sqr<F2>(e);
    t.x = pf_mul<F2>(a, F2::sub(b, f));
    t.y = F2::sub(pf_sqr<F2>(g), pf_triple<F2>(ee));
    t.z = pf_mul<F2>(b, h);
    l.l0 = pf_mul_base<F2>(F2::neg(h), yp);
    l.l3 = pf_mul_base<F2>(pf_triple<F2>(j), xp);
    l.l4 = F2::sub(e, b);
}
// T <- T + Q (Q affine); the chord through T and Q evaluated at P, scaled by X - x_Q Z
template <class F2> ZK_PAIR_FN void miller_add(TwistPoint<F2>& t, Line<F2>& l, const Affine<F2>& q, const typename F2::B::T& xp, const typename F2::B::T& yp) {
    using T = typename F2::T;
    const T theta = F2::sub(t.y, pf_mul<F2>(q.y, t.z));
    const T lambda = F2::sub(t.x, pf_mul<F2>(q.x, t.z));
    const T c = pf_sqr<F2>(theta), d = pf_sqr<F2>(lambda);
    const T e = pf_mul<F2>(lambda, d), f = pf_mul<F2>(t.z, c), g = pf_mul<F2>(t.x, d);
    const T h = F2::sub(F2::add(e, f), F2::dbl(g));
    const T x3 = pf_mul<F2>(lambda, h);
    const T y3 = F2::sub(pf_mul<F2>(theta, F2::sub(g, h)), pf_mul<F2>(e, t.y));
    t.z = pf_mul<F2>(t.z, e);
    t.x = x3;
    t.y = y3;
    l.l0 = pf_mul_base<F2>(lambda, yp);
    l.l3 = pf_mul_base<F2>(F2::neg(theta), xp);
    l.l4 = F2::sub(pf_mul<F2>(theta, q.x), pf_mul<F2>(lambda, q.y));
}

// f_{x, Q}(P); 1 if P or Q is the point at infinity (all-zero coordinates)
template <class F2> ZK_PAIR_FN void miller_loop(Fq12<F2>& f, const Affine<typename F2::B>& p, const Affine<F2>& q) {
    const bool inf = aff_is_inf<typename F2::B>(p) | aff_is_inf<F2>(q);
    TwistPoint<F2> t{q.x, q.y, F2::one()};
    Line<F2> l;
    Fq12<F2> acc = fq12_one<F2>();
    for (int i = 62; i >= 0; i--) {                 // the bits of x are the same on every lane
        fq12_sqr<F2>(acc, acc);
        miller_double<F2>(t, l, p.x, p.y);
        fq12_mul_line<F2>(acc, acc, l);
        if ((BLS12_X >> i) & 1) {
            miller_add<F2>(t, l, q, p.x, p.y);
            fq12_mul_line<F2>(acc, acc, l);
        }
    }
    const Fq12<F2> one = fq12_one<F2>();
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) f.c[i].c[j] = inf ? one.c[i].c[j] : acc.c[i].c[j];
}

// f^(3 (q^12 - 1) / r); f != 0
template <class F2> ZK_PAIR_FN void final_exponentiation(Fq12<F2>& r, const Fq12<F2>& f) {
    Fq12<F2> m, a, b, c, t;
    // easy part: f^((q^6 - 1)(q^2 + 1))
    fq12_inv<F2>(t, f);
    fq12_mul<F2>(t, fq12_conj<F2>(f), t);
    fq12_frobenius<F2, 2>(m, t);
    fq12_mul<F2>(m, m, t);
    // hard part: m^((x - 1)^2 (x + q) (x^2 + q^2 - 1) + 3); in the cyclotomic subgroup the inverse is the conjugate
    fq12_cyclotomic_exp_x<F2>(a, m);
    fq12_mul<F2>(a, a, fq12_conj<F2>(m));               // m^(x - 1)
    fq12_cyclotomic_exp_x<F2>(t, a);
    fq12_mul<F2>(a, t, fq12_conj<F2>(a));               // m^((x - 1)^2)
    fq12_cyclotomic_exp_x<F2>(b, a);
    fq12_frobenius<F2, 1>(t, a);
    fq12_mul<F2>(b, b, t);                              // ^(x + q)
    fq12_cyclotomic_exp_x<F2>(c, b);
    fq12_cyclotomic_exp_x<F2>(c, c);
    fq12_frobenius<F2, 2>(t, b);
    fq12_mul<F2>(c, c, t);
    fq12_mul<F2>(c, c, fq12_conj<F2>(b));               // ^(x^2 + q^2 - 1)
    fq12_cyclotomic_sqr<F2>(t, m);
    fq12_mul<F2>(t, t, m);                              // m^3
    fq12_mul<F2>(r, c, t);
}

// FE(prod_j ML(p[j], q[j])), j < pairs
template <class F2> ZK_PAIR_FN void pairing_product(Fq12<F2>& r, const Affine<typename F2::B>* p, const Affine<F2>* q, size_t pairs) {
    Fq12<F2> acc = fq12_one<F2>(), f;
    for (size_t j = 0; j < pairs; j++) {
        miller_loop<F2>(f, p[j], q[j]);
        fq12_mul<F2>(acc, acc, f);
    }
    final_exponentiation<F2>(r, acc);
}

// ---- packed form: the 144 words of the six Fq2Field coefficients in tower order, internal form -- what k_miller writes, what the
// finish kernel's `want` and zk_pk::e_alpha_beta hold.  On the host an Fq12 is kept over Fq264Field. -----------------------------------
inline Fq12<Fq264Field> fq12_host_from_packed(const uint32_t* w144) {
    Fq12<Fq264Field> f;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) f.c[i].c[j] = Fq264Field::from_dev(Fq2Field::load(w144 + 24 * (3 * i + j)));
    return f;
}
inline void fq12_host_to_packed(uint32_t* w144, const Fq12<Fq264Field>& f) {
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) Fq2Field::store(w144 + 24 * (3 * i + j), Fq264Field::to_dev(f.c[i].c[j]));
}

}  // namespace zk

