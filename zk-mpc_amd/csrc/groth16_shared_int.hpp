// groth16_shared_int.hpp -- the host algebra of ONE collaborative proof (create_proof::<MpcPairingEngine, C>, src/groth16.rs:68-183, on
// shares), cut where a prover can schedule it: the single prover (groth16_shared.hip) runs these functions for its proof, the batch
// prover (groth16_shared_batch.hip) over ranges of proofs.  Every collaborative Groth16 proof of the library is these functions.
#pragma once
#include "groth16_int.hpp"
#include "sharednet.hpp"

namespace zk_shared {

using namespace zk;
using SH1 = Fq64Field;
using SH2 = Fq264Field;
using SX1 = XYZZ<SH1>;
using SX2 = XYZZ<SH2>;

// The key's points as the algebra takes them: delta as is; the public summands as shift() adds them -- on the leader only
struct Key {
    bool leader;
    SX1 delta1, a0, alpha_g1, b0_g1, beta_g1;
    SX2 delta2, b0_g2, beta_g2;
    Key(const zk_pk* pk, bool leader_) : leader(leader_) {
        auto pub1 = [&](const Affine<G1Field>& p) { return leader ? xyzz_from_affine<SH1>(aff_to_host64<G1Field>(p)) : xyzz_inf<SH1>(); };
        auto pub2 = [&](const Affine<G2Field>& p) { return leader ? xyzz_from_affine<SH2>(aff_to_host64<G2Field>(p)) : xyzz_inf<SH2>(); };
        delta1 = xyzz_from_affine<SH1>(aff_to_host64<G1Field>(pk->delta_g1));
        delta2 = xyzz_from_affine<SH2>(aff_to_host64<G2Field>(pk->delta_g2));
        a0 = pub1(pk->a0); alpha_g1 = pub1(pk->alpha_g1); b0_g1 = pub1(pk->b0_g1); beta_g1 = pub1(pk->beta_g1);
        b0_g2 = pub2(pk->b0_g2); beta_g2 = pub2(pk->beta_g2);
    }
};

// One proof's shares on the host, by lane (0 = share, 1 = MAC share under SPDZ)
struct Proof {
    const zk_fr *r[2], *s[2];
    uint32_t rw[2][8], sw[2][8];
    SX1 r_g1[2], s_g1[2];                  // delta r, delta s
    SX2 s_g2[2];                           // delta_2 s
    SX1 h_acc[2], l_acc[2], g_a[2], g1_b[2];
    SX2 g2_b[2];
};

inline void begin(int lanes, const zk_fr* const r[2], const zk_fr* const s[2], Proof* P) {
    for (int l = 0; l < lanes; l++) {
        P->r[l] = r[l]; P->s[l] = s[l];
        fr_abi_to_canon_words(r[l]->l, P->rw[l]);
        fr_abi_to_canon_words(s[l]->l, P->sw[l]);
    }
}
// public point x shared scalar: local host arithmetic (scale_pub_group, share/additive.rs:502-508); independent of each other and
// of the device work
inline void pre_r_g1(const Key& K, Proof* P, int l) { P->r_g1[l] = host64_scalar_mul<SH1>(K.delta1, P->rw[l]); }
inline void pre_s_g1(const Key& K, Proof* P, int l) { P->s_g1[l] = host64_scalar_mul<SH1>(K.delta1, P->sw[l]); }
inline void pre_s_g2(const Key& K, Proof* P, int l) { P->s_g2[l] = host64_scalar_mul<SH2>(K.delta2, P->sw[l]); }

// calculate_coeff (:185-201) on lane l's MSM sums (m1 = H, L, A, B in G1; m2 = B in G2), after the three pre terms of the lane
inline void coeff(const Key& K, Proof* P, int l, const zk_g1_projective m1[4], const zk_g2_projective& m2) {
    P->h_acc[l] = host64_proj_from_abi<SH1>((const uint64_t*)&m1[0]);
    P->l_acc[l] = host64_proj_from_abi<SH1>((const uint64_t*)&m1[1]);
    const SX1 a_acc = host64_proj_from_abi<SH1>((const uint64_t*)&m1[2]), b1_acc = host64_proj_from_abi<SH1>((const uint64_t*)&m1[3]);
    const SX2 b2_acc = host64_proj_from_abi<SH2>((const uint64_t*)&m2);
    P->g_a[l] = xyzz_add<SH1>(xyzz_add<SH1>(xyzz_add<SH1>(P->r_g1[l], K.a0), a_acc), K.alpha_g1);
    P->g1_b[l] = xyzz_add<SH1>(xyzz_add<SH1>(xyzz_add<SH1>(P->s_g1[l], K.b0_g1), b1_acc), K.beta_g1);
    P->g2_b[l] = xyzz_add<SH2>(xyzz_add<SH2>(xyzz_add<SH2>(P->s_g2[l], K.b0_g2), b2_acc), K.beta_g2);
}

inline zk_g1_projective abi1(const SX1& p) { zk_g1_projective o; host64_write_projective<SH1>(xyzz_to_affine<SH1>(p), (uint64_t*)&o); return o; }
inline zk_g2_projective abi2(const SX2& p) { zk_g2_projective o; host64_write_projective<SH2>(xyzz_to_affine<SH2>(p), (uint64_t*)&o); return o; }
inline SX1 point1(const zk_g1_projective& p) { return host64_proj_from_abi<SH1>((const uint64_t*)&p); }

// Lane l's items of the fused open: open(o + y) for o = s, r (y = the leader's 1: the dummy group triple; from_add_shared: mac = share),
// open(s + x) for the three scaled points (x = 0) and the reveal of B.  fr: 2 scalars, g1: 3 points, g2: 1 point.
inline void fused_items(const Key& K, const Proof& P, int l, zk_fr* fr, zk_g1_projective* g1, zk_g2_projective* g2) {
    const Fr y = K.leader ? fp_mul<FrParams>(fp_one<FrParams>(), fp_const<FrParams>(FrParams::INT_TO_EXT)) : fp_zero<FrParams>();
    auto plus_y = [&](const zk_fr* v) { zk_fr o; host_store_ext<FrParams>(o.l, fp_add<FrParams>(host_load_ext<FrParams>(v->l), y)); return o; };
    fr[0] = plus_y(P.s[l]); fr[1] = plus_y(P.r[l]);
    g1[0] = abi1(P.r_g1[l]); g1[1] = abi1(P.g_a[l]); g1[2] = abi1(P.g1_b[l]);
    g2[0] = abi2(P.g2_b[l]);
}

// the local part of GroupShare::scale behind its two opens: z - sx*y (+ sx*oy on the leader), z = 0, y = [leader]; both SPDZ
// lanes hold the same value (key 1)
inline SX1 scale_finish(bool leader, const SX1& sxp, const zk_fr& oy) {
    if (!leader) return xyzz_inf<SH1>();
    uint32_t kw[8];
    fr_abi_to_canon_words(oy.l, kw);
    return xyzz_add<SH1>(host64_scalar_mul<SH1>(sxp, kw), xyzz_neg<SH1>(sxp));
}
// s A + r B1 - r s delta from the three scaled points (:115, :140, :161)
inline SX1 scaled_sum(const SX1& rs_delta, const SX1& s_a, const SX1& r_b1) {
    return xyzz_add<SH1>(xyzz_add<SH1>(s_a, r_b1), xyzz_neg<SH1>(rs_delta));
}
// lane l's share of C (:169-174)
inline zk_g1_projective c_share(const Proof& P, int l, const SX1& t) { return abi1(xyzz_add<SH1>(xyzz_add<SH1>(t, P.l_acc[l]), P.h_acc[l])); }

// Proof::serialize of the opened A, B, C (opened points come normalised: zz = zzz = 1 or all zero, so x and y are the affine point)
inline void write_proof(const zk_g1_projective& a, const zk_g2_projective& b, const zk_g1_projective& c, uint8_t proof[192]) {
    const SX1 A = point1(a), C = point1(c);
    const SX2 B = host64_proj_from_abi<SH2>((const uint64_t*)&b);
    g1_serialize(aff_from_host64<G1Field>(Affine<SH1>{A.x, A.y}), proof);
    g2_serialize(aff_from_host64<G2Field>(Affine<SH2>{B.x, B.y}), proof + 48);
    g1_serialize(aff_from_host64<G1Field>(Affine<SH1>{C.x, C.y}), proof + 144);
}

}  // namespace zk_shared
