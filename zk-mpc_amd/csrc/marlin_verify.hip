// marlin_verify.hip -- Marlin::verify: one proof on the host (zk_marlin_verify_host), a batch on the device (zk_marlin_verify_batch), a
// batch as ONE folded KZG check on the host and on the device (zk_marlin_verify_aggregate*).
//
// Replaces (reference):
//   Marlin::verify                                   arkworks/marlin/src/lib.rs:324-442
//   Proof::deserialize                               marlin/src/data_structures.rs:99-110 (points through GroupAffine::deserialize:
//                                                    canonical, on the curve, in the prime-order subgroup)
//   AHPForR1CS::verifier_*_round, verifier_query_set, construct_linear_combinations   ahp/verifier.rs:42-170, ahp/mod.rs:112-290
//   MarlinKZG10::check_combinations, accumulate_commitments_and_values, KZG10::check  poly-commit/src/marlin/mod.rs:309-420,
//                                                    marlin_pc/mod.rs:342-400, kzg10/mod.rs:320-343
// One equation builder, two back ends.  parse_proof reads the bytes (structure, canonical scalars and abscissae); build_equations
// re-derives the challenges (marlin_transcript.hpp: the provers' transcript) and turns (key, input, proof) into two lists of terms (point reference, Fr scalar), one per query point:
//   L_q = sum_j xi^j (combination j of the commitments)  -  val_q g  -  random_v_q gamma_g  +  z_q W_q        (z = beta, gamma)
// and the proof holds iff e(L_q, h) e(W_q, -beta_h) = 1 for both -- KZG10::check with the witness term moved to the left, so that G2
// only ever sees the key's two points.  The two query points are NOT folded by a random coefficient (kzg10::batch_check takes an rng)
// -- except by the aggregate forms, which are that batch_check over every equation of a batch with the caller's coefficients:
// zk_marlin_verify_aggregate_host on the host, zk_marlin_verify_aggregate_coeffs / zk_marlin_verify_aggregate with the two sums on
// the device (g1_term_fold.hip for the long one, k_g1_scale_fold for the witnesses; sizes from marlin_agg_plan.hpp) and the pairing
// of the two sums on the host.
// The host back end evaluates the terms with host64_scalar_mul and pairing.cuh over Fq264Field; the device back end is
// g1_lincomb.hip (one wave per proof) followed by pairing.hip's kernels as they are.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "groth16_int.hpp"
#include "hostfield64.hpp"
#include "hostgroup.hpp"
#include "internal.hpp"
#include "marlin_agg_plan.hpp"
#include "marlin_lc.hpp"
#include "marlin_transcript.hpp"
#include "pairing.cuh"
#include <chrono>
#include <string.h>
#include <vector>

using namespace zk;

namespace {

using H2 = Fq264Field;
constexpr size_t IVK_COMM = 2 * 97 + 1, IVK_LEN = 24 + 12 * IVK_COMM;      // marlin_pc::Commitment::write: comm | bool | shifted_comm

// the points an equation refers to: the key's sixteen, then the proof's thirteen
enum KeyPoint : uint32_t { KP_INDEX = 0 /* 12: a_row, a_col, a_val, a_row_col, b_.., c_.. */, KP_G = 12, KP_GAMMA_G, KP_SHIFT_H, KP_SHIFT_K, N_KEY_POINTS };
enum ProofPoint : uint32_t { PP_W, PP_Z_A, PP_Z_B, PP_MASK, PP_T, PP_G_1, PP_H_1, PP_G_2, PP_H_2, PP_G_1_SHIFTED, PP_G_2_SHIFTED, PP_WIT_BETA, PP_WIT_GAMMA, N_PROOF_POINTS };
enum Eval : int { E_A_DENOM, E_B_DENOM, E_C_DENOM, E_G_1, E_G_2, E_T, E_Z_B, N_EVALS };      // the proof's order (sorted labels)
constexpr int ROUND_LEN[3] = {4, 3, 2};
constexpr size_t MAX_INPUTS = (size_t)1 << 24;

struct Key {
    const uint8_t* ivk;
    size_t num_constraints, num_non_zero;
    Affine<G1Field> pts[N_KEY_POINTS];
    Affine<G2Field> h, neg_beta_h;
};

bool bytes_below_q(const uint8_t b[48], uint8_t top_mask) {           // little-endian, the flag bits of the last byte masked away
    uint64_t l[6];
    uint8_t t[48];
    memcpy(t, b, 48);
    t[47] &= top_mask;
    memcpy(l, t, 48);
    return host64::cmp(l, host64::P) < 0;
}
Fq fq_from_canonical_bytes(const uint8_t b[48]) {
    uint32_t w[12];
    memcpy(w, b, 48);
    return fp_canon_to_int<FqParams>(fp_unpack<FqParams>(w));
}
bool on_curve_g1(const Affine<G1Field>& p) {
    using F = G1Field;
    return F::eq(F::sqr(p.y), F::add(F::mul(F::sqr(p.x), p.x), F::one()));
}
bool on_curve_g2(const Affine<G2Field>& p) {
    const Affine<H2> a = aff_to_host64<G2Field>(p);
    return H2::eq(H2::sqr(a.y), H2::add(H2::mul(H2::sqr(a.x), a.x), Host64Curve<H2>::b()));
}

// what is wrong with the CALL (ZK_ERR_ARG): the key as the struct gives it
bool load_key(const zk_marlin_vk_host* vk, Key* k) {
    if (!vk || !vk->ivk_bytes || vk->ivk_len != IVK_LEN) return false;
    k->ivk = vk->ivk_bytes;
    uint64_t info[3];
    memcpy(info, vk->ivk_bytes, 24);
    k->num_constraints = info[1];
    k->num_non_zero = info[2];
    if (!info[1] || !info[2] || info[1] > ((uint64_t)1 << 40) || info[2] > ((uint64_t)1 << 40)) return false;
    for (int i = 0; i < 12; i++) {
        const uint8_t* c = vk->ivk_bytes + 24 + i * IVK_COMM;
        // comm (x | y | infinity = 0), no shifted commitment: false, then GroupAffine::zero() = (0, 1, infinity = 1)
        if (c[96] != 0 || c[97] != 0 || c[97 + 1 + 96] != 1 || c[98 + 48] != 1) return false;
        for (int j = 0; j < 96; j++)
            if (c[98 + j] != 0 && j != 48) return false;
        if (!bytes_below_q(c, 0xff) || !bytes_below_q(c + 48, 0xff)) return false;
        k->pts[KP_INDEX + i] = Affine<G1Field>{fq_from_canonical_bytes(c), fq_from_canonical_bytes(c + 48)};
    }
    const zk_g1_affine* g1s[4] = {&vk->g, &vk->gamma_g, &vk->shift_h, &vk->shift_k};
    for (int i = 0; i < 4; i++) {
        if (!zk_words_below_q((const uint64_t*)g1s[i], 2)) return false;
        k->pts[KP_G + i] = host_aff_from_abi<G1Field>((const uint64_t*)g1s[i]);
    }
    for (int i = 0; i < (int)N_KEY_POINTS; i++)
        if (aff_is_inf<G1Field>(k->pts[i]) || !on_curve_g1(k->pts[i])) return false;
    if (!zk_words_below_q((const uint64_t*)&vk->h, 4) || !zk_words_below_q((const uint64_t*)&vk->beta_h, 4)) return false;
    k->h = host_aff_from_abi<G2Field>((const uint64_t*)&vk->h);
    const Affine<G2Field> bh = host_aff_from_abi<G2Field>((const uint64_t*)&vk->beta_h);
    if (aff_is_inf<G2Field>(k->h) || aff_is_inf<G2Field>(bh) || !on_curve_g2(k->h) || !on_curve_g2(bh)) return false;
    k->neg_beta_h = aff_neg<G2Field>(bh);
    return true;
}

// the formatted public input 1 | inputs | zeros up to the domain's size (lib.rs:335-345); false: an input not below r
bool load_input(const zk_fr* inputs, size_t n_inputs, std::vector<HF>* x) {
    const Dom X(n_inputs + 1);
    x->assign(X.size, HF::zero());
    (*x)[0] = HF::one();
    for (size_t i = 0; i < n_inputs; i++) {
        if (!zk_fr_words_valid(inputs[i].l)) return false;
        (*x)[i + 1] = HF::from_abi(inputs[i]);
    }
    return true;
}

// ---- the proof's bytes --------------------------------------------------------------------------------------------------------
struct Parsed {
    bool ok = false;                                // the structure, canonical scalars, canonical abscissae and flag bits
    const uint8_t* pt[N_PROOF_POINTS] = {};         // 48 compressed bytes each
    const uint8_t* ev_bytes = nullptr;              // 7 x 32, as absorbed
    HF ev[N_EVALS];
    bool has_rv[2] = {false, false};
    HF rv[2];
};
bool fr_from_canonical_bytes(const uint8_t* b, HF* out) {
    uint64_t l[4];
    memcpy(l, b, 32);
    if (!zk_fr_words_valid(l)) return false;
    uint32_t w[8];
    memcpy(w, b, 32);
    *out = HF{fp_canon_to_int<FrParams>(fp_unpack<FrParams>(w))};
    return true;
}
// GroupAffine::deserialize up to the curve: the infinity flag stands alone over an all-zero x, else x is below q
bool point_bytes_canonical(const uint8_t b[48]) {
    if (b[47] & 0x40) {
        if (b[47] != 0x40) return false;
        for (int i = 0; i < 47; i++) if (b[i]) return false;
        return true;
    }
    return bytes_below_q(b, 0x3f);
}
Parsed parse_proof(const uint8_t* p, size_t len) {
    Parsed r;
    size_t pos = 0;
    auto take = [&](size_t n) -> const uint8_t* {
        if (len - pos < n) return nullptr;
        const uint8_t* o = p + pos;
        pos += n;
        return o;
    };
    auto u64_is = [&](uint64_t want) {
        const uint8_t* b = take(8);
        uint64_t v;
        if (!b) return false;
        memcpy(&v, b, 8);
        return v == want;
    };
    auto point = [&](uint32_t which) {
        const uint8_t* b = take(48);
        if (!b || !point_bytes_canonical(b)) return false;
        r.pt[which] = b;
        return true;
    };
    if (!u64_is(3)) return r;
    uint32_t o = 0;
    for (int rnd = 0; rnd < 3; rnd++) {
        if (!u64_is((uint64_t)ROUND_LEN[rnd])) return r;
        for (int i = 0; i < ROUND_LEN[rnd]; i++, o++) {
            if (!point(o)) return r;
            const uint8_t* has = take(1);
            // a shifted commitment exactly where the key has a degree bound: g_1, g_2
            if (!has || *has > 1 || (*has == 1) != (o == PP_G_1 || o == PP_G_2)) return r;
            if (*has && !point(o == PP_G_1 ? PP_G_1_SHIFTED : PP_G_2_SHIFTED)) return r;
        }
    }
    if (!u64_is(N_EVALS)) return r;
    if (!(r.ev_bytes = take(32 * N_EVALS))) return r;
    for (int i = 0; i < N_EVALS; i++)
        if (!fr_from_canonical_bytes(r.ev_bytes + 32 * i, &r.ev[i])) return r;
    if (!u64_is(3)) return r;
    const uint8_t* msgs = take(3);                                     // three EmptyMessage: Option::None each
    if (!msgs || msgs[0] || msgs[1] || msgs[2]) return r;
    if (!u64_is(2)) return r;
    for (int q = 0; q < 2; q++) {
        if (!point(PP_WIT_BETA + q)) return r;
        const uint8_t* has = take(1);
        if (!has || *has > 1) return r;
        r.has_rv[q] = *has == 1;
        if (r.has_rv[q]) {
            const uint8_t* b = take(32);
            if (!b || !fr_from_canonical_bytes(b, &r.rv[q])) return r;
        }
    }
    const uint8_t* evals = take(1);                                    // BatchLCProof.evals = None, then the end
    if (!evals || *evals || pos != len) return r;
    r.ok = true;
    return r;
}

// ---- the equations ------------------------------------------------------------------------------------------------------------
struct Term { uint32_t point; uint32_t k[8]; };     // point: a KeyPoint, or N_KEY_POINTS + a ProofPoint; k: the plain integer below r
struct Equations { std::vector<Term> q[2]; };       // at beta, at gamma

// pts: the proof's thirteen points, decompressed (by either back end).  x: load_input's.
Equations build_equations(const Key& key, const std::vector<HF>& x, const Parsed& pr, const Affine<G1Field>* pts) {
    const Dom H(key.num_constraints), K(key.num_non_zero), X(x.size());
    marlin::Transcript fs(key.ivk, IVK_LEN, x);
    Comm comms[PP_H_2 + 1];                                             // the nine commitments, a shifted one where the key has a degree bound
    for (uint32_t o = PP_W; o <= PP_H_2; o++) {
        comms[o].c = pts[o];
        comms[o].has_shift = o == PP_G_1 || o == PP_G_2;
        comms[o].s = comms[o].has_shift ? pts[o == PP_G_1 ? PP_G_1_SHIFTED : PP_G_2_SHIFTED] : aff_inf<G1Field>();
    }
    MarlinLcIn in;
    const marlin::Transcript::Round1 r1 = fs.round1(&comms[PP_W], ROUND_LEN[0], H);
    in.alpha = r1.alpha;
    for (int m = 0; m < 3; m++) in.eta[m] = r1.eta[m];
    in.beta = fs.round2(&comms[PP_T], ROUND_LEN[1], H);
    in.gamma = fs.round3(&comms[PP_G_2], ROUND_LEN[2]);
    const HF xi = fs.evaluations(pr.ev_bytes, 32 * N_EVALS);
    in.z_b_beta = pr.ev[E_Z_B]; in.t_beta = pr.ev[E_T]; in.g_1_beta = pr.ev[E_G_1]; in.g_2_gamma = pr.ev[E_G_2];
    for (int m = 0; m < 3; m++) in.d[m] = pr.ev[E_A_DENOM + m];
    in.x = x.data();
    const MarlinLc c = marlin_lc(H, K, X, in);

    Equations eq;
    const HF one = HF::one();
    auto term = [](std::vector<Term>& v, uint32_t point, const HF& k) {
        Term t;
        t.point = point;
        k.canon_words(t.k);
        v.push_back(t);
    };
    auto pp = [](uint32_t o) { return (uint32_t)N_KEY_POINTS + o; };
    // a combination's constant terms move into its value (marlin/mod.rs:343-350); a degree-bounded oracle queried alone takes a
    // second power of xi with shifted - v shift_power (marlin_pc/mod.rs:359-383)
    {   // beta: g_1, outer_sumcheck, t, z_b
        std::vector<Term>& v = eq.q[0];
        HF cj = one, val = HF::zero();
        term(v, pp(PP_G_1), cj); val = val + pr.ev[E_G_1] * cj; cj = cj * xi;
        term(v, pp(PP_G_1_SHIFTED), cj); term(v, KP_SHIFT_H, (pr.ev[E_G_1] * cj).neg()); cj = cj * xi;
        term(v, pp(PP_MASK), cj); term(v, pp(PP_Z_A), c.z_a * cj); term(v, pp(PP_W), c.w * cj); term(v, pp(PP_H_1), c.h_1 * cj);
        val = val + (c.outer_c_zb + c.outer_c_x + c.outer_c_g1).neg() * cj; cj = cj * xi;
        term(v, pp(PP_T), cj); val = val + pr.ev[E_T] * cj; cj = cj * xi;
        term(v, pp(PP_Z_B), cj); val = val + pr.ev[E_Z_B] * cj;
        term(v, KP_G, val.neg());
        if (pr.has_rv[0]) term(v, KP_GAMMA_G, pr.rv[0].neg());
        term(v, pp(PP_WIT_BETA), in.beta);
    }
    {   // gamma: a_denom, b_denom, c_denom, g_2, inner_sumcheck
        std::vector<Term>& v = eq.q[1];
        HF cj = one, val = HF::zero();
        for (uint32_t m = 0; m < 3; m++) {
            term(v, KP_INDEX + 4 * m + 0, (in.alpha * cj).neg()); term(v, KP_INDEX + 4 * m + 1, (in.beta * cj).neg()); term(v, KP_INDEX + 4 * m + 3, cj);
            val = val + (in.d[m] - c.ba) * cj; cj = cj * xi;
        }
        term(v, pp(PP_G_2), cj); val = val + pr.ev[E_G_2] * cj; cj = cj * xi;
        term(v, pp(PP_G_2_SHIFTED), cj); term(v, KP_SHIFT_K, (pr.ev[E_G_2] * cj).neg()); cj = cj * xi;
        for (uint32_t m = 0; m < 3; m++) term(v, KP_INDEX + 4 * m + 2, c.val[m] * cj);
        term(v, pp(PP_H_2), c.h_2 * cj);
        val = val + c.inner_c.neg() * cj;
        term(v, KP_G, val.neg());
        if (pr.has_rv[1]) term(v, KP_GAMMA_G, pr.rv[1].neg());
        term(v, pp(PP_WIT_GAMMA), in.gamma);
    }
    return eq;
}

void r_words(uint32_t w[8]) { fp_pack<FrParams>(w, fp_const<FrParams>(FrParams::P)); }      // r itself, for the subgroup test

// proof k of a batch: its Miller pairs (L_beta, h), (W_beta, -beta_h), (L_gamma, h), (W_gamma, -beta_h), and per PRODUCT the flag
// that voids it: the host's structural verdict, a point off the curve, a point outside the subgroup (r P != O)
__global__ void __launch_bounds__(64) k_marlin_pairs(size_t count, const uint32_t* __restrict__ lc_out, const uint32_t* __restrict__ lc_inf,
                                                     const uint32_t* __restrict__ pts, const uint32_t* __restrict__ g2, const uint32_t* __restrict__ host_bad,
                                                     const uint32_t* __restrict__ bad_pt, uint32_t* __restrict__ P, uint32_t* __restrict__ Q,
                                                     uint32_t* __restrict__ bad) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= count) return;
    constexpr size_t SEGS = 2 + N_PROOF_POINTS;
    const Affine<G2Field> h = aff_load16<G2Field>(g2, 0), nbh = aff_load16<G2Field>(g2, 1);
    for (int q = 0; q < 2; q++) {
        aff_store16<G1Field>(P, 4 * k + 2 * q, aff_load16<G1Field>(lc_out, SEGS * k + q));
        aff_store16<G1Field>(P, 4 * k + 2 * q + 1, aff_load16<G1Field>(pts, N_KEY_POINTS + N_PROOF_POINTS * k + PP_WIT_BETA + q));
        aff_store16<G2Field>(Q, 4 * k + 2 * q, h);
        aff_store16<G2Field>(Q, 4 * k + 2 * q + 1, nbh);
    }
    uint32_t b = host_bad[k];
    for (size_t i = 0; i < N_PROOF_POINTS; i++) b |= bad_pt[N_PROOF_POINTS * k + i] | (lc_inf[SEGS * k + 2 + i] ? 0u : 1u);
    bad[2 * k] = bad[2 * k + 1] = b ? 1u : 0u;
}

// ---- folded, on the host ------------------------------------------------------------------------------------------------------------------
// KZG10::batch_check (poly-commit/src/kzg10/mod.rs:345) over the 2 count opening equations: with rho_{k,q} = coeffs[2 (2 k + q) ..]
// (128 bits)
//     e( sum rho_{k,q} L_{k,q}, h ) . e( sum rho_{k,q} W_{k,q}, -beta_h ) = 1.
// The first sum point by point: a proof's point occurs in ONE of its two term lists (fold_proof adds, so a builder that listed one
// twice would still be right) and gets one full-width scalar rho c mod r; the key's sixteen occur in every proof's and get one scalar
// each, summed over the batch: 13 count + 16 multiplications through the endomorphism (every point is in the subgroup by then).
void fold_proof(const Equations& eq, const uint64_t* coeffs4, HF proof_s[N_PROOF_POINTS], HF key_s[N_KEY_POINTS]) {
    for (size_t i = 0; i < N_PROOF_POINTS; i++) proof_s[i] = HF::zero();
    for (int q = 0; q < 2; q++) {
        const HF rho = HF::from_u128(coeffs4 + 2 * q);
        for (const Term& t : eq.q[q]) {
            HF& into = t.point < N_KEY_POINTS ? key_s[t.point] : proof_s[t.point - N_KEY_POINTS];
            into = into + rho * HF::from_canon_words(t.k);
        }
    }
}

// what both forms refuse (ZK_ERR_ARG), and the key and the formatted inputs they then work on
int agg_load(const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const size_t* offsets,
             const uint64_t* coeffs, const int* ok_all, Key* key, std::vector<std::vector<HF>>* xs) {
    if (!vk || !count || !proofs || !offsets || !coeffs || !ok_all || count > AGG_MAX_COUNT || (ninp && !inputs) || ninp > MAX_INPUTS) return ZK_ERR_ARG;
    for (size_t k = 0; k < count; k++)
        if (offsets[k + 1] < offsets[k]) return ZK_ERR_ARG;
    if (!load_key(vk, key)) return ZK_ERR_ARG;
    for (size_t i = 0; i < N_KEY_POINTS; i++)
        if (!zk_host_in_subgroup_g1(key->pts[i])) return ZK_ERR_ARG;      // (the endomorphism multiplies the key's points too)
    xs->resize(count);
    for (size_t k = 0; k < count; k++)
        if (!load_input(inputs + k * ninp, ninp, &(*xs)[k])) return ZK_ERR_ARG;
    return ZK_OK;
}
// every proof's structure; false: one does not parse
bool agg_parse(size_t count, const uint8_t* proofs, const size_t* offsets, std::vector<Parsed>* prs) {
    prs->resize(count);
    for (size_t k = 0; k < count; k++) {
        (*prs)[k] = parse_proof(proofs + offsets[k], offsets[k + 1] - offsets[k]);
        if (!(*prs)[k].ok) return false;
    }
    return true;
}
// the two sums through the pairing: the verdict and the folded value
void agg_finish(const Key& key, const XYZZ<Fq64Field>& L, const XYZZ<Fq64Field>& W, int* ok_all, zk_gt* folded) {
    using H1 = Fq64Field;
    const Affine<H1> p2[2] = {xyzz_to_affine<H1>(L), xyzz_to_affine<H1>(W)};
    const Affine<H2> q2[2] = {aff_to_host64<G2Field>(key.h), aff_to_host64<G2Field>(key.neg_beta_h)};
    Fq12<H2> e;
    pairing_product<H2>(e, p2, q2, 2);
    *ok_all = fq12_eq<H2>(e, fq12_one<H2>()) ? 1 : 0;
    if (folded) zk_host_gt_out(folded, e);
}

int aggregate_host(const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const size_t* offsets,
                   const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    using H1 = Fq64Field;
    Key key;
    std::vector<std::vector<HF>> xs;
    ZK_TRY(agg_load(vk, count, inputs, ninp, proofs, offsets, coeffs, ok_all, &key, &xs));
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);
    // every proof's structure and points first: a rejection there ends the call before any multiplication, folded all-zero
    std::vector<Parsed> prs;
    if (!agg_parse(count, proofs, offsets, &prs)) return ZK_OK;
    std::vector<Affine<G1Field>> pts(count * N_PROOF_POINTS);
    for (size_t k = 0; k < count; k++)
        for (size_t i = 0; i < N_PROOF_POINTS; i++) {
            Affine<G1Field>& p = pts[k * N_PROOF_POINTS + i];
            if (!zk_host_decompress_g1(prs[k].pt[i], &p) || !zk_host_in_subgroup_g1(p)) return ZK_OK;
        }
    HF key_s[N_KEY_POINTS];
    for (HF& s : key_s) s = HF::zero();
    XYZZ<H1> L = xyzz_inf<H1>(), W = xyzz_inf<H1>();
    auto mul = [](const Affine<G1Field>& p, const HF& s) {
        uint32_t k[8];
        s.canon_words(k);
        return host64_scalar_mul_glv(xyzz_from_affine<H1>(aff_to_host64<G1Field>(p)), k);
    };
    for (size_t k = 0; k < count; k++) {
        const Affine<G1Field>* pk = &pts[k * N_PROOF_POINTS];
        HF proof_s[N_PROOF_POINTS];
        fold_proof(build_equations(key, xs[k], prs[k], pk), coeffs + 4 * k, proof_s, key_s);
        for (size_t i = 0; i < N_PROOF_POINTS; i++) L = xyzz_add<H1>(L, mul(pk[i], proof_s[i]));
        for (int q = 0; q < 2; q++) {
            const uint64_t* c = coeffs + 4 * k + 2 * q;
            const uint32_t kw[8] = {(uint32_t)c[0], (uint32_t)(c[0] >> 32), (uint32_t)c[1], (uint32_t)(c[1] >> 32), 0, 0, 0, 0};
            W = xyzz_add<H1>(W, host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(pk[PP_WIT_BETA + q])), kw));
        }
    }
    for (size_t i = 0; i < N_KEY_POINTS; i++) L = xyzz_add<H1>(L, mul(key.pts[i], key_s[i]));
    agg_finish(key, L, W, ok_all, folded);
    return ZK_OK;
}

// ---- folded, on the device ------------------------------------------------------------------------------------------------------------
// The same check with the two sums on the device; every size from marlin_agg_plan.hpp (lane = point: a proof's eleven commitment points,
// then every proof's two witnesses side by side, then the key's sixteen).  The host keeps what it is better at: the structure, the
// transcripts and scalars (on the context's helper threads, split as zk_marlin_verify_batch splits them) and the pairing of the two
// sums -- two Miller lanes and one final exponentiation are a fraction of a millisecond in 64-bit limbs and tens of milliseconds on
// one lane of the device, and `folded` comes out of the very code the host form ends in.
// mode: which instantiation of k_g1_term_fold takes the long sum (ZK_TERM_GLV splits every scalar with host64_glv_split first).
void term_words(int mode, const HF& s, uint32_t out[8]) {
    if (mode != ZK_TERM_GLV) { s.canon_words(out); return; }
    uint32_t k[8], k1[8], k2[8];
    s.canon_words(k);
    host64_glv_split(k, k1, k2);                                      // k < r: both halves below 2^127
    for (int i = 0; i < 4; i++) { out[i] = k1[i]; out[4 + i] = k2[i]; }
}

int aggregate_dev(zk_ctx* ctx, const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const size_t* offsets,
                  const uint64_t* coeffs, int* ok_all, zk_gt* folded, int mode) {
    using H1 = Fq64Field;
    static_assert(AGG_PROOF_POINTS == N_PROOF_POINTS && AGG_KEY_POINTS == N_KEY_POINTS && AGG_COMM_POINTS == PP_WIT_BETA && PP_WIT_GAMMA == PP_WIT_BETA + 1,
                  "marlin_agg_plan.hpp lays out other points than the equations name");
    constexpr size_t NP = N_PROOF_POINTS;
    if (!ctx) return ZK_ERR_ARG;
    Key key;
    std::vector<std::vector<HF>> xs;
    ZK_TRY(agg_load(vk, count, inputs, ninp, proofs, offsets, coeffs, ok_all, &key, &xs));
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);
    ZkHostLap lap{ctx, "marlin_verify_agg."};      // with zk_set_profiling: host wall-clock of a phase into "marlin_verify_agg.<phase>"
    const ZkMarlinAggPlan pl = zk_marlin_agg_plan(count);

    // 1. the bytes: structure on the host (a proof that does not parse ends the call), the 13 count compressed points to the device
    std::vector<Parsed> prs;
    if (!agg_parse(count, proofs, offsets, &prs)) return ZK_OK;
    std::vector<uint8_t> comp(pl.comp_bytes);
    for (size_t k = 0; k < count; k++)
        for (size_t i = 0; i < NP; i++) memcpy(&comp[pl.lane_of(k, i) * 48], prs[k].pt[i], 48);
    uint32_t key_w[N_KEY_POINTS * 24];
    for (size_t j = 0; j < N_KEY_POINTS; j++) aff_store<G1Field>(key_w + 24 * j, key.pts[j]);
    lap.lap("parse");
    uint8_t* d_comp;
    uint32_t *d_pts, *d_flag, *d_words, *d_coef, *tpart_a, *tpart_b, *wpart_a, *wpart_b;
    ZK_TRY(zk_scratch(ctx, "magg_comp", pl.comp_bytes, (void**)&d_comp));
    ZK_TRY(zk_scratch(ctx, "magg_pts", pl.pts_bytes, (void**)&d_pts));
    ZK_TRY(zk_scratch(ctx, "magg_flag", pl.flags_bytes, (void**)&d_flag));
    ZK_TRY(zk_scratch(ctx, "magg_words", pl.words_bytes, (void**)&d_words));
    ZK_TRY(zk_scratch(ctx, "magg_coef", pl.coef_bytes, (void**)&d_coef));
    ZK_TRY(zk_scratch(ctx, "term_part_a", pl.term.part_a * AGG_XYZZ_BYTES, (void**)&tpart_a));
    ZK_TRY(zk_scratch(ctx, "term_part_b", pl.term.part_b * AGG_XYZZ_BYTES, (void**)&tpart_b));
    ZK_TRY(zk_scratch(ctx, "magg_wpart_a", pl.wit.part_a * AGG_XYZZ_BYTES, (void**)&wpart_a));
    ZK_TRY(zk_scratch(ctx, "magg_wpart_b", pl.wit.part_b * AGG_XYZZ_BYTES, (void**)&wpart_b));
    hipStream_t st = ctx->stream;
    ZkPhaseTimer tm(ctx);
    ZK_HIP(ctx, hipMemcpyAsync(d_comp, comp.data(), pl.comp_bytes, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_pts + pl.key_first * 24, key_w, sizeof key_w, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_coef, coeffs, pl.coef_bytes, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemsetAsync(d_flag, 0, pl.flags_bytes, st));
    tm.begin("marlin_verify_agg.k_decompress");
    ZK_TRY(zk_decompress_launch(ctx, 1, (const uint32_t*)d_comp, pl.proof_lanes, d_pts, d_flag, nullptr));
    tm.end();
    // the subgroup tests ALWAYS (the key's sixteen were tested on the host): the fold's argument needs prime order, and so does ZK_TERM_GLV
    tm.begin("marlin_verify_agg.k_subgroup");
    ZK_TRY(zk_subgroup_launch(ctx, 1, d_pts, pl.proof_lanes, d_flag, nullptr));
    tm.end();
    // 2. the equations need the ordinates (the transcript absorbs x | y): back they come, with the verdict on the points
    std::vector<uint32_t> pts_w(pl.proof_lanes * 24);
    uint32_t bad = 0;
    ZK_HIP(ctx, hipMemcpyAsync(pts_w.data(), d_pts, pts_w.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(&bad, d_flag, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("decompress");
    if (bad) { tm.resolve(); return ZK_OK; }      // a point off the curve or outside the subgroup: ok_all = 0, folded all-zero
    // 3. sum rho W over the 2 count witnesses (adjacent in the buffer: coefficient 2 k + q meets its point), under the builders
    tm.begin("marlin_verify_agg.k_scale_fold");
    ZK_TRY(zk_g1_scale_fold_launch(ctx, d_pts + pl.wit_first * 24, 1, false, d_coef, pl.wit.lanes, nullptr, wpart_a));
    size_t m_wit = pl.wit.blocks;
    uint32_t* wpart;
    ZK_TRY(zk_g1_sum_down(ctx, wpart_a, wpart_b, &m_wit, &wpart));
    tm.end();
    // 4. the builders, in ranges over the helper threads as zk_marlin_verify_batch has them; a range sums the key's scalars for itself
    std::vector<uint32_t> words(pl.term.lanes * 8);
    const size_t parts = count >= 64 ? 8 : 1;
    std::vector<HF> key_part(parts * N_KEY_POINTS, HF::zero());
    auto build_range = [&](size_t part) {
        HF* key_s = &key_part[part * N_KEY_POINTS];
        for (size_t k = count * part / parts; k < count * (part + 1) / parts; k++) {
            Affine<G1Field> pts[NP];
            for (size_t i = 0; i < NP; i++) pts[i] = aff_load<G1Field>(&pts_w[pl.lane_of(k, i) * 24]);
            HF proof_s[NP];
            fold_proof(build_equations(key, xs[k], prs[k], pts), coeffs + 4 * k, proof_s, key_s);
            for (size_t i = 0; i < NP; i++) term_words(mode, proof_s[i], &words[8 * pl.lane_of(k, i)]);
        }
    };
    {
        std::vector<ZkTask<void>> tasks;
        for (size_t p = 1; p < parts; p++) tasks.push_back(zk_async(ctx, [&build_range, p] { build_range(p); }));
        build_range(0);
        for (auto& t : tasks) t.get();
    }
    for (size_t j = 0; j < N_KEY_POINTS; j++) {
        HF s = HF::zero();
        for (size_t p = 0; p < parts; p++) s = s + key_part[p * N_KEY_POINTS + j];
        term_words(mode, s, &words[8 * pl.key_lane(j)]);
    }
    lap.lap("build");
    // 5. the long sum: one term per lane over the 13 count + 16 points
    ZK_HIP(ctx, hipMemcpyAsync(d_words, words.data(), pl.words_bytes, hipMemcpyHostToDevice, st));
    tm.begin("marlin_verify_agg.k_term_fold");
    ZK_TRY(zk_g1_term_fold_launch(ctx, mode, d_pts, 1, d_words, pl.term.lanes, nullptr, tpart_a));
    size_t m_term = pl.term.blocks;
    uint32_t* tpart;
    ZK_TRY(zk_g1_sum_down(ctx, tpart_a, tpart_b, &m_term, &tpart));
    tm.end();
    if (m_term != pl.term.left || m_wit != pl.wit.left) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_verify_aggregate: a sum-down left another count than its plan");
    std::vector<uint32_t> h_t(m_term * XW), h_w(m_wit * XW);
    ZK_HIP(ctx, hipMemcpyAsync(h_t.data(), tpart, h_t.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(h_w.data(), wpart, h_w.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("device");
    // 6. the last (at most 64) partials of each sum and the pairing, in 64-bit limbs
    XYZZ<H1> L = xyzz_inf<H1>(), W = xyzz_inf<H1>();
    for (size_t i = 0; i < m_term; i++) L = xyzz_add<H1>(L, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_t[i * XW])));
    for (size_t i = 0; i < m_wit; i++) W = xyzz_add<H1>(W, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_w[i * XW])));
    agg_finish(key, L, W, ok_all, folded);
    lap.lap("host_pairing");
    tm.resolve();
    return ZK_OK;
}

}  // namespace

extern "C" int zk_marlin_verify_aggregate_host(const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs, size_t inputs_per_proof, const uint8_t* proofs,
                                               const size_t* offsets, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN_NOCTX
    return aggregate_host(vk, count, inputs, inputs_per_proof, proofs, offsets, coeffs, ok_all, folded);
    ZK_API_END
}

extern "C" int zk_marlin_verify_host(const zk_marlin_vk_host* vk, const zk_fr* inputs, size_t n_inputs, const uint8_t* proof, size_t proof_len, int* ok) {
    ZK_API_BEGIN_NOCTX
    if (!vk || !proof || !ok) return ZK_ERR_ARG;
    Key key;
    std::vector<HF> x;
    if (!load_key(vk, &key) || (n_inputs && !inputs) || n_inputs > MAX_INPUTS || !load_input(inputs, n_inputs, &x)) return ZK_ERR_ARG;
    *ok = 0;
    const Parsed pr = parse_proof(proof, proof_len);
    if (!pr.ok) return ZK_OK;
    using H1 = Fq64Field;
    Affine<G1Field> pts[N_PROOF_POINTS];
    uint32_t rw[8];
    r_words(rw);
    for (uint32_t i = 0; i < N_PROOF_POINTS; i++) {
        if (!zk_host_decompress_g1(pr.pt[i], &pts[i])) return ZK_OK;
        // the plain chain, not the endomorphism's: the point is not known to be in the subgroup yet
        if (!xyzz_is_inf<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(pts[i])), rw))) return ZK_OK;
    }
    const Equations eq = build_equations(key, x, pr, pts);
    const Affine<H2> q2[2] = {aff_to_host64<G2Field>(key.h), aff_to_host64<G2Field>(key.neg_beta_h)};
    for (int q = 0; q < 2; q++) {
        XYZZ<H1> L = xyzz_inf<H1>();
        for (const Term& t : eq.q[q]) {
            const Affine<G1Field>& p = t.point < N_KEY_POINTS ? key.pts[t.point] : pts[t.point - N_KEY_POINTS];
            L = xyzz_add<H1>(L, host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(p)), t.k));
        }
        const Affine<H1> p2[2] = {xyzz_to_affine<H1>(L), aff_to_host64<G1Field>(pts[PP_WIT_BETA + q])};
        Fq12<H2> e;
        pairing_product<H2>(e, p2, q2, 2);
        if (!fq12_eq<H2>(e, fq12_one<H2>())) return ZK_OK;
    }
    *ok = 1;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_marlin_verify_batch(zk_ctx* ctx, const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                      const uint8_t* proofs_host, const size_t* offsets, int* ok) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !vk || !count || !proofs_host || !offsets || !ok || count > ZK_PAIRING_MAX_LANES / 4) return ZK_ERR_ARG;
    for (size_t k = 0; k < count; k++)
        if (offsets[k + 1] < offsets[k]) return ZK_ERR_ARG;
    Key key;
    if (!load_key(vk, &key) || (inputs_per_proof && !inputs_host) || inputs_per_proof > MAX_INPUTS) return ZK_ERR_ARG;
    std::vector<std::vector<HF>> xs(count);
    for (size_t k = 0; k < count; k++)
        if (!load_input(inputs_host + k * inputs_per_proof, inputs_per_proof, &xs[k])) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_verify_batch: a public input is not below r");
    ZkHostLap lap{ctx, "marlin_verify."};         // with zk_set_profiling: host wall-clock of a phase into "marlin_verify.<phase>"

    // 1. the bytes: structure on the host, the 13 count compressed points to the device (a proof without them: infinity)
    constexpr size_t NP = N_PROOF_POINTS, SEGS = 2 + NP;
    std::vector<Parsed> prs(count);
    std::vector<uint8_t> comp(count * NP * 48, 0);
    std::vector<uint32_t> host_bad(count);
    for (size_t k = 0; k < count; k++) {
        prs[k] = parse_proof(proofs_host + offsets[k], offsets[k + 1] - offsets[k]);
        host_bad[k] = prs[k].ok ? 0u : 1u;
        for (size_t i = 0; i < NP; i++) {
            uint8_t* dst = &comp[(k * NP + i) * 48];
            if (prs[k].ok) memcpy(dst, prs[k].pt[i], 48); else dst[47] = 0x40;
        }
    }
    lap.lap("parse");
    const size_t n_pts = N_KEY_POINTS + NP * count, n_pairs = 4 * count;
    uint8_t* d_comp;
    uint32_t *d_pts, *d_flags, *d_g2, *d_idx, *d_k, *d_off, *d_lc, *d_lcinf, *P, *Q, *ml;
    ZK_TRY(zk_scratch(ctx, "mvfy_comp", comp.size(), (void**)&d_comp));
    ZK_TRY(zk_scratch(ctx, "mvfy_pts", n_pts * 96, (void**)&d_pts));
    // any | bad_pt (13 count) | host_bad (count) | bad (2 count) | ok (2 count)
    ZK_TRY(zk_scratch(ctx, "mvfy_flags", (1 + NP * count + count + 2 * count + 2 * count) * 4, (void**)&d_flags));
    ZK_TRY(zk_scratch(ctx, "mvfy_g2", 2 * 192 + FQ12_WORDS * 4, (void**)&d_g2));
    uint32_t *bad_any = d_flags, *bad_pt = d_flags + 1, *d_host_bad = bad_pt + NP * count, *bad = d_host_bad + count;
    int* d_ok = (int*)(bad + 2 * count);
    hipStream_t st = ctx->stream;
    ZkPhaseTimer tm(ctx);
    ZK_HIP(ctx, hipMemcpyAsync(d_comp, comp.data(), comp.size(), hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemsetAsync(bad_any, 0, 4, st));
    tm.begin("marlin_verify.k_decompress");
    ZK_TRY(zk_decompress_launch(ctx, 1, (const uint32_t*)d_comp, NP * count, d_pts + N_KEY_POINTS * 24, bad_any, bad_pt));
    tm.end();
    // 2. the equations need the ordinates (the transcript absorbs x | y): back they come, with the curve flags
    std::vector<uint32_t> pts_w(NP * count * 24), bad_pt_h(NP * count);
    ZK_HIP(ctx, hipMemcpyAsync(pts_w.data(), d_pts + N_KEY_POINTS * 24, pts_w.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(bad_pt_h.data(), bad_pt, bad_pt_h.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("decompress");
    // the builders: ~90 us per proof on one thread -- at count 1 024 that was 91 ms of a 160 ms call, in eight ranges over the
    // context's helper threads it is 12 ms of 60 - 80 (DESIGN 6 "Marlin verification", profiles/marlin_verify_batch*.jsonl); below 64
    // proofs they are under a millisecond beside 33 ms of kernels and stay on the calling thread.  The packing stays in order.
    std::vector<Equations> eqs(count);
    auto build_range = [&](size_t from, size_t to) {
        for (size_t k = from; k < to; k++) {
            bool good = prs[k].ok;
            for (size_t i = 0; i < NP && good; i++) good = bad_pt_h[k * NP + i] == 0;
            if (!good) continue;
            Affine<G1Field> pts[NP];
            for (size_t i = 0; i < NP; i++) pts[i] = aff_load<G1Field>(&pts_w[(k * NP + i) * 24]);
            eqs[k] = build_equations(key, xs[k], prs[k], pts);
        }
    };
    {
        const size_t parts = count >= 64 ? 8 : 1;
        std::vector<ZkTask<void>> tasks;
        for (size_t p = 1; p < parts; p++) tasks.push_back(zk_async(ctx, [&, p] { build_range(count * p / parts, count * (p + 1) / parts); }));
        build_range(0, count / parts);
        for (auto& t : tasks) t.get();
    }
    ZkLincombPack pk;
    uint32_t rw[8];
    r_words(rw);
    for (size_t k = 0; k < count; k++) {
        const Equations& eq = eqs[k];
        for (int q = 0; q < 2; q++) {
            std::vector<uint32_t> idx, ks;
            for (const Term& t : eq.q[q]) {
                idx.push_back(t.point < N_KEY_POINTS ? t.point : (uint32_t)(N_KEY_POINTS + NP * k + (t.point - N_KEY_POINTS)));
                ks.insert(ks.end(), t.k, t.k + 8);
            }
            if (!pk.add(idx.data(), ks.data(), idx.size())) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_verify_batch: an equation has more than 64 terms");
        }
        for (size_t i = 0; i < NP; i++) {                               // r P_i, to be infinity
            const uint32_t idx = (uint32_t)(N_KEY_POINTS + NP * k + i);
            pk.add(&idx, rw, 1);
        }
    }
    pk.finish();
    lap.lap("build");
    // 3. the key's constants, the term lists; combinations; pairs; pairings
    struct Consts { uint32_t g1[N_KEY_POINTS * 24]; uint32_t g2[2 * 48]; uint32_t one[FQ12_WORDS]; } cs;
    for (int i = 0; i < (int)N_KEY_POINTS; i++) aff_store<G1Field>(cs.g1 + 24 * i, key.pts[i]);
    aff_store<G2Field>(cs.g2, key.h);
    aff_store<G2Field>(cs.g2 + 48, key.neg_beta_h);
    fq12_host_to_packed(cs.one, fq12_one<H2>());      // pairs = 2 products against the Fq12 one (k_pairing_finish's `want`)
    ZK_TRY(zk_scratch(ctx, "mvfy_idx", pk.point_index.size() * 4, (void**)&d_idx));
    ZK_TRY(zk_scratch(ctx, "mvfy_k", pk.scalars.size() * 4, (void**)&d_k));
    ZK_TRY(zk_scratch(ctx, "mvfy_off", pk.seg_off.size() * 4, (void**)&d_off));
    ZK_TRY(zk_scratch(ctx, "mvfy_lc", SEGS * count * 96, (void**)&d_lc));
    ZK_TRY(zk_scratch(ctx, "mvfy_lcinf", SEGS * count * 4, (void**)&d_lcinf));
    ZK_TRY(zk_pair_scratch(ctx, n_pairs, &P, &Q, &ml));
    ZK_HIP(ctx, hipMemcpyAsync(d_pts, cs.g1, sizeof cs.g1, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_g2, cs.g2, sizeof cs.g2 + sizeof cs.one, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_host_bad, host_bad.data(), count * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_idx, pk.point_index.data(), pk.point_index.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_k, pk.scalars.data(), pk.scalars.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_off, pk.seg_off.data(), pk.seg_off.size() * 4, hipMemcpyHostToDevice, st));
    tm.begin("marlin_verify.k_lincomb");
    ZK_TRY(zk_g1_lincomb_launch(ctx, d_pts, n_pts, d_idx, d_k, d_off, SEGS * count, pk.lanes(), d_lc, d_lcinf));
    tm.end();
    tm.begin("marlin_verify.k_pairing");
    hipLaunchKernelGGL(k_marlin_pairs, zk_blocks64(count), 64, 0, st, count, (const uint32_t*)d_lc, (const uint32_t*)d_lcinf, (const uint32_t*)d_pts,
                       (const uint32_t*)d_g2, (const uint32_t*)d_host_bad, (const uint32_t*)bad_pt, P, Q, bad);
    ZK_HIP(ctx, hipGetLastError());
    ZK_TRY(zk_miller_launch(ctx, P, Q, n_pairs, ml));
    ZK_TRY(zk_pairing_finish_launch(ctx, ml, 2, 2 * count, nullptr, d_g2 + 2 * 48, bad, d_ok));
    tm.end();
    std::vector<int> ok2(2 * count);
    ZK_HIP(ctx, hipMemcpyAsync(ok2.data(), d_ok, 2 * count * sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    for (size_t k = 0; k < count; k++) ok[k] = (ok2[2 * k] && ok2[2 * k + 1]) ? 1 : 0;
    lap.lap("device");
    tm.resolve();
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_marlin_verify_aggregate_coeffs(zk_ctx* ctx, const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                 const uint8_t* proofs_host, const size_t* offsets, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    return aggregate_dev(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, offsets, coeffs, ok_all, folded, ZK_TERM_DEFAULT);
    ZK_API_END
}

extern "C" int zk_marlin_verify_aggregate(zk_ctx* ctx, const zk_marlin_vk_host* vk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                          const uint8_t* proofs_host, const size_t* offsets, const uint8_t seed[32], int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !seed || !count || count > AGG_MAX_COUNT) return ZK_ERR_ARG;
    std::vector<uint64_t> coeffs(4 * count);
    ZK_TRY(zk_verify_aggregate_coeffs_from_seed(seed, 2 * count, coeffs.data()));
    ZK_TRY(aggregate_dev(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, offsets, coeffs.data(), ok_all, nullptr, ZK_TERM_DEFAULT));
    if (!ok_each) return ZK_OK;
    if (*ok_all) {
        for (size_t k = 0; k < count; k++) ok_each[k] = 1;
        return ZK_OK;
    }
    return zk_marlin_verify_batch(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, offsets, ok_each);
    ZK_API_END
}
