// groth16_verify_keys.hip -- Groth16 verification of a batch on the device and its folded form on the host, over ONE verifying key
// or SEVERAL in one call: proof by proof (zk_groth16_verify_batch, zk_groth16_vkey_verify_batch, zk_groth16_vkey_verify_prepared,
// zk_groth16_vkeys_verify_batch) and as ONE folded pairing product (zk_groth16_verify_aggregate, zk_groth16_vkey_verify_aggregate,
// zk_groth16_vkeys_verify_aggregate, their _coeffs forms and the two host forms).  There is one implementation of each form, written
// over zkvk::Plan (verify_keys_plan.hpp); the single-key entry points build the plan with one slot and the identity permutation.
//
// Replaces (reference): nothing it has as one call -- Groth16::verify is one proof of one key (arkworks/groth16/src/verifier.rs:13-61);
// its application proves several circuits per round, each with a key of its own, and verifies them one by one.  The fold is the one
// of its KZG verifier (poly-commit/src/kzg10/mod.rs:345, batch_check: a random linear combination of the equations, one product of
// pairings).  With 128-bit coefficients r_i and k(i) the key of proof i the batch holds iff
//     prod_i e(r_i A_i, B_i) . prod_k [ e(sum_{k(i)=k} r_i C_i, -delta_k) . e(sum_j s_{k,j} gamma_abc_k[j], -gamma_k) . e(s_{k,0} alpha_k, -beta_k) ] = 1
//     s_{k,0} = sum_{k(i)=k} r_i,   s_{k,j} = sum_{k(i)=k} r_i x_{i,j}   (mod r)
// count + 3 K' Miller loops (K' keys with a proof) and ONE final exponentiation (proof by proof: 3 count and count).  The value is the
// product over the keys of the one-key value on each key's proofs: the final exponentiation is multiplicative.
//
// The plan groups the proofs by key and lays out every launch; the checks of one key's arguments, the staging, the subgroup tests,
// prepare_inputs and r_i A_i (k_g1_scale_fold) are groth16_verify.hip's, the Miller launch and its product pairing.hip's; none of
// them asks about keys.  What is here:
//   k_g1_scale_fold_keyed   sum r_i C_i PER KEY: k_g1_scale_fold's term per lane (in grouped order, through the plan's permutation),
//                           then k_g1_lincomb's segmented tree -- but a key's segment may straddle waves, so a wave writes one XYZZ
//                           partial per piece of a segment it holds, tagged with the key's slot, and the kernel runs again on the
//                           partials (the tree alone) until no key has more than 64 left.  The launches depend on the longest
//                           segment alone; no launch per key, no atomics.  One key: one partial per wave, then the tree alone.
//   k_verify_layout         the proof-by-proof form's pairs in grouped order, -gamma and -delta from the proof's slot.
// The sum_k (ninp_k + 2) full-width multiplications of key points run on the helper threads under the device work or, for many, as
// one k_g1_lincomb launch (DESIGN 6 has the rule; ZK_VFY_KEYS_MUL=host|dev forces either).
// Argument checks and their words belong to the entry points; the forms take a plan that has been accepted, and the keys.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "g1_lincomb.cuh"
#include "groth16_int.hpp"
#include "groth16_verify_int.hpp"
#include "pairing.cuh"
#include "verify_keys_plan.hpp"
#include <stdlib.h>
#include <string.h>

using namespace zk;
using namespace zkvfy;

namespace {

using H1 = Fq64Field;
using H2 = Fq264Field;
constexpr size_t MAX_LANES = ZK_PAIRING_MAX_LANES;
constexpr size_t SCALE_LDS = (size_t)LINCOMB_TAB * XW * 64 * 4;      // the window tables: 98 304 bytes
constexpr size_t SUM_LDS = (size_t)XW * 64 * 4;                      // the tree alone: 12 288 bytes
// key multiplications in all from which the device takes them (DESIGN 6 "Several keys in one call")
constexpr size_t KEYS_MUL_DEV_FROM = 2048;

// ---- k_g1_scale_fold_keyed --------------------------------------------------------------------------------------------------------
// lane g < n holds term g of a level (verify_keys_plan.hpp): point (perm ? perm[g] : g) in_step of `in` (affine table form, or XYZZ
// with in_xyzz) times the 128-bit coeffs[4 (perm ? perm[g] : g) ..] (coeffs = NULL: times one, SUM_LDS bytes of LDS; else SCALE_LDS).
// seg_off / mis: n_seg + 1 words each.  Out: one XYZZ partial per piece and the piece's slot, at the plan's index.
__global__ void __launch_bounds__(64) k_g1_scale_fold_keyed(const uint32_t* __restrict__ in, uint32_t in_step, int in_xyzz, const uint32_t* __restrict__ perm,
                                                            const uint32_t* __restrict__ coeffs, const uint32_t* __restrict__ seg_off,
                                                            const uint32_t* __restrict__ mis, uint32_t n_seg, uint32_t n,
                                                            uint32_t* __restrict__ out_part, uint32_t* __restrict__ out_slot) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane;
    ZkLdsTab tab{lds + lane};
    XYZZ<G1Field> acc = xyzz_inf<G1Field>();
    zkvk::KeyedLane kl{n_seg, g, g + 1, 0};                            // a lane past the end: a piece of its own that nobody reads
    uint32_t src = g;
    if (g < n) {
        kl = zkvk::keyed_lane(seg_off, mis, n_seg, g);
        if (perm) src = perm[g];
    }
    if (coeffs) {
        Affine<G1Field> p = aff_inf<G1Field>();
        uint32_t k[4] = {0, 0, 0, 0};
        if (g < n) {
            p = aff_load16<G1Field>(in, (size_t)src * in_step);
            const uint4 c = reinterpret_cast<const uint4*>(coeffs)[src];
            k[0] = c.x; k[1] = c.y; k[2] = c.z; k[3] = c.w;
        }
        acc = lincomb_term<G1Field, ZkLdsTab, 4>(p, k, tab);
        __syncthreads();                                               // (the tree reuses entry 0 of the tables)
    } else if (g < n) {
        acc = in_xyzz ? xyzz_load16<G1Field>(in, (size_t)src * in_step) : xyzz_from_affine<G1Field>(aff_load16<G1Field>(in, (size_t)src * in_step));
    }
    // the segmented tree over the pieces: after step s the lane at offset 0 mod 2 s of its piece holds the sum of its 2 s lanes; a lane
    // reads lane + s only while that lies inside its own piece
    tab.put(0, acc);
#pragma unroll 1
    for (uint32_t s = 1; s < 64; s <<= 1) {
        __syncthreads();
        const bool act = (((g - kl.lo) & (2 * s - 1)) == 0) && g + s < kl.hi;
        if (act) {
            ZkLdsTab other{lds + lane + s};
            acc = xyzz_add<G1Field>(acc, other.get(0));
        }
        __syncthreads();
        if (act) tab.put(0, acc);
    }
    if (g < n && g == kl.lo) {
        xyzz_store16<G1Field>(out_part, kl.out, acc);
        out_slot[kl.out] = kl.slot;
    }
}

// ---- k_verify_layout ----------------------------------------------------------------------------------------------------------------
// grouped position g holds proof perm[g] (perm = NULL: proof g) of slot slot_of[g] (slot_of = NULL: slot 0): P[3 g ..] = A, prepared
// inputs, C;  Q[3 g ..] = B, -gamma, -delta of the slot (negs: -gamma | -delta per slot).  ac, b, bad_ac, bad_b are in the caller's
// order (stage_proofs: table form from the decompression, with their off-curve flags), prep in grouped order.
__global__ void __launch_bounds__(64) k_verify_layout(size_t count, const uint32_t* __restrict__ perm, const uint32_t* __restrict__ slot_of,
                                                      const uint32_t* __restrict__ prep, const uint32_t* __restrict__ ac, const uint32_t* __restrict__ b,
                                                      const uint32_t* __restrict__ negs, const uint32_t* __restrict__ bad_ac,
                                                      const uint32_t* __restrict__ bad_b, uint32_t* __restrict__ P, uint32_t* __restrict__ Q,
                                                      uint32_t* __restrict__ bad) {
    const size_t g = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (g >= count) return;
    const size_t i = perm ? perm[g] : g, s = slot_of ? slot_of[g] : 0;
    aff_store16<G1Field>(P, 3 * g, aff_load16<G1Field>(ac, 2 * i));
    aff_store16<G1Field>(P, 3 * g + 1, aff_load16<G1Field>(prep, g));
    aff_store16<G1Field>(P, 3 * g + 2, aff_load16<G1Field>(ac, 2 * i + 1));
    aff_store16<G2Field>(Q, 3 * g, aff_load16<G2Field>(b, i));
    aff_store16<G2Field>(Q, 3 * g + 1, aff_load16<G2Field>(negs, 2 * s));
    aff_store16<G2Field>(Q, 3 * g + 2, aff_load16<G2Field>(negs, 2 * s + 1));
    bad[g] = bad_ac[2 * i] | bad_ac[2 * i + 1] | bad_b[i];
}

// one level of the keyed sum, on ctx->stream, no wait
int keyed_launch(zk_ctx* ctx, const uint32_t* in, uint32_t in_step, bool in_xyzz, const uint32_t* perm, const uint32_t* coeffs, const uint32_t* meta,
                 size_t slots, size_t n, uint32_t* out_part, uint32_t* out_slot) {
    if (!ctx->lds_attr_done[ZK_LDS_SCALE_FOLD_KEYED]) {
        ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_g1_scale_fold_keyed, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCALE_LDS));
        ctx->lds_attr_done[ZK_LDS_SCALE_FOLD_KEYED] = true;
    }
    hipLaunchKernelGGL(k_g1_scale_fold_keyed, zk_blocks64(n), 64, coeffs ? SCALE_LDS : SUM_LDS, ctx->stream, in, in_step, in_xyzz ? 1 : 0, perm, coeffs, meta,
                       meta + (slots + 1), (uint32_t)slots, (uint32_t)n, out_part, out_slot);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// ---- arguments --------------------------------------------------------------------------------------------------------------------------
int plan_refusal(zk_ctx* ctx, zkvk::Refusal why, size_t bad, const uint32_t* key_of, size_t n_keys, size_t inputs_len, const char* entry) {
    const std::string e(entry);
    switch (why) {
        case zkvk::PLAN_OK: return ZK_OK;
        case zkvk::PLAN_EMPTY: ZK_FAIL(ctx, ZK_ERR_ARG, e + ": count = 0 or n_keys = 0");
        case zkvk::PLAN_KEY_OF:
            ZK_FAIL(ctx, ZK_ERR_ARG, e + ": key_of[" + std::to_string(bad) + "] = " + std::to_string(key_of[bad]) + " is not below n_keys = " + std::to_string(n_keys));
        case zkvk::PLAN_INPUTS_LEN:
            ZK_FAIL(ctx, ZK_ERR_ARG, e + ": inputs_len = " + std::to_string(inputs_len) + ", the proofs' keys take " + std::to_string(bad) + " public inputs");
        default: ZK_FAIL(ctx, ZK_ERR_ARG, e + ": more proofs or public inputs than one call takes");
    }
}
// what the device forms refuse of ONE key and its arguments, in the words of the entry point `entry` (a zk_pk without verifying-key
// parts is refused where its vkey is asked for: zk_pk_vkey), and the one-slot plan of what they accept
int one_key_args(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, size_t max_count,
                 const char* entry, zkvk::Plan* pl) {
    if (!ctx || !vk || !count || !proofs_host || count > max_count) return ZK_ERR_ARG;
    ZK_TRY(inputs_ok(ctx, vk, count, inputs_host, ninp, entry));
    size_t bad = 0;
    return zkvk::make_plan(1, count, nullptr, &ninp, count * ninp, pl, &bad) == zkvk::PLAN_OK ? ZK_OK : ZK_ERR_ARG;
}
// ... and of the folded forms beyond that
int one_key_fold_args(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, const int* ok_all,
                      const char* entry, zkvk::Plan* pl) {
    if (!ok_all || (ninp && !inputs_host)) return ZK_ERR_ARG;      // (silently, before inputs_ok words anything about ninp)
    return one_key_args(ctx, vk, count, inputs_host, ninp, proofs_host, MAX_LANES - 3, entry, pl);
}
// what every several-key device form refuses, and the plan of what it accepts
int keys_args(zk_ctx* ctx, const zk_vkey* const* vkeys, size_t n_keys, size_t count, const uint32_t* key_of, const zk_fr* inputs_host, size_t inputs_len,
              const uint8_t* proofs_host, const char* entry, zkvk::Plan* pl) {
    if (!ctx || !vkeys || !key_of || !proofs_host || (inputs_len && !inputs_host)) return ZK_ERR_ARG;
    if (!n_keys || !count) return plan_refusal(ctx, zkvk::PLAN_EMPTY, 0, key_of, n_keys, inputs_len, entry);
    std::vector<size_t> ninp(n_keys);
    for (size_t k = 0; k < n_keys; k++) {
        if (!vkeys[k]) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": vkeys[" + std::to_string(k) + "] is null");
        ninp[k] = vkeys[k]->ninp();
    }
    size_t bad = 0;
    const zkvk::Refusal why = zkvk::make_plan(n_keys, count, key_of, ninp.data(), inputs_len, pl, &bad);
    ZK_TRY(plan_refusal(ctx, why, bad, key_of, n_keys, inputs_len, entry));
    for (size_t i = 0; i < inputs_len; i++)
        if (!zk_fr_words_valid(inputs_host[i].l)) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": public input " + std::to_string(i) + " is not below r");
    return ZK_OK;
}
int lanes_refusal(zk_ctx* ctx, bool fits, const char* entry, const char* what) {
    if (!fits) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": " + what + " is above 2^22 Miller lanes");
    return ZK_OK;
}

// ---- the coefficient sums of every slot ---------------------------------------------------------------------------------------------
// S[soff[s] + j] += s_{k,j} of slot s (j <= ninp of its key), over the grouped positions [lo, hi) only
template <class NinpOf>
void slot_sums(const zkvk::Plan& pl, const NinpOf& ninp_of, const std::vector<size_t>& soff, const uint64_t* coeffs, const zk_fr* inputs, size_t lo, size_t hi,
               HF* S) {
    const size_t K = pl.slots();
    for (size_t s = zkvk::keyed_slot_of(pl.seg_off.data(), (uint32_t)K, (uint32_t)lo); s < K && pl.seg_off[s] < hi; s++) {
        const size_t n = ninp_of(s);
        HF* out = S + soff[s];
        for (size_t g = std::max<size_t>(lo, pl.seg_off[s]); g < std::min<size_t>(hi, pl.seg_off[s + 1]); g++) {
            const size_t i = pl.proof_at(g);
            const HF r = HF::from_u128(coeffs + 2 * i);      // lo + 2^64 hi
            out[0] = out[0] + r;
            for (size_t j = 0; j < n; j++) out[j + 1] = out[j + 1] + r * HF::from_abi(inputs[pl.in_off[i] + j]);
        }
    }
}

// ---- folded, on the host ----------------------------------------------------------------------------------------------------------------
// key_of = NULL: every proof under vks[0] (zk_groth16_verify_aggregate_host).  The lanes: the proofs in the caller's order, then
// delta, gamma, beta of every used key.
int aggregate_keys_host(const zk_vk_host* vks, size_t n_keys, size_t count, const uint32_t* key_of, const zk_fr* inputs, size_t inputs_len,
                        const uint8_t* proofs, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    if (!vks || !proofs || !coeffs || !ok_all || !n_keys || !count || (inputs_len && !inputs)) return ZK_ERR_ARG;
    std::vector<size_t> ninp(n_keys);
    for (size_t k = 0; k < n_keys; k++) ninp[k] = vks[k].gamma_abc_len ? vks[k].gamma_abc_len - 1 : 0;
    zkvk::Plan pl;
    size_t bad = 0;
    if (zkvk::make_plan(n_keys, count, key_of, ninp.data(), inputs_len, &pl, &bad) != zkvk::PLAN_OK || !pl.fold_fits()) return ZK_ERR_ARG;
    for (size_t s = 0; s < pl.slots(); s++)
        if (!zk_vk_host_ok(&vks[pl.used[s]], ninp[pl.used[s]])) return ZK_ERR_ARG;
    if (!inputs_below_r(inputs, inputs_len)) return ZK_ERR_ARG;
    const size_t K = pl.slots(), n = pl.fold_lanes();
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);
    std::vector<Affine<H1>> P(n);
    std::vector<Affine<H2>> Q(n);
    std::vector<XYZZ<H1>> c_sum(K, xyzz_inf<H1>());
    for (size_t s = 0; s < K; s++)
        for (size_t g = pl.seg_off[s]; g < pl.seg_off[s + 1]; g++) {
            const size_t i = pl.proof_at(g);
            Affine<G1Field> a, c;
            Affine<G2Field> b;
            if (!host_proof_points(proofs + i * 192, true, &a, &b, &c)) return ZK_OK;
            uint32_t k[8];
            coeff_words(coeffs + 2 * i, k);
            P[i] = xyzz_to_affine<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(a)), k));
            Q[i] = aff_to_host64<G2Field>(b);
            c_sum[s] = xyzz_add<H1>(c_sum[s], host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(c)), k));
        }
    std::vector<size_t> soff(K + 1, 0);
    for (size_t s = 0; s < K; s++) soff[s + 1] = soff[s] + ninp[pl.used[s]] + 1;
    std::vector<HF> S(soff[K], HF::zero());
    slot_sums(pl, [&](size_t s) { return ninp[pl.used[s]]; }, soff, coeffs, inputs, 0, count, S.data());
    for (size_t s = 0; s < K; s++) {
        const zk_vk_host* vk = &vks[pl.used[s]];
        XYZZ<H1> pi = xyzz_inf<H1>();
        uint32_t k[8];
        for (size_t j = 0; j <= ninp[pl.used[s]]; j++) {
            S[soff[s] + j].canon_words(k);
            pi = xyzz_add<H1>(pi, host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->gamma_abc_g1[j])), k));
        }
        S[soff[s]].canon_words(k);
        const size_t t = count + 3 * s;
        P[t] = xyzz_to_affine<H1>(c_sum[s]);
        Q[t] = aff_neg<H2>(zk_host_g2(&vk->delta_g2));
        P[t + 1] = xyzz_to_affine<H1>(pi);
        Q[t + 1] = aff_neg<H2>(zk_host_g2(&vk->gamma_g2));
        P[t + 2] = xyzz_to_affine<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->alpha_g1)), k));
        Q[t + 2] = aff_neg<H2>(zk_host_g2(&vk->beta_g2));
    }
    Fq12<H2> r;
    pairing_product<H2>(r, P.data(), Q.data(), n);
    *ok_all = fq12_eq<H2>(r, fq12_one<H2>()) ? 1 : 0;
    if (folded) zk_host_gt_out(folded, r);
    return ZK_OK;
}

// ---- the key multiplications ----------------------------------------------------------------------------------------------------------
// term t of slot s: j = t <= ninp: S[soff[s] + j] gamma_abc[j];  t = ninp + 1: S[soff[s]] alpha.  pi[s] = the sum of the first kind,
// al[s] the second.
bool keys_mul_on_device(const zkvk::Plan& pl) {
    const char* e = getenv("ZK_VFY_KEYS_MUL");
    if (e && !strcmp(e, "host")) return false;
    if (e && !strcmp(e, "dev")) return true;
    return pl.mul_terms >= KEYS_MUL_DEV_FROM;
}
void keys_mul_host(zk_ctx* ctx, const zk_vkey* const* vkeys, const zkvk::Plan& pl, const std::vector<size_t>& soff, const std::vector<HF>& S,
                   std::vector<XYZZ<H1>>* pi, std::vector<XYZZ<H1>>* al) {
    const size_t K = pl.slots();
    std::vector<size_t> toff(K + 1, 0);                                // terms in front of slot s
    for (size_t s = 0; s < K; s++) toff[s + 1] = toff[s] + vkeys[pl.used[s]]->ninp() + 2;
    std::vector<XYZZ<H1>> mul(toff[K]);
    zk_over_ranges(ctx, toff[K], 16, [&](size_t lo, size_t hi) {
        size_t s = 0;
        for (size_t t = lo; t < hi; t++) {
            while (toff[s + 1] <= t) s++;
            const zk_vkey* vk = vkeys[pl.used[s]];
            const size_t j = t - toff[s], ninp = vk->ninp();
            uint32_t k[8];
            S[soff[s] + (j <= ninp ? j : 0)].canon_words(k);
            const Affine<G1Field> p = j <= ninp ? aff_load<G1Field>(&vk->abc_host[24 * j]) : vk->alpha_g1;
            const XYZZ<H1> x = xyzz_from_affine<H1>(aff_to_host64<G1Field>(p));
            mul[t] = vk->points_in_subgroup ? host64_scalar_mul_glv(x, k) : host64_scalar_mul<H1>(x, k);
        }
    });
    for (size_t s = 0; s < K; s++) {
        const size_t ninp = vkeys[pl.used[s]]->ninp();
        XYZZ<H1> sum = xyzz_inf<H1>();
        for (size_t j = 0; j <= ninp; j++) sum = xyzz_add<H1>(sum, mul[toff[s] + j]);
        (*pi)[s] = sum;
        (*al)[s] = mul[toff[s] + ninp + 1];
    }
}
// The same as ONE k_g1_lincomb launch: the used keys' gamma_abc words and their alphas as one point array, a key's terms cut into
// segments of at most 64 (the kernel's wave) whose sums the host adds, alpha a segment of its own.  Enqueued on ctx->stream, no wait;
// the caller reads seg_slot.size() affine points back from *d_out and hands them to keys_mul_dev_collect.
struct KeysMulDev {
    std::vector<uint32_t> seg_slot;      // per segment: 2 slot (a piece of pi) or 2 slot + 1 (alpha)
    uint32_t* d_out = nullptr;
    std::vector<uint32_t> h_out;         // seg_slot.size() x 24 words, filled by the caller's copy
    std::vector<uint32_t> pts;           // what the uploads read: kept until the caller has waited for the stream
    ZkLincombPack pack;
};
int keys_mul_dev_launch(zk_ctx* ctx, const zk_vkey* const* vkeys, const zkvk::Plan& pl, const std::vector<size_t>& soff, const std::vector<HF>& S, KeysMulDev* km) {
    const size_t K = pl.slots();
    std::vector<uint32_t>& pts = km->pts;
    ZkLincombPack& pack = km->pack;
    std::vector<uint32_t> idx, k8;
    for (size_t s = 0; s < K; s++) {
        const zk_vkey* vk = vkeys[pl.used[s]];
        const size_t ninp = vk->ninp(), base = pts.size() / 24;
        pts.insert(pts.end(), vk->abc_host.begin(), vk->abc_host.begin() + 24 * (ninp + 1));
        pts.resize(pts.size() + 24);
        aff_store<G1Field>(&pts[pts.size() - 24], vk->alpha_g1);
        for (size_t j0 = 0; j0 <= ninp; j0 += LINCOMB_MAX_TERMS) {
            const size_t len = std::min<size_t>(LINCOMB_MAX_TERMS, ninp + 1 - j0);
            idx.resize(len);
            k8.resize(8 * len);
            for (size_t t = 0; t < len; t++) {
                idx[t] = (uint32_t)(base + j0 + t);
                S[soff[s] + j0 + t].canon_words(&k8[8 * t]);
            }
            if (!pack.add(idx.data(), k8.data(), len)) return ZK_ERR_STATE;
            km->seg_slot.push_back((uint32_t)(2 * s));
        }
        const uint32_t ia = (uint32_t)(base + ninp + 1);
        uint32_t ka[8];
        S[soff[s]].canon_words(ka);
        if (!pack.add(&ia, ka, 1)) return ZK_ERR_STATE;
        km->seg_slot.push_back((uint32_t)(2 * s + 1));
    }
    pack.finish();
    const size_t n_seg = km->seg_slot.size();
    uint32_t *d_pts, *d_idx, *d_k, *d_off, *d_inf;
    ZK_TRY(zk_scratch(ctx, "vk_mul_pts", pts.size() * 4, (void**)&d_pts));
    ZK_TRY(zk_scratch(ctx, "vk_mul_idx", pack.point_index.size() * 4, (void**)&d_idx));
    ZK_TRY(zk_scratch(ctx, "vk_mul_k", pack.scalars.size() * 4, (void**)&d_k));
    ZK_TRY(zk_scratch(ctx, "vk_mul_off", pack.seg_off.size() * 4, (void**)&d_off));
    ZK_TRY(zk_scratch(ctx, "vk_mul_out", n_seg * 96, (void**)&km->d_out));
    ZK_TRY(zk_scratch(ctx, "vk_mul_inf", n_seg * 4, (void**)&d_inf));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_pts, pts.data(), pts.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_idx, pack.point_index.data(), pack.point_index.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_k, pack.scalars.data(), pack.scalars.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_off, pack.seg_off.data(), pack.seg_off.size() * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(zk_g1_lincomb_launch(ctx, d_pts, pts.size() / 24, d_idx, d_k, d_off, n_seg, pack.lanes(), km->d_out, d_inf));
    km->h_out.resize(n_seg * 24);
    return ZK_OK;
}
void keys_mul_dev_collect(const KeysMulDev& km, std::vector<XYZZ<H1>>* pi, std::vector<XYZZ<H1>>* al) {
    for (auto& p : *pi) p = xyzz_inf<H1>();
    for (size_t g = 0; g < km.seg_slot.size(); g++) {
        const XYZZ<H1> x = xyzz_from_affine<H1>(aff_to_host64<G1Field>(aff_load<G1Field>(&km.h_out[24 * g])));
        const size_t s = km.seg_slot[g] >> 1;
        if (km.seg_slot[g] & 1) (*al)[s] = x;
        else (*pi)[s] = xyzz_add<H1>((*pi)[s], x);
    }
}

// ---- folded, on the device ------------------------------------------------------------------------------------------------------------
// vkeys[pl.used[s]] is the key of slot s; the subgroup tests run ALWAYS: the fold's soundness argument needs prime-order groups, and
// the Miller loop is not bilinear for a B outside G2.  The tail lanes: delta, gamma, beta of every slot behind the proofs.
int aggregate_keys_dev(zk_ctx* ctx, const zk_vkey* const* vkeys, const zkvk::Plan& pl, const zk_fr* inputs_host, const uint8_t* proofs_host,
                       const uint64_t* coeffs, int* ok_all, zk_gt* folded, const char* entry) {
    const size_t count = pl.count, K = pl.slots(), n = pl.fold_lanes();
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);

    // every level's seg_off | mis back to back
    std::vector<uint32_t> meta;
    meta.reserve(pl.meta_words);
    for (const zkvk::Level& lv : pl.levels) {
        meta.insert(meta.end(), lv.seg_off.begin(), lv.seg_off.end());
        meta.insert(meta.end(), lv.mis.begin(), lv.mis.end());
    }
    uint32_t *d_coef, *d_perm = nullptr, *d_meta, *ac, *b, *flags, *P, *Q, *ml, *part[2], *tag[2];
    ZK_TRY(zk_scratch(ctx, "agg_coef", count * 16, (void**)&d_coef));
    ZK_TRY(zk_scratch(ctx, "agg_flags", 4, (void**)&flags));
    if (!pl.identity()) ZK_TRY(zk_scratch(ctx, "vk_perm", count * 4, (void**)&d_perm));
    ZK_TRY(zk_scratch(ctx, "vk_meta", pl.meta_words * 4, (void**)&d_meta));
    ZK_TRY(zk_pair_scratch(ctx, n, &P, &Q, &ml));
    ZK_TRY(zk_fold_scratch(ctx, n, nullptr, nullptr));        // (reserved now: zk_miller_product takes them with the kernels in flight)
    ZK_TRY(zk_scratch(ctx, "vk_part_a", pl.part_a * XW * 4, (void**)&part[0]));
    ZK_TRY(zk_scratch(ctx, "vk_part_b", (pl.part_b + 1) * XW * 4, (void**)&part[1]));
    ZK_TRY(zk_scratch(ctx, "vk_tag_a", pl.part_a * 4, (void**)&tag[0]));
    ZK_TRY(zk_scratch(ctx, "vk_tag_b", (pl.part_b + 1) * 4, (void**)&tag[1]));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_coef, coeffs, count * 16, hipMemcpyHostToDevice, st));
    if (d_perm) ZK_HIP(ctx, hipMemcpyAsync(d_perm, pl.perm.data(), count * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_meta, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, st));
    ZkPhaseTimer tm(ctx);                         // with zk_set_profiling: "verify_aggregate.<phase>", device time by events
    ZkHostLap lap{ctx, "verify_aggregate."};      // ... and host wall-clock since the lap before
    std::vector<uint8_t> staging;
    ZK_TRY(stage_proofs(ctx, count, proofs_host, true, flags, nullptr, nullptr, &ac, &b, &staging, &tm, &lap));      // "k_decompress", "k_subgroup"
    tm.begin("verify_aggregate.k_scale");
    ZK_TRY(zk_g1_scale_fold_launch(ctx, ac, 2, false, d_coef, count, P, nullptr));                    // r_i A_i -> P[0 .. count)
    ZK_HIP(ctx, hipMemcpyAsync(Q, b, count * 192, hipMemcpyDeviceToDevice, st));
    for (size_t l = 0; l < pl.levels.size(); l++) {                                                    // sum r_i C_i per slot
        const uint32_t* lm = d_meta + l * 2 * (K + 1);
        if (!l) ZK_TRY(keyed_launch(ctx, ac + 24, 2, false, d_perm, d_coef, lm, K, pl.levels[0].n, part[0], tag[0]));
        else ZK_TRY(keyed_launch(ctx, part[(l - 1) & 1], 1, true, nullptr, nullptr, lm, K, pl.levels[l].n, part[l & 1], tag[l & 1]));
    }
    tm.end();
    const size_t last = (pl.levels.size() - 1) & 1, m_part = pl.fin_off[K];

    // under the device work: the coefficient sums over ranges of grouped positions, then the key multiplications
    std::vector<size_t> soff(K + 1, 0);
    for (size_t s = 0; s < K; s++) soff[s + 1] = soff[s] + vkeys[pl.used[s]]->ninp() + 1;
    const size_t tasks = std::min<size_t>(8, (count + 4095) / 4096), per = (count + tasks - 1) / tasks;
    std::vector<std::vector<HF>> part_s(tasks, std::vector<HF>(soff[K], HF::zero()));
    auto ninp_of = [&](size_t s) { return vkeys[pl.used[s]]->ninp(); };
    zk_over_ranges(ctx, tasks, tasks, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; t++)
            slot_sums(pl, ninp_of, soff, coeffs, inputs_host, std::min(count, t * per), std::min(count, (t + 1) * per), part_s[t].data());
    });
    std::vector<HF>& S = part_s[0];
    for (size_t t = 1; t < tasks; t++)
        for (size_t j = 0; j < soff[K]; j++) S[j] = S[j] + part_s[t][j];
    std::vector<XYZZ<H1>> pi(K), al(K);
    KeysMulDev km;
    const bool mul_dev = keys_mul_on_device(pl);
    if (mul_dev) ZK_TRY(keys_mul_dev_launch(ctx, vkeys, pl, soff, S, &km));
    else keys_mul_host(ctx, vkeys, pl, soff, S, &pi, &al);
    lap.lap("host_sums");
    // (only now: a copy into pageable memory waits for the stream, and the host work above is meant to run under the kernels)
    std::vector<uint32_t> h_part(m_part * XW), h_tag(m_part);
    uint32_t bad = 0;
    ZK_HIP(ctx, hipMemcpyAsync(h_part.data(), part[last], h_part.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(h_tag.data(), tag[last], h_tag.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, st));
    if (mul_dev) ZK_HIP(ctx, hipMemcpyAsync(km.h_out.data(), km.d_out, km.h_out.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("wait_scale");
    if (bad) { tm.resolve(); return ZK_OK; }                       // a point off its curve or outside its subgroup: ok_all = 0, folded all-zero
    if (mul_dev) keys_mul_dev_collect(km, &pi, &al);

    std::vector<uint32_t> tail_p(3 * K * 24), tail_q(3 * K * 48);
    for (size_t s = 0; s < K; s++) {
        const zk_vkey* vk = vkeys[pl.used[s]];
        XYZZ<H1> c_sum = xyzz_inf<H1>();
        for (size_t i = pl.fin_off[s]; i < pl.fin_off[s + 1]; i++) {
            if (h_tag[i] != s) ZK_FAIL(ctx, ZK_ERR_STATE, std::string(entry) + ": a partial of the keyed sum carries another key's slot");
            c_sum = xyzz_add<H1>(c_sum, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_part[i * XW])));
        }
        aff_store<G1Field>(&tail_p[(3 * s) * 24], aff_from_host64<G1Field>(xyzz_to_affine<H1>(c_sum)));
        aff_store<G1Field>(&tail_p[(3 * s + 1) * 24], aff_from_host64<G1Field>(xyzz_to_affine<H1>(pi[s])));
        aff_store<G1Field>(&tail_p[(3 * s + 2) * 24], aff_from_host64<G1Field>(xyzz_to_affine<H1>(al[s])));
        aff_store<G2Field>(&tail_q[(3 * s) * 48], aff_neg<G2Field>(vk->delta_g2));
        aff_store<G2Field>(&tail_q[(3 * s + 1) * 48], aff_neg<G2Field>(vk->gamma_g2));
        aff_store<G2Field>(&tail_q[(3 * s + 2) * 48], aff_neg<G2Field>(vk->beta_g2));
    }
    ZK_HIP(ctx, hipMemcpyAsync(P + count * 24, tail_p.data(), tail_p.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(Q + count * 48, tail_q.data(), tail_q.size() * 4, hipMemcpyHostToDevice, st));
    tm.begin("verify_aggregate.k_miller");
    ZK_TRY(zk_miller_launch(ctx, P, Q, n, ml));
    tm.end();
    Fq12<H2> r;
    ZK_TRY(zk_miller_product(ctx, ml, n, &r, &tm, &lap));      // "k_fold", "wait_miller", "host_finish" (waits: the tails may go)
    tm.resolve();
    *ok_all = fq12_eq<H2>(r, fq12_one<H2>()) ? 1 : 0;
    if (folded) zk_host_gt_out(folded, r);
    return ZK_OK;
}

// ---- proof by proof ---------------------------------------------------------------------------------------------------------------------
// The per-point flags of the staging (off the curve, with check_subgroup outside the subgroup) go into each proof's verdict by
// k_verify_layout.  prepared (or NULL; one slot only): the caller's prepared inputs, coordinates below q, in place of inputs_host
// (verify_proof_with_prepared_inputs).
int verify_keys_batch(zk_ctx* ctx, const zk_vkey* const* vkeys, const zkvk::Plan& pl, const zk_fr* inputs_host, const zk_g1_affine* prepared,
                      const uint8_t* proofs_host, bool check_subgroup, int* ok) {
    const size_t count = pl.count, K = pl.slots(), n = pl.batch_lanes();
    if (prepared && K != 1) return ZK_ERR_ARG;
    // the keys' constants per slot (-gamma | -delta of every slot, then every e(alpha, beta)), the slot of every grouped position,
    // the inputs in grouped order
    const size_t want_at = K * 2 * 48;
    std::vector<uint32_t> consts(want_at + K * FQ12_WORDS), slot_of(K > 1 ? count : 0), prep_w(prepared ? count * 24 : 0);
    for (size_t s = 0; s < K; s++) {
        const zk_vkey* vk = vkeys[pl.used[s]];
        aff_store<G2Field>(&consts[(2 * s) * 48], vk->neg_gamma_g2);
        aff_store<G2Field>(&consts[(2 * s + 1) * 48], vk->neg_delta_g2);
        memcpy(&consts[want_at + s * FQ12_WORDS], vk->e_alpha_beta, FQ12_WORDS * 4);
        for (size_t g = pl.seg_off[s]; K > 1 && g < pl.seg_off[s + 1]; g++) slot_of[g] = (uint32_t)s;
    }
    for (size_t k = 0; k < prep_w.size() / 24; k++) aff_store<G1Field>(&prep_w[24 * k], host_aff_from_abi<G1Field>((const uint64_t*)&prepared[k]));
    std::vector<zk_fr> gin(pl.identity() || prepared ? 0 : pl.gin_off[K]);      // (the identity plan: the caller's array is in grouped order)
    for (size_t g = 0, at = 0; g < count && !gin.empty(); g++) {
        const size_t i = pl.perm[g], len = pl.in_off[i + 1] - pl.in_off[i];
        if (len) memcpy(&gin[at], inputs_host + pl.in_off[i], len * sizeof(zk_fr));
        at += len;
    }
    const zk_fr* grouped = pl.identity() ? inputs_host : gin.data();
    uint32_t *d_consts, *d_slot = nullptr, *d_perm = nullptr, *ac, *b, *flags, *P, *Q, *ml, *prep;
    ZK_TRY(zk_scratch(ctx, "vk_consts", consts.size() * 4, (void**)&d_consts));
    if (K > 1) ZK_TRY(zk_scratch(ctx, "vk_slot", count * 4, (void**)&d_slot));
    if (!pl.identity()) ZK_TRY(zk_scratch(ctx, "vk_perm", count * 4, (void**)&d_perm));
    ZK_TRY(zk_scratch(ctx, "vfy_flags", (1 + 5 * count) * 4 + count * 4, (void**)&flags));      // any | bad_ac | bad_b | bad | inf | ok
    ZK_TRY(zk_scratch(ctx, "vfy_prep", count * 96, (void**)&prep));
    ZK_TRY(zk_pair_scratch(ctx, n, &P, &Q, &ml));
    uint32_t *bad_any = flags, *bad_ac = flags + 1, *bad_b = bad_ac + 2 * count, *bad = bad_b + count, *inf = bad + count;
    int* d_ok = (int*)(inf + count);
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_consts, consts.data(), consts.size() * 4, hipMemcpyHostToDevice, st));
    if (d_slot) ZK_HIP(ctx, hipMemcpyAsync(d_slot, slot_of.data(), count * 4, hipMemcpyHostToDevice, st));
    if (d_perm) ZK_HIP(ctx, hipMemcpyAsync(d_perm, pl.perm.data(), count * 4, hipMemcpyHostToDevice, st));
    std::vector<uint8_t> staging;
    ZK_TRY(stage_proofs(ctx, count, proofs_host, check_subgroup, bad_any, bad_ac, bad_b, &ac, &b, &staging));
    if (prepared) ZK_HIP(ctx, hipMemcpyAsync(prep, prep_w.data(), count * 96, hipMemcpyHostToDevice, st));
    for (size_t s = 0; s < K && !prepared; s++)      // (the one step whose launches grow with the used keys)
        ZK_TRY(prepare_inputs_dev(ctx, vkeys[pl.used[s]], pl.seg_off[s + 1] - pl.seg_off[s], grouped + pl.gin_off[s], prep + (size_t)pl.seg_off[s] * 24,
                                  inf + pl.seg_off[s]));
    hipLaunchKernelGGL(k_verify_layout, zk_blocks64(count), 64, 0, st, count, (const uint32_t*)d_perm, (const uint32_t*)d_slot, (const uint32_t*)prep,
                       (const uint32_t*)ac, (const uint32_t*)b, (const uint32_t*)d_consts, (const uint32_t*)bad_ac, (const uint32_t*)bad_b, P, Q, bad);
    ZK_HIP(ctx, hipGetLastError());
    ZK_TRY(zk_miller_launch(ctx, P, Q, n, ml));
    ZK_TRY(zk_pairing_finish_launch(ctx, ml, 3, count, nullptr, d_consts + want_at, bad, d_ok, d_slot));      // each proof against ITS key's e(alpha, beta)
    std::vector<int> okg(pl.identity() ? 0 : count);
    ZK_HIP(ctx, hipMemcpyAsync(pl.identity() ? ok : okg.data(), d_ok, count * sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    for (size_t g = 0; g < okg.size(); g++) ok[pl.perm[g]] = okg[g];      // back in the caller's order
    return ZK_OK;
}

// ---- seeded: the fold, and where it fails the checked proof-by-proof form to locate the bad proofs (agg: the entry point's name) ----
int aggregate_seeded(zk_ctx* ctx, const zk_vkey* const* vkeys, const zkvk::Plan& pl, const zk_fr* inputs_host, const uint8_t* proofs_host,
                     const uint8_t seed[32], int* ok_all, int* ok_each, const char* agg) {
    std::vector<uint64_t> coeffs(2 * pl.count);
    ZK_TRY(zk_verify_aggregate_coeffs_from_seed(seed, pl.count, coeffs.data()));
    ZK_TRY(aggregate_keys_dev(ctx, vkeys, pl, inputs_host, proofs_host, coeffs.data(), ok_all, nullptr, agg));
    if (!ok_each) return ZK_OK;
    if (*ok_all) {
        for (size_t i = 0; i < pl.count; i++) ok_each[i] = 1;
        return ZK_OK;
    }
    if (!pl.batch_fits()) return ZK_ERR_ARG;
    return verify_keys_batch(ctx, vkeys, pl, inputs_host, nullptr, proofs_host, true, ok_each);
}

}  // namespace

// ---- one key: the one-slot plan ---------------------------------------------------------------------------------------------------------
extern "C" int zk_groth16_vkey_verify_batch(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                            const uint8_t* proofs_host, int check_subgroup, int* ok) {
    ZK_API_BEGIN(ctx)
    if (!ok) return ZK_ERR_ARG;
    zkvk::Plan pl;
    ZK_TRY(one_key_args(ctx, vkey, count, inputs_host, inputs_per_proof, proofs_host, MAX_LANES / 3, "zk_groth16_vkey_verify_batch", &pl));
    return verify_keys_batch(ctx, &vkey, pl, inputs_host, nullptr, proofs_host, check_subgroup != 0, ok);
    ZK_API_END
}
extern "C" int zk_groth16_vkey_verify_prepared(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_g1_affine* prepared, const uint8_t* proofs_host,
                                               int check_subgroup, int* ok) {
    ZK_API_BEGIN(ctx)
    if (!prepared || !ok || !ctx || !vkey || !count || !proofs_host || count > MAX_LANES / 3) return ZK_ERR_ARG;
    for (size_t k = 0; k < count; k++)
        if (!zk_words_below_q((const uint64_t*)&prepared[k], 2)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_vkey_verify_prepared: a prepared input's coordinate is not below q");
    zkvk::Plan pl;
    size_t bad = 0;
    const size_t none = 0;                                             // (no public input is read)
    if (zkvk::make_plan(1, count, nullptr, &none, 0, &pl, &bad) != zkvk::PLAN_OK) return ZK_ERR_ARG;
    return verify_keys_batch(ctx, &vkey, pl, nullptr, prepared, proofs_host, check_subgroup != 0, ok);
    ZK_API_END
}
extern "C" int zk_groth16_vkey_verify_aggregate_coeffs(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                       const uint8_t* proofs_host, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_vkey_verify_aggregate";
    if (!coeffs) return ZK_ERR_ARG;
    zkvk::Plan pl;
    ZK_TRY(one_key_fold_args(ctx, vkey, count, inputs_host, inputs_per_proof, proofs_host, ok_all, entry, &pl));
    return aggregate_keys_dev(ctx, &vkey, pl, inputs_host, proofs_host, coeffs, ok_all, folded, entry);
    ZK_API_END
}
extern "C" int zk_groth16_vkey_verify_aggregate(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                const uint8_t* proofs_host, const uint8_t seed[32], int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_vkey_verify_aggregate";
    if (!seed) return ZK_ERR_ARG;
    zkvk::Plan pl;
    ZK_TRY(one_key_fold_args(ctx, vkey, count, inputs_host, inputs_per_proof, proofs_host, ok_all, entry, &pl));
    return aggregate_seeded(ctx, &vkey, pl, inputs_host, proofs_host, seed, ok_all, ok_each, entry);
    ZK_API_END
}

// ---- the forms on a proving key: the same on the vkey the key owns ------------------------------------------------------------------
static int pk_verify_batch(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, bool check_subgroup,
                           int* ok) {
    static const char* const entry = "zk_groth16_verify_batch";
    if (!ctx || !pk || !count || !proofs_host || !ok) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, entry, &vk));
    zkvk::Plan pl;
    ZK_TRY(one_key_args(ctx, vk, count, inputs_host, ninp, proofs_host, MAX_LANES / 3, entry, &pl));
    return verify_keys_batch(ctx, &vk, pl, inputs_host, nullptr, proofs_host, check_subgroup, ok);
}
extern "C" int zk_groth16_verify_batch(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                       const uint8_t* proofs_host, int* ok) {
    ZK_API_BEGIN(ctx)
    return pk_verify_batch(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, false, ok);
    ZK_API_END
}
extern "C" int zk_groth16_verify_batch_checked(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                               const uint8_t* proofs_host, int* ok) {
    ZK_API_BEGIN(ctx)
    return pk_verify_batch(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, true, ok);
    ZK_API_END
}
extern "C" int zk_groth16_verify_aggregate_coeffs(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                  const uint8_t* proofs_host, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_verify_aggregate";
    if (!ctx || !pk || !coeffs || !count || !proofs_host || !ok_all || count > MAX_LANES - 3 || (inputs_per_proof && !inputs_host)) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, entry, &vk));
    zkvk::Plan pl;
    ZK_TRY(one_key_fold_args(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, ok_all, entry, &pl));
    return aggregate_keys_dev(ctx, &vk, pl, inputs_host, proofs_host, coeffs, ok_all, folded, entry);
    ZK_API_END
}
extern "C" int zk_groth16_verify_aggregate(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                           const uint8_t* proofs_host, const uint8_t seed[32], int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_verify_aggregate";
    if (!ctx || !pk || !seed || !count || count > MAX_LANES - 3) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, entry, &vk));
    zkvk::Plan pl;
    ZK_TRY(one_key_fold_args(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, ok_all, entry, &pl));
    return aggregate_seeded(ctx, &vk, pl, inputs_host, proofs_host, seed, ok_all, ok_each, entry);
    ZK_API_END
}
extern "C" int zk_groth16_verify_aggregate_host(const zk_vk_host* vk, size_t count, const zk_fr* inputs, size_t inputs_per_proof, const uint8_t* proofs,
                                                const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN_NOCTX
    if (!vk || vk->gamma_abc_len != inputs_per_proof + 1) return ZK_ERR_ARG;
    return aggregate_keys_host(vk, 1, count, nullptr, inputs, count * inputs_per_proof, proofs, coeffs, ok_all, folded);
    ZK_API_END
}

// ---- several keys -----------------------------------------------------------------------------------------------------------------------
extern "C" int zk_groth16_vkeys_verify_batch(zk_ctx* ctx, const zk_vkey* const* vkeys, size_t n_keys, size_t count, const uint32_t* key_of,
                                             const zk_fr* inputs_host, size_t inputs_len, const uint8_t* proofs_host, int check_subgroup, int* ok) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_vkeys_verify_batch";
    if (!ok) return ZK_ERR_ARG;
    zkvk::Plan pl;
    ZK_TRY(keys_args(ctx, vkeys, n_keys, count, key_of, inputs_host, inputs_len, proofs_host, entry, &pl));
    ZK_TRY(lanes_refusal(ctx, pl.batch_fits(), entry, "3 count"));
    return verify_keys_batch(ctx, vkeys, pl, inputs_host, nullptr, proofs_host, check_subgroup != 0, ok);
    ZK_API_END
}

extern "C" int zk_groth16_vkeys_verify_aggregate_coeffs(zk_ctx* ctx, const zk_vkey* const* vkeys, size_t n_keys, size_t count, const uint32_t* key_of,
                                                        const zk_fr* inputs_host, size_t inputs_len, const uint8_t* proofs_host, const uint64_t* coeffs,
                                                        int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_vkeys_verify_aggregate";
    if (!coeffs || !ok_all) return ZK_ERR_ARG;
    zkvk::Plan pl;
    ZK_TRY(keys_args(ctx, vkeys, n_keys, count, key_of, inputs_host, inputs_len, proofs_host, entry, &pl));
    ZK_TRY(lanes_refusal(ctx, pl.fold_fits(), entry, "count + 3 used keys"));
    return aggregate_keys_dev(ctx, vkeys, pl, inputs_host, proofs_host, coeffs, ok_all, folded, entry);
    ZK_API_END
}

extern "C" int zk_groth16_vkeys_verify_aggregate(zk_ctx* ctx, const zk_vkey* const* vkeys, size_t n_keys, size_t count, const uint32_t* key_of,
                                                 const zk_fr* inputs_host, size_t inputs_len, const uint8_t* proofs_host, const uint8_t seed[32],
                                                 int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    static const char* const entry = "zk_groth16_vkeys_verify_aggregate";
    if (!seed || !ok_all) return ZK_ERR_ARG;
    zkvk::Plan pl;
    ZK_TRY(keys_args(ctx, vkeys, n_keys, count, key_of, inputs_host, inputs_len, proofs_host, entry, &pl));
    ZK_TRY(lanes_refusal(ctx, pl.fold_fits(), entry, "count + 3 used keys"));
    return aggregate_seeded(ctx, vkeys, pl, inputs_host, proofs_host, seed, ok_all, ok_each, entry);
    ZK_API_END
}

extern "C" int zk_groth16_verify_aggregate_keys_host(const zk_vk_host* vks, size_t n_keys, size_t count, const uint32_t* key_of, const zk_fr* inputs,
                                                     size_t inputs_len, const uint8_t* proofs, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN_NOCTX
    if (!key_of) return ZK_ERR_ARG;
    return aggregate_keys_host(vks, n_keys, count, key_of, inputs, inputs_len, proofs, coeffs, ok_all, folded);
    ZK_API_END
}
