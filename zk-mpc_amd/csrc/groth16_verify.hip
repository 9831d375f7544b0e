// groth16_verify.hip -- Groth16 verification: one proof on the host, a batch on the device proof by proof (zk_groth16_verify_batch),
// and a batch as ONE folded pairing product (zk_groth16_verify_aggregate), with the building block the fold needs beyond pairing.hip:
// the sum of many G1 points that belong to no resident table.
//
// Replaces (reference):
//   Groth16::verify (prepare_inputs, verify_proof_with_prepared_inputs)          arkworks/groth16/src/verifier.rs:13-61
// and for the folded form nothing the reference has for Groth16 (Groth16::verify is one proof); the fold itself is the one of its
// KZG verifier (poly-commit/src/kzg10/mod.rs:345, batch_check: a random linear combination of the equations, one product of
// pairings).  With coefficients r_i the batch holds iff
//     prod_i e(r_i A_i, B_i) . e(sum_i r_i C_i, -delta) . e(sum_j s_j gamma_abc[j], -gamma) . e(s_0 alpha, -beta) = 1
//     s_0 = sum_i r_i,  s_j = sum_i r_i x_{i,j} (mod r)
// count + 3 Miller loops and ONE final exponentiation (the batch form: 3 count and count).
//
// Every device form runs on a zk_vkey (groth16_vkey.hip); the entry points that take a zk_pk are the same code on the vkey the key owns.
// The prepared inputs gamma_abc[0] + sum x_i gamma_abc[i] of a batch are g1_prepare_inputs.hip's fixed-base kernel over the vkey's
// window table (prepare_inputs_dev; a key too large for a table: zk_msm_g1_multi_dev over gamma_abc), also a public step of its own
// (zk_groth16_prepare_inputs, zk_groth16_vkey_verify_prepared).
//   k_verify_layout   one proof per lane: the proof's three pairs laid out for the Miller launch.
//   k_g1_scale_fold   per lane an affine point and a 128-bit coefficient -> r P in XYZZ by g1_lincomb.cuh's fixed signed windows
//                     (32 windows; the digit selects a table entry in LDS and a sign, never the control flow), then either per
//                     lane the affine point (the Miller loop's P array) or a wave tree of complete additions through LDS and one
//                     XYZZ partial per block, or both.  Without coefficients it only sums (XYZZ partials or affine points).
// Both device forms check their arguments (device_args_ok) and stage their proofs (stage_proofs) by the same code and run pairing.hip's
// kernels behind it; the folded form ends in its zk_miller_product.  The host re-launches the sum on its partials until at most 64
// are left and finishes those itself in 64-bit limbs.
// The folded form's key multiplications -- the ninp + 2 full-width multiplications s_0 alpha, s_j gamma_abc[j] -- run on the
// context's helper threads under the device work, whatever ninp is (one MSM over gamma_abc in their place: DESIGN 6, not kept).
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "fsrng.hpp"
#include "g1_lincomb.cuh"
#include "groth16_int.hpp"
#include "groth16_verify_int.hpp"
#include "pairing.cuh"
#include <string.h>

using namespace zk;

namespace {

using H1 = Fq64Field;
using H2 = Fq264Field;
constexpr size_t MAX_LANES = ZK_PAIRING_MAX_LANES;
constexpr size_t SCALE_LDS = (size_t)LINCOMB_TAB * XW * 64 * 4;      // the window tables: 98 304 bytes
constexpr size_t SUM_LDS = (size_t)XW * 64 * 4;                      // the tree alone: 12 288 bytes


// ---- k_verify_layout --------------------------------------------------------------------------------------------------------------
// proof k: P[3 k .. 3 k + 2] = A, prepared inputs, C;  Q[3 k ..] = B, -gamma, -delta.  ac holds (A_k, C_k) at 2 k, 2 k + 1 and b
// holds B_k (table form, from the decompression, with their off-curve flags bad_ac / bad_b); prep the prepared inputs; negs = -gamma | -delta.
__global__ void __launch_bounds__(64) k_verify_layout(size_t count, const uint32_t* __restrict__ prep, const uint32_t* __restrict__ ac,
                                                      const uint32_t* __restrict__ b, const uint32_t* __restrict__ negs,
                                                      const uint32_t* __restrict__ bad_ac, const uint32_t* __restrict__ bad_b, uint32_t* __restrict__ P,
                                                      uint32_t* __restrict__ Q, uint32_t* __restrict__ bad) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= count) return;
    aff_store16<G1Field>(P, 3 * k, aff_load16<G1Field>(ac, 2 * k));
    aff_store16<G1Field>(P, 3 * k + 1, aff_load16<G1Field>(prep, k));
    aff_store16<G1Field>(P, 3 * k + 2, aff_load16<G1Field>(ac, 2 * k + 1));
    aff_store16<G2Field>(Q, 3 * k, aff_load16<G2Field>(b, k));
    aff_store16<G2Field>(Q, 3 * k + 1, aff_load16<G2Field>(negs, 0));
    aff_store16<G2Field>(Q, 3 * k + 2, aff_load16<G2Field>(negs, 1));
    bad[k] = bad_ac[2 * k] | bad_ac[2 * k + 1] | bad_b[k];
}

// ---- k_g1_scale_fold --------------------------------------------------------------------------------------------------------------
// lane g < n: point g in_step of `in` (affine table form, or XYZZ with in_xyzz) times coeffs[4 g ..] (128 bits, low word first;
// coeffs = NULL: times one, and the launch needs SUM_LDS bytes of LDS only, else SCALE_LDS).  out_aff (or NULL): the n products as
// affine points.  out_part (or NULL): one XYZZ sum per block.
__global__ void __launch_bounds__(64) k_g1_scale_fold(const uint32_t* __restrict__ in, uint32_t in_step, int in_xyzz, const uint32_t* __restrict__ coeffs,
                                                      uint32_t n, uint32_t* __restrict__ out_aff, uint32_t* __restrict__ out_part) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane;
    ZkLdsTab tab{lds + lane};
    XYZZ<G1Field> acc = xyzz_inf<G1Field>();
    if (coeffs) {
        Affine<G1Field> p = aff_inf<G1Field>();
        uint32_t k[4] = {0, 0, 0, 0};
        if (g < n) {
            p = aff_load16<G1Field>(in, (size_t)g * in_step);
            const uint4 c = reinterpret_cast<const uint4*>(coeffs)[g];
            k[0] = c.x; k[1] = c.y; k[2] = c.z; k[3] = c.w;
        }
        acc = lincomb_term<G1Field, ZkLdsTab, 4>(p, k, tab);
        __syncthreads();                                               // (the tree reuses entry 0 of the tables)
    } else if (g < n) {
        acc = in_xyzz ? xyzz_load16<G1Field>(in, (size_t)g * in_step) : xyzz_from_affine<G1Field>(aff_load16<G1Field>(in, (size_t)g * in_step));
    }
    if (out_aff && g < n) aff_store16<G1Field>(out_aff, g, xyzz_to_affine<G1Field>(acc));
    if (!out_part) return;
    // the complete addition: equal points double, opposite points cancel, infinity passes
#pragma unroll 1
    for (uint32_t s = 1; s < 64; s <<= 1) {
        const uint32_t pos = lane & (2 * s - 1);
        if (pos == s) tab.put(0, acc);
        __syncthreads();
        if (pos == 0) {
            ZkLdsTab other{lds + lane + s};
            acc = xyzz_add<G1Field>(acc, other.get(0));
        }
        __syncthreads();
    }
    if (lane == 0) xyzz_store16<G1Field>(out_part, blockIdx.x, acc);
}

}  // namespace

// ---- launches (internal.hpp: the Marlin aggregate runs them too) --------------------------------------------------------------------
int zk_g1_scale_fold_launch(zk_ctx* ctx, const uint32_t* in, uint32_t in_step, bool in_xyzz, const uint32_t* coeffs, size_t n, uint32_t* out_aff,
                            uint32_t* out_part) {
    if (!ctx->lds_attr_done[ZK_LDS_SCALE_FOLD]) {
        ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_g1_scale_fold, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCALE_LDS));
        ctx->lds_attr_done[ZK_LDS_SCALE_FOLD] = true;
    }
    hipLaunchKernelGGL(k_g1_scale_fold, zk_blocks64(n), 64, coeffs ? SCALE_LDS : SUM_LDS, ctx->stream, in, in_step, in_xyzz ? 1 : 0, coeffs, (uint32_t)n,
                       out_aff, out_part);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
// the m XYZZ partials in a summed down to at most 64 (a and b: room for m and m / 64 + 1 points); *res says where they are
int zk_g1_sum_down(zk_ctx* ctx, uint32_t* a, uint32_t* b, size_t* m, uint32_t** res) {
    while (*m > 64) {
        ZK_TRY(zk_g1_scale_fold_launch(ctx, a, 1, true, nullptr, *m, nullptr, b));
        *m = zk_blocks64(*m);
        std::swap(a, b);
    }
    *res = a;
    return ZK_OK;
}

bool zk_vk_host_ok(const zk_vk_host* vk, size_t ninp) {
    if (!vk || !vk->gamma_abc_g1 || vk->gamma_abc_len != ninp + 1) return false;
    if (!zk_words_below_q((const uint64_t*)&vk->alpha_g1, 2) || !zk_words_below_q((const uint64_t*)&vk->beta_g2, 4) ||
        !zk_words_below_q((const uint64_t*)&vk->gamma_g2, 4) || !zk_words_below_q((const uint64_t*)&vk->delta_g2, 4))
        return false;
    for (size_t i = 0; i <= ninp; i++)
        if (!zk_words_below_q((const uint64_t*)&vk->gamma_abc_g1[i], 2)) return false;
    return true;
}

namespace zkvfy {      // (groth16_verify_int.hpp: groth16_verify_keys.hip runs the same steps over several keys)

// ---- host halves --------------------------------------------------------------------------------------------------------------------
HF coeff_fr(const uint64_t* c) { return HF::from_u128(c); }      // lo + 2^64 hi
// s[0] = sum r_i, s[j + 1] = sum r_i x_{i,j} over the proofs [lo, hi)
void coeff_sums(const uint64_t* coeffs, const zk_fr* inputs, size_t ninp, size_t lo, size_t hi, HF* s) {
    for (size_t j = 0; j <= ninp; j++) s[j] = HF::zero();
    for (size_t i = lo; i < hi; i++) {
        const HF r = coeff_fr(coeffs + 2 * i);
        s[0] = s[0] + r;
        for (size_t j = 0; j < ninp; j++) s[j + 1] = s[j + 1] + r * HF::from_abi(inputs[i * ninp + j]);
    }
}
void coeff_words(const uint64_t* c, uint32_t k[8]) {
    k[0] = (uint32_t)c[0]; k[1] = (uint32_t)(c[0] >> 32); k[2] = (uint32_t)c[1]; k[3] = (uint32_t)(c[1] >> 32);
    k[4] = k[5] = k[6] = k[7] = 0;
}

// ---- what the forms share: checks and staging ---------------------------------------------------------------------------------------
bool inputs_below_r(const zk_fr* inputs, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!zk_fr_words_valid(inputs[i].l)) return false;
    return true;
}
bool vk_host_ok(const zk_vk_host* vk, size_t ninp) { return zk_vk_host_ok(vk, ninp); }
// prepare_inputs (verifier.rs:18-33) on host values
XYZZ<H1> host_prepare(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs) {
    XYZZ<H1> acc = xyzz_from_affine<H1>(zk_host_g1(&vk->gamma_abc_g1[0]));
    for (size_t i = 0; i < n_inputs; i++) {
        uint32_t kw[8];
        fr_abi_to_canon_words(inputs[i].l, kw);
        acc = xyzz_add<H1>(acc, host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->gamma_abc_g1[i + 1])), kw));
    }
    return acc;
}
// one proof's bytes as A, B, C on the host; false: a point off its curve, or with check_subgroup outside its subgroup (the test of
// Proof::deserialize: subgroup.cuh, host instantiation)
bool host_proof_points(const uint8_t proof[192], bool check_subgroup, Affine<G1Field>* a, Affine<G2Field>* b, Affine<G1Field>* c) {
    if (!zk_host_decompress_g1(proof, a) || !zk_host_decompress_g2(proof + 48, b) || !zk_host_decompress_g1(proof + 144, c)) return false;
    return !check_subgroup || (zk_host_in_subgroup_g1(*a) && zk_host_in_subgroup_g2(*b) && zk_host_in_subgroup_g1(*c));
}
// what prepare_inputs refuses of count input vectors, in the words of the entry point `entry`
int inputs_ok(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const char* entry) {
    if (vk->ninp() != ninp) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": inputs_per_proof is not num_instance - 1");
    if (ninp && !inputs_host) return ZK_ERR_ARG;
    if (ninp && count > ((size_t)1 << 30) / ninp) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": more than 2^30 public inputs in one call");
    if (!inputs_below_r(inputs_host, count * ninp)) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": a public input is not below r");
    return ZK_OK;
}
// what the device forms refuse of their key and arguments, in the words of the entry point `entry` (a zk_pk without verifying-key
// parts is refused where its vkey is asked for: zk_pk_vkey)
int device_args_ok(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, size_t max_count,
                   const char* entry) {
    if (!ctx || !vk || !count || !proofs_host || count > max_count) return ZK_ERR_ARG;
    return inputs_ok(ctx, vk, count, inputs_host, ninp, entry);
}
// The points of count proofs onto the device, for both device forms: the compressed (A_k, C_k) and the compressed B_k split out of
// the proofs' bytes into *staging (the caller keeps it until it has waited for the stream: the uploads read it), uploaded and
// decompressed into table form -- (*ac)[2 k], (*ac)[2 k + 1] = A_k, C_k and (*b)[k] = B_k -- and with check_subgroup tested for
// membership, one launch over the 2 count G1 points and one over the count G2 points whatever count is.  bad_any: one word, cleared
// here, set by a point off its curve or outside its subgroup.  bad_ac, bad_b (both or neither; else NULL): the same per point, 2 count
// and count words, "outside the subgroup" ORed into the off-curve flags.  tm, lap (both, or NULL): the caller's timers; tm gets the
// two decompress launches as "<lap->prefix>k_decompress" and the two subgroup launches as "<lap->prefix>k_subgroup".
int stage_proofs(zk_ctx* ctx, size_t count, const uint8_t* proofs_host, bool check_subgroup, uint32_t* bad_any, uint32_t* bad_ac, uint32_t* bad_b,
                 uint32_t** ac, uint32_t** b, std::vector<uint8_t>* staging, ZkPhaseTimer* tm, ZkHostLap* lap) {
    const bool timed = tm && lap && tm->enabled;
    staging->resize(count * 192);
    uint8_t *g1c = staging->data(), *g2c = g1c + count * 2 * 48;
    for (size_t k = 0; k < count; k++) {
        const uint8_t* pr = proofs_host + k * 192;
        memcpy(&g1c[(2 * k) * 48], pr, 48);
        memcpy(&g2c[k * 96], pr + 48, 96);
        memcpy(&g1c[(2 * k + 1) * 48], pr + 144, 48);
    }
    uint8_t *d_g1c, *d_g2c;
    ZK_TRY(zk_scratch(ctx, "vfy_g1c", count * 2 * 48, (void**)&d_g1c));
    ZK_TRY(zk_scratch(ctx, "vfy_g2c", count * 96, (void**)&d_g2c));
    ZK_TRY(zk_scratch(ctx, "vfy_ac", count * 2 * 96, (void**)ac));
    ZK_TRY(zk_scratch(ctx, "vfy_b", count * 192, (void**)b));
    ZK_HIP(ctx, hipMemcpyAsync(d_g1c, g1c, count * 2 * 48, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(d_g2c, g2c, count * 96, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipMemsetAsync(bad_any, 0, 4, ctx->stream));
    if (timed) tm->begin((std::string(lap->prefix) + "k_decompress").c_str());
    ZK_TRY(zk_decompress_launch(ctx, 1, (const uint32_t*)d_g1c, 2 * count, *ac, bad_any, bad_ac));
    ZK_TRY(zk_decompress_launch(ctx, 2, (const uint32_t*)d_g2c, count, *b, bad_any, bad_b));
    if (timed) tm->end();
    if (!check_subgroup) return ZK_OK;
    if (timed) tm->begin((std::string(lap->prefix) + "k_subgroup").c_str());
    ZK_TRY(zk_subgroup_launch(ctx, 1, *ac, 2 * count, bad_any, bad_ac, bad_ac != nullptr));
    ZK_TRY(zk_subgroup_launch(ctx, 2, *b, count, bad_any, bad_b, bad_b != nullptr));
    if (timed) tm->end();
    return ZK_OK;
}

// ---- proof by proof -------------------------------------------------------------------------------------------------------------------
// Groth16::verify on host values: e(A, B) e(prepared, -gamma) e(C, -delta) == e(alpha, beta)
int verify_host(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs, const uint8_t proof[192], int* ok, bool check_subgroup) {
    if (!proof || !ok || (n_inputs && !inputs) || !vk_host_ok(vk, n_inputs) || !inputs_below_r(inputs, n_inputs)) return ZK_ERR_ARG;
    *ok = 0;
    Affine<G1Field> a, c;
    Affine<G2Field> b;
    if (!host_proof_points(proof, check_subgroup, &a, &b, &c)) return ZK_OK;
    const XYZZ<H1> acc = host_prepare(vk, inputs, n_inputs);
    const Affine<H1> P[3] = {aff_to_host64<G1Field>(a), xyzz_to_affine<H1>(acc), aff_to_host64<G1Field>(c)};
    const Affine<H2> Q[3] = {aff_to_host64<G2Field>(b), aff_neg<H2>(zk_host_g2(&vk->gamma_g2)), aff_neg<H2>(zk_host_g2(&vk->delta_g2))};
    Fq12<H2> lhs, rhs;
    pairing_product<H2>(lhs, P, Q, 3);
    const Affine<H1> alpha = zk_host_g1(&vk->alpha_g1);
    const Affine<H2> beta = zk_host_g2(&vk->beta_g2);
    pairing_product<H2>(rhs, &alpha, &beta, 1);
    *ok = fq12_eq<H2>(lhs, rhs) ? 1 : 0;
    return ZK_OK;
}

// prepare_inputs for count proofs on the device, on ctx->stream: prep = count affine points (table form), inf = count infinity flags.
// A key with a window table (or without public inputs): k_g1_prepare_inputs, no wait.  A key too large for one: count vectors of
// ninp scalars through zk_msm_g1_multi_dev over gamma_abc[1 ..] (inputs_ok keeps count * ninp within that call's limit; it cuts the
// vectors into jobs itself), gamma_abc[0] added and the points normalised on the host -- the same points; that path waits.
int prepare_inputs_dev(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, uint32_t* prep, uint32_t* inf) {
    const size_t ninp = vk->ninp();
    hipStream_t st = ctx->stream;
    uint32_t *d_in = nullptr, *d_dig = nullptr;
    if (ninp) {
        ZK_TRY(zk_scratch(ctx, "vfy_in", count * ninp * 32 + 32, (void**)&d_in));
        ZK_HIP(ctx, hipMemcpyAsync(d_in, inputs_host, count * ninp * 32, hipMemcpyHostToDevice, st));
    }
    if (!ninp || vk->win) {
        if (ninp) ZK_TRY(zk_scratch(ctx, "vfy_digits", count * ninp * 32, (void**)&d_dig));
        return zk_g1_prepare_inputs_launch(ctx, d_in, count, ninp, vk->win, vk->gamma_abc->dev, d_dig, prep, inf);
    }
    std::vector<zk_g1_projective> sums(count);
    ZK_TRY(zk_msm_g1_multi_dev(ctx, vk->gamma_abc, 1, d_in, ninp, ninp, count, sums.data()));
    const XYZZ<H1> g0 = xyzz_from_affine<H1>(aff_to_host64<G1Field>(aff_load<G1Field>(vk->abc_host.data())));
    std::vector<XYZZ<H1>> x(count);
    for (size_t k = 0; k < count; k++) x[k] = xyzz_add<H1>(host64_proj_from_abi<H1>((const uint64_t*)&sums[k]), g0);
    const std::vector<Affine<H1>> a = host64_batch_to_affine<H1>(x);
    std::vector<uint32_t> w(count * 24), fl(count);
    for (size_t k = 0; k < count; k++) {
        aff_store<G1Field>(&w[24 * k], aff_from_host64<G1Field>(a[k]));
        fl[k] = aff_is_inf<H1>(a[k]) ? 1u : 0u;
    }
    ZK_HIP(ctx, hipMemcpyAsync(prep, w.data(), count * 96, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(inf, fl.data(), count * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    return ZK_OK;
}

// The per-point flags of the staging (off the curve, with check_subgroup outside the subgroup) go into each proof's verdict by
// k_verify_layout.  prepared (or NULL): the caller's prepared inputs in place of inputs_host (verify_proof_with_prepared_inputs).
int verify_batch(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const zk_g1_affine* prepared,
                 const uint8_t* proofs_host, int* ok, bool check_subgroup, const char* entry) {
    if (!ok) return ZK_ERR_ARG;
    std::vector<uint32_t> prep_w;
    if (prepared) {
        if (!ctx || !vk || !count || !proofs_host || count > MAX_LANES / 3) return ZK_ERR_ARG;
        for (size_t k = 0; k < count; k++)
            if (!zk_words_below_q((const uint64_t*)&prepared[k], 2)) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": a prepared input's coordinate is not below q");
        prep_w.resize(count * 24);
        for (size_t k = 0; k < count; k++) aff_store<G1Field>(&prep_w[24 * k], host_aff_from_abi<G1Field>((const uint64_t*)&prepared[k]));
    } else {
        ZK_TRY(device_args_ok(ctx, vk, count, inputs_host, ninp, proofs_host, MAX_LANES / 3, entry));
    }
    struct Consts { uint32_t negs[2 * 48]; uint32_t want[FQ12_WORDS]; } cs;      // the key's constants
    aff_store<G2Field>(cs.negs, vk->neg_gamma_g2);
    aff_store<G2Field>(cs.negs + 48, vk->neg_delta_g2);
    memcpy(cs.want, vk->e_alpha_beta, sizeof cs.want);

    const size_t n = 3 * count;
    uint32_t *d_cs, *ac, *b, *flags, *P, *Q, *ml, *prep;
    ZK_TRY(zk_scratch(ctx, "vfy_cs", sizeof cs, (void**)&d_cs));
    ZK_TRY(zk_scratch(ctx, "vfy_flags", (1 + 5 * count) * 4 + count * 4, (void**)&flags));      // any | bad_ac | bad_b | bad | inf | ok
    ZK_TRY(zk_scratch(ctx, "vfy_prep", count * 96, (void**)&prep));
    ZK_TRY(zk_pair_scratch(ctx, n, &P, &Q, &ml));
    uint32_t *bad_any = flags, *bad_ac = flags + 1, *bad_b = bad_ac + 2 * count, *bad = bad_b + count, *inf = bad + count;
    int* d_ok = (int*)(inf + count);
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_cs, &cs, sizeof cs, hipMemcpyHostToDevice, st));
    std::vector<uint8_t> staging;
    ZK_TRY(stage_proofs(ctx, count, proofs_host, check_subgroup, bad_any, bad_ac, bad_b, &ac, &b, &staging));
    if (prepared) ZK_HIP(ctx, hipMemcpyAsync(prep, prep_w.data(), count * 96, hipMemcpyHostToDevice, st));
    else ZK_TRY(prepare_inputs_dev(ctx, vk, count, inputs_host, prep, inf));
    hipLaunchKernelGGL(k_verify_layout, zk_blocks64(count), 64, 0, st, count, (const uint32_t*)prep, (const uint32_t*)ac, (const uint32_t*)b,
                       (const uint32_t*)d_cs, (const uint32_t*)bad_ac, (const uint32_t*)bad_b, P, Q, bad);
    ZK_HIP(ctx, hipGetLastError());
    ZK_TRY(zk_miller_launch(ctx, P, Q, n, ml));
    ZK_TRY(zk_pairing_finish_launch(ctx, ml, 3, count, nullptr, d_cs + 2 * 48, bad, d_ok));
    ZK_HIP(ctx, hipMemcpyAsync(ok, d_ok, count * sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    return ZK_OK;
}

// ---- folded -----------------------------------------------------------------------------------------------------------------------------
// what both aggregate forms refuse beyond their key's checks
bool agg_args_ok(size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const uint64_t* coeffs, const int* ok_all) {
    if (!count || !proofs || !coeffs || !ok_all || count > MAX_LANES - 3 || (ninp && !inputs)) return false;
    return true;
}

int aggregate_host(const zk_vk_host* vk, size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const uint64_t* coeffs, int* ok_all,
                   zk_gt* folded) {
    if (!agg_args_ok(count, inputs, ninp, proofs, coeffs, ok_all) || !vk_host_ok(vk, ninp) || !inputs_below_r(inputs, count * ninp)) return ZK_ERR_ARG;
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);
    std::vector<Affine<H1>> P(count + 3);
    std::vector<Affine<H2>> Q(count + 3);
    XYZZ<H1> c_sum = xyzz_inf<H1>();
    for (size_t i = 0; i < count; i++) {
        const uint8_t* pr = proofs + i * 192;
        Affine<G1Field> a, c;
        Affine<G2Field> b;
        if (!host_proof_points(pr, true, &a, &b, &c)) return ZK_OK;
        uint32_t k[8];
        coeff_words(coeffs + 2 * i, k);
        P[i] = xyzz_to_affine<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(a)), k));
        Q[i] = aff_to_host64<G2Field>(b);
        c_sum = xyzz_add<H1>(c_sum, host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(c)), k));
    }
    std::vector<HF> s(ninp + 1);
    coeff_sums(coeffs, inputs, ninp, 0, count, s.data());
    XYZZ<H1> pi = xyzz_inf<H1>();
    for (size_t j = 0; j <= ninp; j++) {
        uint32_t k[8];
        s[j].canon_words(k);
        pi = xyzz_add<H1>(pi, host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->gamma_abc_g1[j])), k));
    }
    uint32_t k0[8];
    s[0].canon_words(k0);
    P[count] = xyzz_to_affine<H1>(c_sum);
    Q[count] = aff_neg<H2>(zk_host_g2(&vk->delta_g2));
    P[count + 1] = xyzz_to_affine<H1>(pi);
    Q[count + 1] = aff_neg<H2>(zk_host_g2(&vk->gamma_g2));
    P[count + 2] = xyzz_to_affine<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->alpha_g1)), k0));
    Q[count + 2] = aff_neg<H2>(zk_host_g2(&vk->beta_g2));
    Fq12<H2> r;
    pairing_product<H2>(r, P.data(), Q.data(), count + 3);
    *ok_all = fq12_eq<H2>(r, fq12_one<H2>()) ? 1 : 0;
    if (folded) zk_host_gt_out(folded, r);
    return ZK_OK;
}

int aggregate_dev(zk_ctx* ctx, const zk_vkey* pk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, const uint64_t* coeffs,
                  int* ok_all, zk_gt* folded, const char* entry) {
    if (!agg_args_ok(count, inputs_host, ninp, proofs_host, coeffs, ok_all)) return ZK_ERR_ARG;
    ZK_TRY(device_args_ok(ctx, pk, count, inputs_host, ninp, proofs_host, MAX_LANES - 3, entry));
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);
    const std::vector<uint32_t>& abc_w = pk->abc_host;

    const size_t n = count + 3, n_part = zk_blocks64(count);
    uint32_t *d_coef, *ac, *b, *flags, *P, *Q, *ml, *part_a, *part_b;
    ZK_TRY(zk_scratch(ctx, "agg_coef", count * 16, (void**)&d_coef));
    ZK_TRY(zk_scratch(ctx, "agg_flags", 4, (void**)&flags));
    ZK_TRY(zk_pair_scratch(ctx, n, &P, &Q, &ml));
    ZK_TRY(zk_fold_scratch(ctx, n, nullptr, nullptr));        // (reserved now: zk_miller_product takes them with the kernels in flight)
    ZK_TRY(zk_scratch(ctx, "agg_part_a", n_part * XW * 4, (void**)&part_a));
    ZK_TRY(zk_scratch(ctx, "agg_part_b", (n_part / 64 + 1) * XW * 4, (void**)&part_b));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_coef, coeffs, count * 16, hipMemcpyHostToDevice, st));
    ZkPhaseTimer tm(ctx);                         // with zk_set_profiling: "verify_aggregate.<phase>", device time by events
    ZkHostLap lap{ctx, "verify_aggregate."};      // ... and host wall-clock since the lap before
    // the subgroup tests ALWAYS: the fold's soundness argument needs prime-order groups, and the Miller loop is not bilinear for a B outside G2
    std::vector<uint8_t> staging;
    ZK_TRY(stage_proofs(ctx, count, proofs_host, true, flags, nullptr, nullptr, &ac, &b, &staging, &tm, &lap));      // "k_decompress", "k_subgroup"
    tm.begin("verify_aggregate.k_scale");
    ZK_TRY(zk_g1_scale_fold_launch(ctx, ac, 2, false, d_coef, count, P, nullptr));                    // r_i A_i -> P[0 .. count)
    ZK_HIP(ctx, hipMemcpyAsync(Q, b, count * 192, hipMemcpyDeviceToDevice, st));
    ZK_TRY(zk_g1_scale_fold_launch(ctx, ac + 24, 2, false, d_coef, count, nullptr, part_a));          // sum r_i C_i, a partial per wave
    size_t m_part = n_part;
    uint32_t* part;
    ZK_TRY(zk_g1_sum_down(ctx, part_a, part_b, &m_part, &part));
    tm.end();

    // under the device work: the coefficient sums over ranges of proofs, then the ninp + 2 multiplications of key points side by side
    const size_t tasks = std::min<size_t>(8, (count + 4095) / 4096);
    std::vector<HF> part_s(tasks * (ninp + 1)), s(ninp + 1, HF::zero());
    const size_t per = (count + tasks - 1) / tasks;
    zk_over_ranges(ctx, tasks, tasks, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; t++) coeff_sums(coeffs, inputs_host, ninp, std::min(count, t * per), std::min(count, (t + 1) * per), &part_s[t * (ninp + 1)]);
    });
    for (size_t t = 0; t < tasks; t++)
        for (size_t j = 0; j <= ninp; j++) s[j] = s[j] + part_s[t * (ninp + 1) + j];
    std::vector<XYZZ<H1>> key_mul(ninp + 2);      // s_j gamma_abc[j], then s_0 alpha
    auto mul_key = [&](size_t j) {
        uint32_t k[8];
        s[j <= ninp ? j : 0].canon_words(k);
        const Affine<G1Field> p = j <= ninp ? aff_load<G1Field>(&abc_w[24 * j]) : pk->alpha_g1;
        const XYZZ<H1> x = xyzz_from_affine<H1>(aff_to_host64<G1Field>(p));
        key_mul[j] = pk->points_in_subgroup ? host64_scalar_mul_glv(x, k) : host64_scalar_mul<H1>(x, k);
    };
    {
        std::vector<ZkTask<void>> ts;
        for (size_t j = 1; j < ninp + 2; j++) ts.push_back(zk_async(ctx, [&mul_key, j] { mul_key(j); }));
        mul_key(0);
    }
    lap.lap("host_sums");
    // (only now: a copy into pageable memory waits for the stream, and the host work above is meant to run under the kernels)
    std::vector<uint32_t> h_part(m_part * XW);
    uint32_t bad = 0;
    ZK_HIP(ctx, hipMemcpyAsync(h_part.data(), part, h_part.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("wait_scale");
    if (bad) { tm.resolve(); return ZK_OK; }                       // a point off its curve or outside its subgroup: ok_all = 0, folded all-zero

    XYZZ<H1> c_sum = xyzz_inf<H1>(), pi = xyzz_inf<H1>();
    for (size_t i = 0; i < m_part; i++) c_sum = xyzz_add<H1>(c_sum, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_part[i * XW])));
    for (size_t j = 0; j <= ninp; j++) pi = xyzz_add<H1>(pi, key_mul[j]);
    struct Tail { uint32_t p[3 * 24]; uint32_t q[3 * 48]; } tail;
    aff_store<G1Field>(tail.p, aff_from_host64<G1Field>(xyzz_to_affine<H1>(c_sum)));
    aff_store<G1Field>(tail.p + 24, aff_from_host64<G1Field>(xyzz_to_affine<H1>(pi)));
    aff_store<G1Field>(tail.p + 48, aff_from_host64<G1Field>(xyzz_to_affine<H1>(key_mul[ninp + 1])));
    aff_store<G2Field>(tail.q, aff_neg<G2Field>(pk->delta_g2));
    aff_store<G2Field>(tail.q + 48, aff_neg<G2Field>(pk->gamma_g2));
    aff_store<G2Field>(tail.q + 96, aff_neg<G2Field>(pk->beta_g2));
    ZK_HIP(ctx, hipMemcpyAsync(P + count * 24, tail.p, sizeof tail.p, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(Q + count * 48, tail.q, sizeof tail.q, hipMemcpyHostToDevice, st));
    tm.begin("verify_aggregate.k_miller");
    ZK_TRY(zk_miller_launch(ctx, P, Q, n, ml));
    tm.end();
    Fq12<H2> r;
    ZK_TRY(zk_miller_product(ctx, ml, n, &r, &tm, &lap));      // "k_fold", "wait_miller", "host_finish"
    tm.resolve();
    *ok_all = fq12_eq<H2>(r, fq12_one<H2>()) ? 1 : 0;
    if (folded) zk_host_gt_out(folded, r);
    return ZK_OK;
}

}  // namespace zkvfy
using namespace zkvfy;

extern "C" int zk_groth16_verify_host(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs, const uint8_t proof[192], int* ok) {
    ZK_API_BEGIN_NOCTX
    return verify_host(vk, inputs, n_inputs, proof, ok, false);
    ZK_API_END
}
extern "C" int zk_groth16_verify_host_checked(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs, const uint8_t proof[192], int* ok) {
    ZK_API_BEGIN_NOCTX
    return verify_host(vk, inputs, n_inputs, proof, ok, true);
    ZK_API_END
}
extern "C" int zk_groth16_prepare_inputs_host(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs, zk_g1_affine* out) {
    ZK_API_BEGIN_NOCTX
    if (!out || (n_inputs && !inputs) || !vk_host_ok(vk, n_inputs) || !inputs_below_r(inputs, n_inputs)) return ZK_ERR_ARG;
    host_aff_to_abi<G1Field>((uint64_t*)out, aff_from_host64<G1Field>(xyzz_to_affine<H1>(host_prepare(vk, inputs, n_inputs))));
    return ZK_OK;
    ZK_API_END
}
extern "C" int zk_groth16_prepare_inputs(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                         zk_g1_affine* prepared_out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !vkey || !count || !prepared_out || count > MAX_LANES / 3) return ZK_ERR_ARG;
    ZK_TRY(inputs_ok(ctx, vkey, count, inputs_host, inputs_per_proof, "zk_groth16_prepare_inputs"));
    uint32_t *prep, *inf;
    ZK_TRY(zk_scratch(ctx, "vfy_prep", count * 96, (void**)&prep));
    ZK_TRY(zk_scratch(ctx, "vfy_flags", count * 4, (void**)&inf));
    ZK_TRY(prepare_inputs_dev(ctx, vkey, count, inputs_host, prep, inf));
    std::vector<uint32_t> w(count * 24), fl(count);
    ZK_HIP(ctx, hipMemcpyAsync(w.data(), prep, count * 96, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(fl.data(), inf, count * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t k = 0; k < count; k++) {
        const Affine<G1Field> a = aff_load<G1Field>(&w[24 * k]);
        if ((fl[k] != 0) != aff_is_inf<G1Field>(a)) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_groth16_prepare_inputs: the infinity flag and the point disagree");
        host_aff_to_abi<G1Field>((uint64_t*)&prepared_out[k], a);
    }
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_groth16_vkey_verify_batch(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                            const uint8_t* proofs_host, int check_subgroup, int* ok) {
    ZK_API_BEGIN(ctx)
    return verify_batch(ctx, vkey, count, inputs_host, inputs_per_proof, nullptr, proofs_host, ok, check_subgroup != 0, "zk_groth16_vkey_verify_batch");
    ZK_API_END
}
extern "C" int zk_groth16_vkey_verify_prepared(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_g1_affine* prepared, const uint8_t* proofs_host,
                                               int check_subgroup, int* ok) {
    ZK_API_BEGIN(ctx)
    if (!prepared) return ZK_ERR_ARG;
    return verify_batch(ctx, vkey, count, nullptr, 0, prepared, proofs_host, ok, check_subgroup != 0, "zk_groth16_vkey_verify_prepared");
    ZK_API_END
}
extern "C" int zk_groth16_vkey_verify_aggregate_coeffs(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                       const uint8_t* proofs_host, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    return aggregate_dev(ctx, vkey, count, inputs_host, inputs_per_proof, proofs_host, coeffs, ok_all, folded, "zk_groth16_vkey_verify_aggregate");
    ZK_API_END
}

// ---- the forms on a proving key: the same code on the vkey the key owns ----------------------------------------------------------
extern "C" int zk_groth16_verify_batch(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                       const uint8_t* proofs_host, int* ok) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !count || !proofs_host || !ok) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, "zk_groth16_verify_batch", &vk));
    return verify_batch(ctx, vk, count, inputs_host, inputs_per_proof, nullptr, proofs_host, ok, false, "zk_groth16_verify_batch");
    ZK_API_END
}
extern "C" int zk_groth16_verify_batch_checked(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                               const uint8_t* proofs_host, int* ok) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !count || !proofs_host || !ok) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, "zk_groth16_verify_batch", &vk));
    return verify_batch(ctx, vk, count, inputs_host, inputs_per_proof, nullptr, proofs_host, ok, true, "zk_groth16_verify_batch");
    ZK_API_END
}

extern "C" int zk_groth16_verify_aggregate_coeffs(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                  const uint8_t* proofs_host, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !agg_args_ok(count, inputs_host, inputs_per_proof, proofs_host, coeffs, ok_all)) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, "zk_groth16_verify_aggregate", &vk));
    return aggregate_dev(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, coeffs, ok_all, folded, "zk_groth16_verify_aggregate");
    ZK_API_END
}

extern "C" int zk_groth16_verify_aggregate_host(const zk_vk_host* vk, size_t count, const zk_fr* inputs, size_t inputs_per_proof, const uint8_t* proofs,
                                                const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN_NOCTX
    return aggregate_host(vk, count, inputs, inputs_per_proof, proofs, coeffs, ok_all, folded);
    ZK_API_END
}

extern "C" int zk_verify_aggregate_coeffs_from_seed(const uint8_t seed[32], size_t count, uint64_t* coeffs_out) {
    ZK_API_BEGIN_NOCTX
    if (!seed || (count && !coeffs_out)) return ZK_ERR_ARG;
    zkfs::ChaChaRng rng = zkfs::ChaChaRng::from_seed(seed, 20);
    for (size_t i = 0; i < count; i++) {
        coeffs_out[2 * i] = rng.next_u64();
        coeffs_out[2 * i + 1] = rng.next_u64();
        if (!(coeffs_out[2 * i] | coeffs_out[2 * i + 1])) coeffs_out[2 * i] = 1;
    }
    return ZK_OK;
    ZK_API_END
}

// the seeded form on a vkey, in the words of the entry points agg / batch (the located verdicts are the checked batch form's)
static int aggregate_seeded(zk_ctx* ctx, const zk_vkey* vk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host,
                            const uint8_t seed[32], int* ok_all, int* ok_each, const char* agg, const char* batch) {
    std::vector<uint64_t> coeffs(2 * count);
    ZK_TRY(zk_verify_aggregate_coeffs_from_seed(seed, count, coeffs.data()));
    ZK_TRY(aggregate_dev(ctx, vk, count, inputs_host, ninp, proofs_host, coeffs.data(), ok_all, nullptr, agg));
    if (!ok_each) return ZK_OK;
    if (*ok_all) {
        for (size_t i = 0; i < count; i++) ok_each[i] = 1;
        return ZK_OK;
    }
    return verify_batch(ctx, vk, count, inputs_host, ninp, nullptr, proofs_host, ok_each, true, batch);
}
extern "C" int zk_groth16_verify_aggregate(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                           const uint8_t* proofs_host, const uint8_t seed[32], int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !seed || !count || count > MAX_LANES - 3) return ZK_ERR_ARG;
    const zk_vkey* vk;
    ZK_TRY(zk_pk_vkey(ctx, pk, "zk_groth16_verify_aggregate", &vk));
    return aggregate_seeded(ctx, vk, count, inputs_host, inputs_per_proof, proofs_host, seed, ok_all, ok_each, "zk_groth16_verify_aggregate",
                            "zk_groth16_verify_batch");
    ZK_API_END
}
extern "C" int zk_groth16_vkey_verify_aggregate(zk_ctx* ctx, const zk_vkey* vkey, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                const uint8_t* proofs_host, const uint8_t seed[32], int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    if (!seed || !count || count > MAX_LANES - 3) return ZK_ERR_ARG;
    return aggregate_seeded(ctx, vkey, count, inputs_host, inputs_per_proof, proofs_host, seed, ok_all, ok_each, "zk_groth16_vkey_verify_aggregate",
                            "zk_groth16_vkey_verify_batch");
    ZK_API_END
}

extern "C" int zk_diag_g1_scale_sum_dev(zk_ctx* ctx, const zk_g1_affine* pts, const uint64_t* coeffs, size_t n, zk_g1_affine* scaled_out,
                                        zk_g1_projective* sum_out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pts || !sum_out || !n || n > MAX_LANES) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&pts[i], 2)) return ZK_ERR_ARG;
    std::vector<uint32_t> w(n * 24);
    for (size_t i = 0; i < n; i++) aff_store<G1Field>(&w[24 * i], host_aff_from_abi<G1Field>((const uint64_t*)&pts[i]));
    const size_t n_part = zk_blocks64(n);
    uint32_t *d_pts, *d_coef = nullptr, *d_aff = nullptr, *part_a, *part_b;
    ZK_TRY(zk_scratch(ctx, "agg_diag_pts", n * 96, (void**)&d_pts));
    if (coeffs) ZK_TRY(zk_scratch(ctx, "agg_coef", n * 16, (void**)&d_coef));
    if (scaled_out) ZK_TRY(zk_scratch(ctx, "agg_diag_aff", n * 96, (void**)&d_aff));
    ZK_TRY(zk_scratch(ctx, "agg_part_a", n_part * XW * 4, (void**)&part_a));
    ZK_TRY(zk_scratch(ctx, "agg_part_b", (n_part / 64 + 1) * XW * 4, (void**)&part_b));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_pts, w.data(), n * 96, hipMemcpyHostToDevice, st));
    if (coeffs) ZK_HIP(ctx, hipMemcpyAsync(d_coef, coeffs, n * 16, hipMemcpyHostToDevice, st));
    ZK_TRY(zk_g1_scale_fold_launch(ctx, d_pts, 1, false, d_coef, n, d_aff, part_a));
    size_t m = n_part;
    uint32_t* part;
    ZK_TRY(zk_g1_sum_down(ctx, part_a, part_b, &m, &part));
    std::vector<uint32_t> h_part(m * XW);
    ZK_HIP(ctx, hipMemcpyAsync(h_part.data(), part, h_part.size() * 4, hipMemcpyDeviceToHost, st));
    if (scaled_out) ZK_HIP(ctx, hipMemcpyAsync(w.data(), d_aff, n * 96, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    XYZZ<H1> sum = xyzz_inf<H1>();
    for (size_t i = 0; i < m; i++) sum = xyzz_add<H1>(sum, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_part[i * XW])));
    host64_write_projective<H1>(xyzz_to_affine<H1>(sum), (uint64_t*)sum_out);
    if (scaled_out)
        for (size_t i = 0; i < n; i++) host_aff_to_abi<G1Field>((uint64_t*)&scaled_out[i], aff_load<G1Field>(&w[24 * i]));
    return ZK_OK;
    ZK_API_END
}
