// groth16_verify.hip -- Groth16 verification: one proof on the host (zk_groth16_verify_host), prepare_inputs on the host and on the
// device, and the steps that the batch forms of groth16_verify_keys.hip run for any number of keys: the checks of one key's
// arguments, the staging of the proofs, and the sum of many G1 points that belong to no resident table.
//
// Replaces (reference):
//   Groth16::verify (prepare_inputs, verify_proof_with_prepared_inputs)          arkworks/groth16/src/verifier.rs:13-61
//
// The prepared inputs gamma_abc[0] + sum x_i gamma_abc[i] of a batch are g1_prepare_inputs.hip's fixed-base kernel over the vkey's
// window table (prepare_inputs_dev; a key too large for a table: zk_msm_g1_multi_dev over gamma_abc), also a public step of its own
// (zk_groth16_prepare_inputs, zk_groth16_vkey_verify_prepared).
//   k_g1_scale_fold   per lane an affine point and a 128-bit coefficient -> r P in XYZZ by g1_lincomb.cuh's fixed signed windows
//                     (32 windows; the digit selects a table entry in LDS and a sign, never the control flow), then either per
//                     lane the affine point (the Miller loop's P array) or a wave tree of complete additions through LDS and one
//                     XYZZ partial per block, or both.  Without coefficients it only sums (XYZZ partials or affine points).
// The host re-launches the sum on its partials until at most 64 are left (zk_g1_sum_down) and finishes those itself in 64-bit limbs;
// the folded Groth16 form takes r_i A_i from it, the Marlin aggregate and g1_term_fold.hip its sums.
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

namespace zkvfy {      // (groth16_verify_int.hpp: the batch forms of groth16_verify_keys.hip run these steps)

// ---- host halves --------------------------------------------------------------------------------------------------------------------
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
// The points of count proofs onto the device, for every device form: the compressed (A_k, C_k) and the compressed B_k split out of
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

// ---- one proof, and prepare_inputs -------------------------------------------------------------------------------------------------------------------
// Groth16::verify on host values: e(A, B) e(prepared, -gamma) e(C, -delta) == e(alpha, beta)
int verify_host(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs, const uint8_t proof[192], int* ok, bool check_subgroup) {
    if (!proof || !ok || (n_inputs && !inputs) || !zk_vk_host_ok(vk, n_inputs) || !inputs_below_r(inputs, n_inputs)) return ZK_ERR_ARG;
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
    if (!out || (n_inputs && !inputs) || !zk_vk_host_ok(vk, n_inputs) || !inputs_below_r(inputs, n_inputs)) return ZK_ERR_ARG;
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
