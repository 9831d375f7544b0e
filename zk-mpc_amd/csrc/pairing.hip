// pairing.hip -- the BLS12-377 pairing on the device and Groth16 verification of batches.
//
// Replaces (reference):
//   PairingEngine::product_of_pairings / miller_loop / final_exponentiation      arkworks/algebra/ec/src/lib.rs:80-130, models/bls12/mod.rs
//   Groth16::verify (prepare_inputs, verify_proof_with_prepared_inputs)          arkworks/groth16/src/verifier.rs:13-61
// The arithmetic is pairing.cuh, instantiated over Fq2Field here for the kernels and over Fq264Field for the host forms.
//
//   k_miller          one pairing per lane: (G1 affine, G2 affine) -> the Miller value, an Fq12 of 144 packed words
//   k_pairing_finish  one product per lane: the product of its `pairs` Miller values, the final exponentiation, then the GT value
//                     in the ABI's form and / or the verdict against a given GT value
//   k_verify_prepare  one proof per lane: gamma_abc[0] + sum x_i gamma_abc[i] by double-and-add (the usual handful of public
//                     inputs; a key with very many would want the multi-vector MSM instead), and the proof's three pairs laid out
//   k_diag_fq12       the tower operations, one case per lane (tests)
// Lanes of a wave never part on data inside the pairing: the bits of x are compile-time constants, infinity is a select at the
// end.  (k_verify_prepare's scalar multiplication does branch on scalar bits; it is microseconds beside the Miller loops.)
// Registers: an Fq12 is 156 limb words, and a product of two needs three of them live: the tower functions are calls and their
// temporaries live in scratch (DESIGN 5 has the figures from the compiler's metadata).
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "pairing.cuh"
#include <string.h>

using namespace zk;

namespace {

using D2 = Fq2Field;
using H2 = Fq264Field;
constexpr int GTW = 144;            // 32-bit words of an Fq12, packed (either form)

__device__ __forceinline__ void fq12_store_packed(uint32_t* w, const Fq12<D2>& f) {
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) felt_store16<D2>(w + 24 * (3 * i + j), f.c[i].c[j]);
}
__device__ __forceinline__ Fq12<D2> fq12_load_packed(const uint32_t* w) {
    Fq12<D2> f;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) f.c[i].c[j] = felt_load16<D2>(w + 24 * (3 * i + j));
    return f;
}

// EXT: the points are the ABI's structs (Montgomery words of the reference); else table form (internal, packed)
template <bool EXT>
__global__ void __launch_bounds__(64) k_miller(const uint32_t* __restrict__ p, const uint32_t* __restrict__ q, size_t n, uint32_t* __restrict__ out) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    Affine<G1Field> P = aff_load16<G1Field>(p, i);
    Affine<G2Field> Q = aff_load16<G2Field>(q, i);
    if (EXT) {      // all-zero words stay all-zero: infinity keeps its encoding
        P = Affine<G1Field>{FqField::ext_to_int(P.x), FqField::ext_to_int(P.y)};
        Q = Affine<G2Field>{D2::ext_to_int(Q.x), D2::ext_to_int(Q.y)};
    }
    Fq12<D2> f;
    miller_loop<D2>(f, P, Q);
    fq12_store_packed(out + i * GTW, f);
}

// gt (or NULL): count GT values in the ABI's form.  ok (or NULL): ok[k] = the product equals `want` (packed, internal form) and
// bad[k] (or NULL) is clear.
__global__ void __launch_bounds__(64) k_pairing_finish(const uint32_t* __restrict__ ml, size_t pairs, size_t count, uint32_t* __restrict__ gt,
                                                       const uint32_t* __restrict__ want, const uint32_t* __restrict__ bad, int* __restrict__ ok) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= count) return;
    Fq12<D2> acc = fq12_load_packed(ml + k * pairs * GTW);
    for (size_t j = 1; j < pairs; j++) {
        const Fq12<D2> f = fq12_load_packed(ml + (k * pairs + j) * GTW);
        fq12_mul<D2>(acc, acc, f);
    }
    Fq12<D2> r;
    final_exponentiation<D2>(r, acc);
    if (gt) fq12_to_ext<D2>(gt + k * GTW, r);
    if (ok) {
        const Fq12<D2> w = fq12_load_packed(want);
        ok[k] = (fq12_eq<D2>(r, w) && !(bad && bad[k])) ? 1 : 0;
    }
}

// proof k: P[3 k .. 3 k + 2] = A, prepared inputs, C;  Q[3 k ..] = B, -gamma, -delta.  ac holds (A_k, C_k) at 2 k, 2 k + 1 and b
// holds B_k (table form, from the decompression, with their off-curve flags bad_ac / bad_b); negs = -gamma | -delta.
__global__ void __launch_bounds__(64) k_verify_prepare(size_t count, size_t ninp, const uint32_t* __restrict__ inputs, const uint32_t* __restrict__ gamma_abc,
                                                       const uint32_t* __restrict__ ac, const uint32_t* __restrict__ b, const uint32_t* __restrict__ negs,
                                                       const uint32_t* __restrict__ bad_ac, const uint32_t* __restrict__ bad_b, uint32_t* __restrict__ P,
                                                       uint32_t* __restrict__ Q, uint32_t* __restrict__ bad) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= count) return;
    XYZZ<G1Field> acc = xyzz_from_affine<G1Field>(aff_load16<G1Field>(gamma_abc, 0));
    for (size_t i = 0; i < ninp; i++) {
        uint32_t kw[8];
        fp_pack<FrParams>(kw, fp_ext_to_canon<FrParams>(fr_load(inputs, k * ninp + i)));
        acc = xyzz_add<G1Field>(acc, xyzz_scalar_mul<G1Field>(aff_load16<G1Field>(gamma_abc, i + 1), kw, 8));
    }
    aff_store16<G1Field>(P, 3 * k, aff_load16<G1Field>(ac, 2 * k));
    aff_store16<G1Field>(P, 3 * k + 1, xyzz_to_affine<G1Field>(acc));
    aff_store16<G1Field>(P, 3 * k + 2, aff_load16<G1Field>(ac, 2 * k + 1));
    aff_store16<G2Field>(Q, 3 * k, aff_load16<G2Field>(b, k));
    aff_store16<G2Field>(Q, 3 * k + 1, aff_load16<G2Field>(negs, 0));
    aff_store16<G2Field>(Q, 3 * k + 2, aff_load16<G2Field>(negs, 1));
    bad[k] = bad_ac[2 * k] | bad_ac[2 * k + 1] | bad_b[k];
}

// ---- the tower operations as a test hook: op 0 a b, 1 a^2, 2 a times the line (b.c[0].c[0], b.c[1].c[0], b.c[1].c[1]), 3 1 / a,
// 4 - 6 a^(q^1..3), 7 the cyclotomic squaring of a.  A case is (a, b) in the ABI's form; one result per case. ----------------------------
template <class F2>
__host__ __device__ void diag_fq12_op(int op, const uint32_t* in, uint32_t* out) {
    const Fq12<F2> a = fq12_from_ext<F2>(in), b = fq12_from_ext<F2>(in + GTW);
    Fq12<F2> r = a;
    switch (op) {
        case 0: fq12_mul<F2>(r, a, b); break;
        case 1: fq12_sqr<F2>(r, a); break;
        case 2: fq12_mul_line<F2>(r, a, Line<F2>{b.c[0].c[0], b.c[1].c[0], b.c[1].c[1]}); break;
        case 3: fq12_inv<F2>(r, a); break;
        case 4: fq12_frobenius<F2, 1>(r, a); break;
        case 5: fq12_frobenius<F2, 2>(r, a); break;
        case 6: fq12_frobenius<F2, 3>(r, a); break;
        case 7: fq12_cyclotomic_sqr<F2>(r, a); break;
        default: break;
    }
    fq12_to_ext<F2>(out, r);
}
__global__ void __launch_bounds__(64) k_diag_fq12(int op, const uint32_t* __restrict__ in, uint32_t* __restrict__ out, size_t n) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    diag_fq12_op<D2>(op, in + i * 2 * GTW, out + i * GTW);
}

inline unsigned blocks64(size_t n) { return (unsigned)((n + 63) / 64); }
constexpr size_t PAIRING_MAX_LANES = ZK_PAIRING_MAX_LANES;

// ---- host forms ----------------------------------------------------------------------------------------------------------------------
Fq12<H2> host_gt(const zk_gt* g) {
    uint32_t w[GTW];
    memcpy(w, g, sizeof w);
    return fq12_from_ext<H2>(w);
}
void host_gt_out(zk_gt* g, const Fq12<H2>& f) {
    uint32_t w[GTW];
    fq12_to_ext<H2>(w, f);
    memcpy(g, w, sizeof w);
}

// Groth16::verify on host values: e(A, B) e(prepared, -gamma) e(C, -delta) == e(alpha, beta)
struct HostVk {
    Affine<Fq64Field> alpha;
    Affine<H2> beta, neg_gamma, neg_delta;
};
void host_e_alpha_beta(const HostVk& vk, Fq12<H2>& out) { pairing_product<H2>(out, &vk.alpha, &vk.beta, 1); }

// the key's e(alpha, beta), packed internal words; computed once per key
void pk_e_alpha_beta(const zk_pk* pk, uint32_t out[GTW]) {
    std::lock_guard<std::mutex> g(pk->e_alpha_beta_mu);
    if (!pk->have_e_alpha_beta) {
        HostVk vk;
        vk.alpha = aff_to_host64<G1Field>(pk->alpha_g1);
        vk.beta = aff_to_host64<G2Field>(pk->beta_g2);
        Fq12<H2> e;
        host_e_alpha_beta(vk, e);
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 3; j++) D2::store(pk->e_alpha_beta + 24 * (3 * i + j), H2::to_dev(e.c[i].c[j]));
        pk->have_e_alpha_beta = true;
    }
    memcpy(out, pk->e_alpha_beta, GTW * 4);
}

}  // namespace

// the two kernels for a caller that has laid out its pairs on the device already (marlin_verify.hip): table-form points, `want` and
// `bad` as k_pairing_finish takes them, ok[k] on the device; on ctx->stream, no wait
int zk_miller_launch(zk_ctx* ctx, const uint32_t* p_dev, const uint32_t* q_dev, size_t n, uint32_t* ml_dev) {
    hipLaunchKernelGGL(k_miller<false>, blocks64(n), 64, 0, ctx->stream, p_dev, q_dev, n, ml_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int zk_miller_ext_launch(zk_ctx* ctx, const uint32_t* p_dev, const uint32_t* q_dev, size_t n, uint32_t* ml_dev) {
    hipLaunchKernelGGL(k_miller<true>, blocks64(n), 64, 0, ctx->stream, p_dev, q_dev, n, ml_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int zk_pairing_finish_launch(zk_ctx* ctx, const uint32_t* ml_dev, size_t pairs, size_t count, const uint32_t* want_dev, const uint32_t* bad_dev, int* ok_dev) {
    hipLaunchKernelGGL(k_pairing_finish, blocks64(count), 64, 0, ctx->stream, ml_dev, pairs, count, (uint32_t*)nullptr, want_dev, bad_dev, ok_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

extern "C" int zk_gt_exponent_multiple(void) {
    ZK_API_BEGIN_NOCTX
    return ZK_GT_EXPONENT_MULTIPLE;
    ZK_API_END
}

extern "C" int zk_pairing_products_host(const zk_g1_affine* p, const zk_g2_affine* q, size_t pairs, size_t count, zk_gt* outs) {
    ZK_API_BEGIN_NOCTX
    if (!p || !q || !outs || !pairs || !count || pairs > PAIRING_MAX_LANES / count) return ZK_ERR_ARG;
    std::vector<Affine<Fq64Field>> P(pairs);
    std::vector<Affine<H2>> Q(pairs);
    for (size_t k = 0; k < count; k++) {
        for (size_t j = 0; j < pairs; j++) {
            if (!zk_words_below_q((const uint64_t*)&p[k * pairs + j], 2) || !zk_words_below_q((const uint64_t*)&q[k * pairs + j], 4)) return ZK_ERR_ARG;
            P[j] = zk_host_g1(&p[k * pairs + j]);
            Q[j] = zk_host_g2(&q[k * pairs + j]);
        }
        Fq12<H2> r;
        pairing_product<H2>(r, P.data(), Q.data(), pairs);
        host_gt_out(&outs[k], r);
    }
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_pairing_products(zk_ctx* ctx, const zk_g1_affine* p, const zk_g2_affine* q, size_t pairs, size_t count, zk_gt* outs) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !p || !q || !outs || !pairs || !count || pairs > PAIRING_MAX_LANES / count) return ZK_ERR_ARG;
    const size_t n = pairs * count;
    uint32_t *dp, *dq, *ml, *gt;
    ZK_TRY(zk_scratch(ctx, "pair_p", n * 96, (void**)&dp));
    ZK_TRY(zk_scratch(ctx, "pair_q", n * 192, (void**)&dq));
    ZK_TRY(zk_scratch(ctx, "pair_ml", n * GTW * 4, (void**)&ml));
    ZK_TRY(zk_scratch(ctx, "pair_gt", count * GTW * 4, (void**)&gt));
    ZK_HIP(ctx, hipMemcpyAsync(dp, p, n * 96, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(dq, q, n * 192, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_miller<true>, blocks64(n), 64, 0, ctx->stream, (const uint32_t*)dp, (const uint32_t*)dq, n, ml);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pairing_finish, blocks64(count), 64, 0, ctx->stream, (const uint32_t*)ml, pairs, count, gt, (const uint32_t*)nullptr,
                       (const uint32_t*)nullptr, (int*)nullptr);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(outs, gt, count * GTW * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_gt_is_one(const zk_gt* a) {
    ZK_API_BEGIN_NOCTX
    if (!a) return 0;
    zk_gt one;
    host_gt_out(&one, fq12_one<H2>());
    return memcmp(a, &one, sizeof one) == 0 ? 1 : 0;
    ZK_API_END
}
extern "C" int zk_gt_eq(const zk_gt* a, const zk_gt* b) {
    ZK_API_BEGIN_NOCTX
    return (a && b && memcmp(a, b, sizeof(zk_gt)) == 0) ? 1 : 0;
    ZK_API_END
}
extern "C" int zk_gt_mul(const zk_gt* a, const zk_gt* b, zk_gt* out) {
    ZK_API_BEGIN_NOCTX
    if (!a || !b || !out || !zk_words_below_q((const uint64_t*)a, 12) || !zk_words_below_q((const uint64_t*)b, 12)) return ZK_ERR_ARG;
    Fq12<H2> r;
    fq12_mul<H2>(r, host_gt(a), host_gt(b));
    host_gt_out(out, r);
    return ZK_OK;
    ZK_API_END
}

namespace {
// check_subgroup: A, B, C also pass the subgroup test of Proof::deserialize (subgroup.cuh, host instantiation)
int verify_host(const zk_vk_host* vk, const zk_fr* inputs, size_t n_inputs, const uint8_t proof[192], int* ok, bool check_subgroup) {
    if (!vk || !proof || !ok || !vk->gamma_abc_g1 || vk->gamma_abc_len != n_inputs + 1 || (n_inputs && !inputs)) return ZK_ERR_ARG;
    if (!zk_words_below_q((const uint64_t*)&vk->alpha_g1, 2) || !zk_words_below_q((const uint64_t*)&vk->beta_g2, 4) ||
        !zk_words_below_q((const uint64_t*)&vk->gamma_g2, 4) || !zk_words_below_q((const uint64_t*)&vk->delta_g2, 4))
        return ZK_ERR_ARG;
    for (size_t i = 0; i <= n_inputs; i++)
        if (!zk_words_below_q((const uint64_t*)&vk->gamma_abc_g1[i], 2)) return ZK_ERR_ARG;
    for (size_t i = 0; i < n_inputs; i++)
        if (!zk_fr_words_valid(inputs[i].l)) return ZK_ERR_ARG;
    *ok = 0;
    Affine<G1Field> a, c;
    Affine<G2Field> b;
    if (!zk_host_decompress_g1(proof, &a) || !zk_host_decompress_g2(proof + 48, &b) || !zk_host_decompress_g1(proof + 144, &c)) return ZK_OK;
    if (check_subgroup && !(zk_host_in_subgroup_g1(a) && zk_host_in_subgroup_g2(b) && zk_host_in_subgroup_g1(c))) return ZK_OK;
    // prepare_inputs (verifier.rs:18-33)
    XYZZ<Fq64Field> acc = xyzz_from_affine<Fq64Field>(zk_host_g1(&vk->gamma_abc_g1[0]));
    for (size_t i = 0; i < n_inputs; i++) {
        uint32_t kw[8];
        fr_abi_to_canon_words(inputs[i].l, kw);
        acc = xyzz_add<Fq64Field>(acc, host64_scalar_mul<Fq64Field>(xyzz_from_affine<Fq64Field>(zk_host_g1(&vk->gamma_abc_g1[i + 1])), kw));
    }
    const Affine<Fq64Field> P[3] = {aff_to_host64<G1Field>(a), xyzz_to_affine<Fq64Field>(acc), aff_to_host64<G1Field>(c)};
    const Affine<H2> Q[3] = {aff_to_host64<G2Field>(b), aff_neg<H2>(zk_host_g2(&vk->gamma_g2)), aff_neg<H2>(zk_host_g2(&vk->delta_g2))};
    Fq12<H2> lhs, rhs;
    pairing_product<H2>(lhs, P, Q, 3);
    const Affine<Fq64Field> alpha = zk_host_g1(&vk->alpha_g1);
    const Affine<H2> beta = zk_host_g2(&vk->beta_g2);
    pairing_product<H2>(rhs, &alpha, &beta, 1);
    *ok = fq12_eq<H2>(lhs, rhs) ? 1 : 0;
    return ZK_OK;
}

// check_subgroup: behind the decompression one launch over the 2 count G1 points and one over the count G2 points OR "outside the
// subgroup" into the off-curve flags, which k_verify_prepare folds into the proof's verdict
int verify_batch(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof, const uint8_t* proofs_host, int* ok,
                 bool check_subgroup) {
    if (!ctx || !pk || !count || !proofs_host || !ok || count > PAIRING_MAX_LANES / 3) return ZK_ERR_ARG;
    if (!pk->gamma_abc || pk->gamma_abc->n == 0 || aff_is_inf<G2Field>(pk->gamma_g2))
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_verify_batch: the key has no verifying-key parts (gamma_g2, gamma_abc_g1)");
    const size_t ninp = inputs_per_proof;
    if (pk->gamma_abc->n != ninp + 1) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_verify_batch: inputs_per_proof is not num_instance - 1");
    if (ninp && !inputs_host) return ZK_ERR_ARG;
    for (size_t i = 0; i < count * ninp; i++)
        if (!zk_fr_words_valid(inputs_host[i].l)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_verify_batch: a public input is not below r");

    // host staging: the compressed G1 points (A_k, C_k), the compressed B_k, the key's constants
    struct Consts { uint32_t negs[2 * 48]; uint32_t want[GTW]; };
    std::vector<uint8_t> g1c(count * 2 * 48), g2c(count * 96);
    for (size_t k = 0; k < count; k++) {
        const uint8_t* pr = proofs_host + k * 192;
        memcpy(&g1c[(2 * k) * 48], pr, 48);
        memcpy(&g2c[k * 96], pr + 48, 96);
        memcpy(&g1c[(2 * k + 1) * 48], pr + 144, 48);
    }
    Consts cs;
    aff_store<G2Field>(cs.negs, aff_neg<G2Field>(pk->gamma_g2));
    aff_store<G2Field>(cs.negs + 48, aff_neg<G2Field>(pk->delta_g2));
    pk_e_alpha_beta(pk, cs.want);

    const size_t n = 3 * count;
    uint8_t *d_g1c, *d_g2c;
    uint32_t *d_in, *d_cs, *ac, *b, *flags, *P, *Q, *ml;
    int* d_ok;
    ZK_TRY(zk_scratch(ctx, "vfy_g1c", g1c.size(), (void**)&d_g1c));
    ZK_TRY(zk_scratch(ctx, "vfy_g2c", g2c.size(), (void**)&d_g2c));
    ZK_TRY(zk_scratch(ctx, "vfy_in", count * ninp * 32 + 32, (void**)&d_in));
    ZK_TRY(zk_scratch(ctx, "vfy_cs", sizeof cs, (void**)&d_cs));
    ZK_TRY(zk_scratch(ctx, "vfy_ac", count * 2 * 96, (void**)&ac));
    ZK_TRY(zk_scratch(ctx, "vfy_b", count * 192, (void**)&b));
    ZK_TRY(zk_scratch(ctx, "vfy_flags", (1 + 4 * count) * 4 + count * 4, (void**)&flags));      // any | bad_ac | bad_b | bad | ok
    ZK_TRY(zk_scratch(ctx, "pair_p", n * 96, (void**)&P));
    ZK_TRY(zk_scratch(ctx, "pair_q", n * 192, (void**)&Q));
    ZK_TRY(zk_scratch(ctx, "pair_ml", n * GTW * 4, (void**)&ml));
    uint32_t *bad_any = flags, *bad_ac = flags + 1, *bad_b = bad_ac + 2 * count, *bad = bad_b + count;
    d_ok = (int*)(bad + count);
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_g1c, g1c.data(), g1c.size(), hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_g2c, g2c.data(), g2c.size(), hipMemcpyHostToDevice, st));
    if (ninp) ZK_HIP(ctx, hipMemcpyAsync(d_in, inputs_host, count * ninp * 32, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_cs, &cs, sizeof cs, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemsetAsync(bad_any, 0, 4, st));
    ZK_TRY(zk_decompress_launch(ctx, 1, (const uint32_t*)d_g1c, 2 * count, ac, bad_any, bad_ac));
    ZK_TRY(zk_decompress_launch(ctx, 2, (const uint32_t*)d_g2c, count, b, bad_any, bad_b));
    if (check_subgroup) {
        ZK_TRY(zk_subgroup_launch(ctx, 1, ac, 2 * count, bad_any, bad_ac, true));
        ZK_TRY(zk_subgroup_launch(ctx, 2, b, count, bad_any, bad_b, true));
    }
    hipLaunchKernelGGL(k_verify_prepare, blocks64(count), 64, 0, st, count, ninp, (const uint32_t*)d_in, (const uint32_t*)pk->gamma_abc->dev,
                       (const uint32_t*)ac, (const uint32_t*)b, (const uint32_t*)d_cs, (const uint32_t*)bad_ac, (const uint32_t*)bad_b, P, Q, bad);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_miller<false>, blocks64(n), 64, 0, st, (const uint32_t*)P, (const uint32_t*)Q, n, ml);
    ZK_HIP(ctx, hipGetLastError());
    hipLaunchKernelGGL(k_pairing_finish, blocks64(count), 64, 0, st, (const uint32_t*)ml, (size_t)3, count, (uint32_t*)nullptr,
                       (const uint32_t*)(d_cs + 2 * 48), (const uint32_t*)bad, d_ok);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(ok, d_ok, count * sizeof(int), hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    return ZK_OK;
}
}  // namespace

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
extern "C" int zk_groth16_verify_batch(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                       const uint8_t* proofs_host, int* ok) {
    ZK_API_BEGIN(ctx)
    return verify_batch(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, ok, false);
    ZK_API_END
}
extern "C" int zk_groth16_verify_batch_checked(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                               const uint8_t* proofs_host, int* ok) {
    ZK_API_BEGIN(ctx)
    return verify_batch(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, ok, true);
    ZK_API_END
}

extern "C" int zk_diag_fq12_host(int op, const zk_gt* in_pairs, zk_gt* out, size_t n_cases) {
    ZK_API_BEGIN_NOCTX
    if (!in_pairs || !out || op < 0 || op > 7 || n_cases < 1 || n_cases > ((size_t)1 << 20)) return ZK_ERR_ARG;
    if (!zk_words_below_q((const uint64_t*)in_pairs, (int)(24 * n_cases))) return ZK_ERR_ARG;
    for (size_t i = 0; i < n_cases; i++) {
        uint32_t in[2 * GTW], o[GTW];
        memcpy(in, &in_pairs[2 * i], sizeof in);
        diag_fq12_op<H2>(op, in, o);
        memcpy(&out[i], o, sizeof o);
    }
    return ZK_OK;
    ZK_API_END
}
extern "C" int zk_diag_fq12_dev(zk_ctx* ctx, int op, const zk_gt* in_pairs, zk_gt* out, size_t n_cases) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in_pairs || !out || op < 0 || op > 7 || n_cases < 1 || n_cases > ((size_t)1 << 20)) return ZK_ERR_ARG;
    if (!zk_words_below_q((const uint64_t*)in_pairs, (int)(24 * n_cases))) return ZK_ERR_ARG;
    uint32_t *din, *dout;
    ZK_TRY(zk_scratch(ctx, "diag_fq12_in", n_cases * 2 * GTW * 4, (void**)&din));
    ZK_TRY(zk_scratch(ctx, "diag_fq12_out", n_cases * GTW * 4, (void**)&dout));
    ZK_HIP(ctx, hipMemcpyAsync(din, in_pairs, n_cases * 2 * GTW * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_diag_fq12, blocks64(n_cases), 64, 0, ctx->stream, op, (const uint32_t*)din, dout, n_cases);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(out, dout, n_cases * GTW * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
    ZK_API_END
}
