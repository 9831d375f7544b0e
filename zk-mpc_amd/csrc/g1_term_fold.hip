// g1_term_fold.hip -- the sum of MANY G1 terms k_g P_g with full-width scalars, every term its own point: one term per lane, one wave
// per block, one XYZZ partial per block (the partials go down through zk_g1_sum_down and the last 64 are added on the host).
//
// Replaces (reference): the commitment side of KZG10::batch_check (poly-commit/src/kzg10/mod.rs:345-389: total_c += comm * randomizer
// ... over every equation) for a batch of Marlin proofs, where marlin_verify.hip has regrouped the sum by POINT: 13 count + 16 points
// that belong to no resident table, each with one scalar rho c mod r.  The MSM pipeline (msm.hip) wants one table and long vectors;
// k_g1_lincomb (g1_lincomb.hip) sums within segments of at most a wave; k_g1_scale_fold (groth16_verify.hip) has this shape with
// 128-bit coefficients.  The kernel here is two things that run on the device already, composed:
//   * the per-lane term of g1_lincomb.cuh -- fixed signed 4-bit windows, the digit selects a table entry in LDS and a sign, never the
//     control flow, so every lane of a wave runs the same schedule whatever its scalar is;
//   * the wave tree of k_g1_scale_fold: complete additions (equal points double, opposite points cancel, infinity passes) through
//     entry 0 of the LDS tables.
// Two instantiations behind one launch function:
//   ZK_TERM_FULL  lincomb_term<G1Field, ZkLdsTab, 8>: the words are 256 raw bits, 64 windows, any curve point -- exactly the body of
//                 k_g1_lincomb in front of exactly the tree of k_g1_scale_fold;
//   ZK_TERM_GLV   lincomb_term_glv: the words are k1 | k2 (128 raw bits each), 32 windows of two additions, the second operand
//                 through phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ) -- for points of the prime-order subgroup only.
// Both take LINCOMB_TAB XW 64 4 = 98 304 bytes of dynamic LDS (eight XYZZ entries per lane, word-interleaved: devutil.cuh ZkLdsTab).
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "g1_lincomb.cuh"
#include "hostfield64.hpp"
#include "hostgroup.hpp"
#include "internal.hpp"
#include "marlin_agg_plan.hpp"
#include <string.h>
#include <vector>

using namespace zk;

namespace zk {
template <> struct GlvBeta<G1Field> {
    static ZK_HD Fq get() { return fp_const<FqParams>(FqParams::BETA); }
};
}  // namespace zk

namespace {

constexpr size_t TERM_LDS = (size_t)LINCOMB_TAB * XW * 64 * 4;       // 98 304 bytes
constexpr size_t TERM_MAX_LANES = (size_t)1 << 22;

// lane g < n: point g in_step of `in` times words[8 g ..]; lanes beyond n carry infinity and a zero scalar (they load nothing and
// store nothing).  out_aff (or NULL): the n products as affine points.  out_part (or NULL): one XYZZ sum per block.
template <int MODE>
__global__ void __launch_bounds__(64) k_g1_term_fold(const uint32_t* __restrict__ in, uint32_t in_step, const uint32_t* __restrict__ words, uint32_t n,
                                                     uint32_t* __restrict__ out_aff, uint32_t* __restrict__ out_part) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane;
    ZkLdsTab tab{lds + lane};
    Affine<G1Field> p = aff_inf<G1Field>();
    uint32_t k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (g < n) {
        p = aff_load16<G1Field>(in, (size_t)g * in_step);
        const uint4* kp = reinterpret_cast<const uint4*>(words) + 2 * (size_t)g;
        const uint4 a = kp[0], b = kp[1];
        k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
    }
    XYZZ<G1Field> acc;
    if constexpr (MODE == ZK_TERM_GLV) acc = lincomb_term_glv<G1Field, ZkLdsTab>(p, k, k + 4, tab);
    else acc = lincomb_term<G1Field, ZkLdsTab, 8>(p, k, tab);
    __syncthreads();                                                   // (the tree reuses entry 0 of the tables)
    if (out_aff && g < n) aff_store16<G1Field>(out_aff, g, xyzz_to_affine<G1Field>(acc));
    if (!out_part) return;
    // the tree of k_g1_scale_fold
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

template <int MODE>
int term_fold_launch(zk_ctx* ctx, ZkLdsAttr slot, const uint32_t* in, uint32_t in_step, const uint32_t* words, size_t n, uint32_t* out_aff,
                     uint32_t* out_part) {
    if (!ctx->lds_attr_done[slot]) {
        ZK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_g1_term_fold<MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)TERM_LDS));
        ctx->lds_attr_done[slot] = true;
    }
    hipLaunchKernelGGL(k_g1_term_fold<MODE>, zk_blocks64(n), 64, TERM_LDS, ctx->stream, in, in_step, words, (uint32_t)n, out_aff, out_part);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

}  // namespace

int zk_g1_term_fold_launch(zk_ctx* ctx, int mode, const uint32_t* in, uint32_t in_step, const uint32_t* words, size_t n, uint32_t* out_aff,
                           uint32_t* out_part) {
    if (!in || !words || !n || n > TERM_MAX_LANES || !in_step) return ZK_ERR_ARG;
    if (mode == ZK_TERM_FULL) return term_fold_launch<ZK_TERM_FULL>(ctx, ZK_LDS_TERM_FOLD_FULL, in, in_step, words, n, out_aff, out_part);
    if (mode == ZK_TERM_GLV) return term_fold_launch<ZK_TERM_GLV>(ctx, ZK_LDS_TERM_FOLD_GLV, in, in_step, words, n, out_aff, out_part);
    return ZK_ERR_ARG;
}

extern "C" int zk_diag_g1_term_sum_dev(zk_ctx* ctx, const zk_g1_affine* pts, const uint32_t* words, size_t n, int mode, zk_g1_affine* scaled_out,
                                       zk_g1_projective* sum_out) {
    ZK_API_BEGIN(ctx)
    using H1 = Fq64Field;
    if (!ctx || !pts || !words || !sum_out || !n || n > TERM_MAX_LANES || (mode != ZK_TERM_FULL && mode != ZK_TERM_GLV)) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&pts[i], 2)) return ZK_ERR_ARG;
    std::vector<uint32_t> w(n * 24);
    for (size_t i = 0; i < n; i++) aff_store<G1Field>(&w[24 * i], host_aff_from_abi<G1Field>((const uint64_t*)&pts[i]));
    const ZkSumPlan sp = zk_sum_plan(n);
    uint32_t *d_pts, *d_words, *d_aff = nullptr, *part_a, *part_b;
    ZK_TRY(zk_scratch(ctx, "term_diag_pts", n * AGG_AFF_BYTES, (void**)&d_pts));
    ZK_TRY(zk_scratch(ctx, "term_diag_words", n * 32, (void**)&d_words));
    if (scaled_out) ZK_TRY(zk_scratch(ctx, "term_diag_aff", n * AGG_AFF_BYTES, (void**)&d_aff));
    ZK_TRY(zk_scratch(ctx, "term_part_a", sp.part_a * AGG_XYZZ_BYTES, (void**)&part_a));
    ZK_TRY(zk_scratch(ctx, "term_part_b", sp.part_b * AGG_XYZZ_BYTES, (void**)&part_b));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_pts, w.data(), n * AGG_AFF_BYTES, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_words, words, n * 32, hipMemcpyHostToDevice, st));
    ZkPhaseTimer tm(ctx);                          // with zk_set_profiling: the kernel and its sum-down by device events (the A/B of the modes)
    tm.begin(mode == ZK_TERM_GLV ? "diag_term_sum.k_term_fold_glv" : "diag_term_sum.k_term_fold_full");
    ZK_TRY(zk_g1_term_fold_launch(ctx, mode, d_pts, 1, d_words, n, d_aff, part_a));
    size_t m = sp.blocks;
    uint32_t* part;
    ZK_TRY(zk_g1_sum_down(ctx, part_a, part_b, &m, &part));
    tm.end();
    if (m != sp.left) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_diag_g1_term_sum_dev: the sum-down left another count than its plan");
    std::vector<uint32_t> h_part(m * XW);
    ZK_HIP(ctx, hipMemcpyAsync(h_part.data(), part, h_part.size() * 4, hipMemcpyDeviceToHost, st));
    if (scaled_out) ZK_HIP(ctx, hipMemcpyAsync(w.data(), d_aff, n * AGG_AFF_BYTES, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    tm.resolve();
    XYZZ<H1> sum = xyzz_inf<H1>();
    for (size_t i = 0; i < m; i++) sum = xyzz_add<H1>(sum, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_part[i * XW])));
    host64_write_projective<H1>(xyzz_to_affine<H1>(sum), (uint64_t*)sum_out);
    if (scaled_out)
        for (size_t i = 0; i < n; i++) host_aff_to_abi<G1Field>((uint64_t*)&scaled_out[i], aff_load<G1Field>(&w[24 * i]));
    return ZK_OK;
    ZK_API_END
}
