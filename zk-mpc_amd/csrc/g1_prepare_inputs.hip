// g1_prepare_inputs.hip -- Groth16's prepare_inputs for many proofs of one key as a FIXED-BASE sum: gamma_abc is fixed per key, so the
// key carries window multiples of every gamma_abc[j], j >= 1, and a prepared input costs additions only.
//
// Replaces (reference): prepare_inputs (arkworks/groth16/src/verifier.rs:18-33: g_ic = gamma_abc[0] + sum_j x_j gamma_abc[j + 1], one
// double-and-add multiplication per input).
//
// The recoding is g1_lincomb.cuh's: x + 0x888...8 = sum n_w 16^w, so x = sum (n_w - 8) 16^w with 64 digits in [-8, 7] (x < r < 2^253:
// the sum stays below 2^256 and there is no carry digit).  The table holds m 16^w gamma_abc[j] for m = 1 .. 8 as affine points:
// 64 windows x 8 entries x 96 B = 48 KiB per input, read from global memory (L2) by address; a digit's sign negates y.
//   k_g1_window_table     one table entry per lane: m P by a four-bit double-and-add, 4 w doublings, one inversion.
//   k_fr_recode           one input per lane: the reference's Montgomery form -> canonical words + 0x888...8 (8 words).
//   k_g1_prepare_inputs   a proof is a segment of L lanes, L a power of two <= 64 the same for the whole launch, so no segment
//                         straddles a wave (one wave per block).  Lane l takes the items t = l, l + L, ... of its proof's ninp x 64
//                         (input, window) items, t = 64 j + w -- a proof with more items than lanes loops inside the lane, it never
//                         takes more waves -- and accumulates in XYZZ with the COMPLETE mixed addition (accumulator at infinity,
//                         equal points, opposite points, a table entry at infinity); a zero digit is skipped.  A tree of complete
//                         additions through LDS (12 KiB: the tree only) sums the segment; its first lane adds gamma_abc[0] and
//                         writes the affine point and an infinity flag.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "groth16_int.hpp"

using namespace zk;

namespace {

constexpr uint32_t PREP_ITEMS_PER_LANE = 8;      // lanes per proof: the power of two that leaves a lane at most this many items, up to a wave

__global__ void __launch_bounds__(64) k_g1_window_table(const uint32_t* __restrict__ abc, size_t n_entries, uint32_t* __restrict__ win) {
    const size_t e = blockIdx.x * (size_t)64 + threadIdx.x;
    if (e >= n_entries) return;
    const size_t j = e / ZK_PREP_ENTRIES;
    const uint32_t w = (uint32_t)(e / 8 % ZK_PREP_WINDOWS), m = (uint32_t)(e % 8) + 1;
    const Affine<G1Field> p = aff_load16<G1Field>(abc, j + 1);
    XYZZ<G1Field> acc = xyzz_inf<G1Field>();
#pragma unroll 1
    for (int b = 3; b >= 0; b--) {
        acc = xyzz_dbl<G1Field>(acc);
        if ((m >> b) & 1) acc = xyzz_madd<G1Field>(acc, p);
    }
#pragma unroll 1
    for (uint32_t i = 0; i < 4 * w; i++) acc = xyzz_dbl<G1Field>(acc);
    aff_store16<G1Field>(win, e, xyzz_to_affine<G1Field>(acc));      // (infinity -- a gamma_abc entry at infinity, a torsion point -- is (0, 0))
}

__global__ void __launch_bounds__(256) k_fr_recode(const uint32_t* __restrict__ inputs, size_t n, uint32_t* __restrict__ digits) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    uint32_t k[8], carry = 0;
    fp_pack<FrParams>(k, fp_ext_to_canon<FrParams>(fr_load(inputs, i)));
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const uint64_t t = (uint64_t)k[q] + 0x88888888u + carry;
        k[q] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
    uint4* o = reinterpret_cast<uint4*>(digits) + 2 * i;
    o[0] = make_uint4(k[0], k[1], k[2], k[3]);
    o[1] = make_uint4(k[4], k[5], k[6], k[7]);
}

// proof k = lanes k L .. k L + L - 1 (L = 1 << log_l); digits: k_fr_recode's words of input (k, j) at 8 (k ninp + j)
__global__ void __launch_bounds__(64) k_g1_prepare_inputs(size_t count, uint32_t ninp, uint32_t log_l, const uint32_t* __restrict__ digits,
                                                          const uint32_t* __restrict__ win, const uint32_t* __restrict__ abc,
                                                          uint32_t* __restrict__ out_aff, uint32_t* __restrict__ out_inf) {
    __shared__ uint32_t lds[XW * 64];
    const uint32_t lane = threadIdx.x, L = 1u << log_l, l = lane & (L - 1);
    const size_t k = (blockIdx.x * (size_t)64 + lane) >> log_l;
    XYZZ<G1Field> acc = xyzz_inf<G1Field>();
    if (k < count) {
        const uint32_t items = ninp * (uint32_t)ZK_PREP_WINDOWS;
        const uint32_t* kd = digits + 8 * k * ninp;
#pragma unroll 1
        for (uint32_t t = l; t < items; t += L) {
            const uint32_t j = t / (uint32_t)ZK_PREP_WINDOWS, w = t % (uint32_t)ZK_PREP_WINDOWS;
            const int d = (int)((kd[8 * (size_t)j + (w >> 3)] >> (4 * (w & 7))) & 15u) - 8;
            if (d == 0) continue;
            Affine<G1Field> q = aff_load16<G1Field>(win, (size_t)t * 8 + (size_t)((d < 0 ? -d : d) - 1));
            if (d < 0) q = aff_neg<G1Field>(q);
            acc = xyzz_madd<G1Field>(acc, q);
        }
    }
    // the segmented tree: after step s the lane at offset 0 mod 2 s of its segment holds the sum of its 2 s lanes
    ZkLdsTab tab{lds + lane};
    tab.put(0, acc);
#pragma unroll 1
    for (uint32_t s = 1; s < L; s <<= 1) {
        __syncthreads();
        const bool act = (l & (2 * s - 1)) == 0;
        if (act) {
            ZkLdsTab other{lds + lane + s};
            acc = xyzz_add<G1Field>(acc, other.get(0));
        }
        __syncthreads();
        if (act) tab.put(0, acc);
    }
    if (l == 0 && k < count) {
        acc = xyzz_madd<G1Field>(acc, aff_load16<G1Field>(abc, 0));
        aff_store16<G1Field>(out_aff, k, xyzz_to_affine<G1Field>(acc));
        out_inf[k] = xyzz_is_inf<G1Field>(acc) ? 1u : 0u;
    }
}

}  // namespace

int zk_g1_window_table_launch(zk_ctx* ctx, const uint32_t* abc_dev, size_t ninp, uint32_t* win_dev) {
    const size_t n = ninp * ZK_PREP_ENTRIES;
    if (!n || !abc_dev || !win_dev || zk_blocks64(n) == 0 || n > ((size_t)1 << 36)) return ZK_ERR_ARG;
    hipLaunchKernelGGL(k_g1_window_table, zk_blocks64(n), 64, 0, ctx->stream, abc_dev, n, win_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int zk_g1_prepare_inputs_launch(zk_ctx* ctx, const uint32_t* inputs_dev, size_t count, size_t ninp, const uint32_t* win_dev, const uint32_t* abc_dev,
                                uint32_t* digits_dev, uint32_t* out_aff_dev, uint32_t* out_inf_dev) {
    if (!count || count > ZK_PAIRING_MAX_LANES || ninp > ((size_t)1 << 24) || !abc_dev || !out_aff_dev || !out_inf_dev) return ZK_ERR_ARG;
    if (ninp && (!inputs_dev || !win_dev || !digits_dev || count > ((size_t)1 << 30) / ninp)) return ZK_ERR_ARG;
    uint32_t log_l = 0;
    while (log_l < 6 && ((size_t)PREP_ITEMS_PER_LANE << log_l) < ninp * ZK_PREP_WINDOWS) log_l++;
    if (ninp) {
        const size_t n = count * ninp;
        hipLaunchKernelGGL(k_fr_recode, (unsigned)((n + 255) / 256), 256, 0, ctx->stream, inputs_dev, n, digits_dev);
        ZK_HIP(ctx, hipGetLastError());
    }
    hipLaunchKernelGGL(k_g1_prepare_inputs, zk_blocks64(count << log_l), 64, 0, ctx->stream, count, (uint32_t)ninp, log_l, (const uint32_t*)digits_dev,
                       win_dev, abc_dev, out_aff_dev, out_inf_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
