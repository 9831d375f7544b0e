// g1_lincomb.hip -- many SHORT linear combinations of G1 points in one launch: segment s = sum k_t P_t over its (at most 64) terms,
// different points and full-width scalars in every segment.
//
// Replaces (reference): the commitment arithmetic of MarlinKZG10::check_combinations -- LinearCombination over commitments,
// accumulate_commitments_and_values (arkworks/poly-commit/src/marlin/mod.rs:33-118, :309-420, marlin_pc/mod.rs:342-400) -- and the
// subgroup test of GroupAffine::deserialize (ec/src/models/short_weierstrass_jacobian.rs:171-183, :888-905: r P == O), as a batch.
// The MSM pipeline (msm.hip) is for long vectors over one table; k_g1_prepare_inputs (g1_prepare_inputs.hip) is for sums over ONE
// table that carries its window multiples.  Here:
//   * one TERM per lane, one wave per block.  The caller's segments are packed into waves so that none straddles one
//     (ZkLincombPack); the lanes left over in a wave join the segment before them with a zero scalar;
//   * the per-lane multiplication is g1_lincomb.cuh: fixed signed 4-bit windows, the same doublings and one addition per window on
//     every lane, table of 8 XYZZ entries per lane in LDS (8 x 192 B x 64 lanes = 96 KiB of the CU's 160), word-interleaved across the
//     lanes (devutil.cuh: ZkLdsTab);
//   * a segmented tree over the wave through LDS with the complete addition (equal points double, opposite points cancel); the
//     segment's first lane converts to affine (one inversion) and writes the point and an infinity flag.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "g1_lincomb.cuh"
#include "hostfield64.hpp"
#include "hostgroup.hpp"
#include "internal.hpp"
#include <string.h>
#include <vector>

using namespace zk;

namespace {

constexpr size_t LINCOMB_LDS = (size_t)LINCOMB_TAB * XW * 64 * 4;     // 98 304 bytes

struct HostTab {
    XYZZ<Fq64Field> t[LINCOMB_TAB];
    void put(int e, const XYZZ<Fq64Field>& p) { t[e] = p; }
    XYZZ<Fq64Field> get(int e) const { return t[e]; }
};

// lane g (< n_lanes) holds term g: point point_index[g] of `points` (table form; an index >= n_points counts as infinity) times
// scalars[8 g ..]; segment s is the lanes seg_off[s] .. seg_off[s + 1] - 1, all within one wave; seg_off[0] = 0, seg_off[n_seg] = n_lanes.
__global__ void __launch_bounds__(64) k_g1_lincomb(const uint32_t* __restrict__ points, uint32_t n_points, const uint32_t* __restrict__ point_index,
                                                   const uint32_t* __restrict__ scalars, const uint32_t* __restrict__ seg_off, uint32_t n_seg,
                                                   uint32_t n_lanes, uint32_t* __restrict__ out_aff, uint32_t* __restrict__ out_inf) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, wave0 = blockIdx.x * 64u, g = wave0 + lane;
    uint32_t s_lo = g, s_hi = g + 1, seg = n_seg, k[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    Affine<G1Field> p = aff_inf<G1Field>();
    if (g < n_lanes) {
        uint32_t lo = 0, hi = n_seg;                                   // the last s with seg_off[s] <= g
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (seg_off[mid] <= g) lo = mid; else hi = mid;
        }
        seg = lo;
        s_lo = max(seg_off[lo], wave0);
        s_hi = min(seg_off[lo + 1], wave0 + 64u);
        const uint4* kp = reinterpret_cast<const uint4*>(scalars) + 2 * (size_t)g;
        const uint4 a = kp[0], b = kp[1];
        k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
        const uint32_t pi = point_index[g];
        if (pi < n_points) p = aff_load16<G1Field>(points, pi);
    }
    ZkLdsTab tab{lds + lane};
    XYZZ<G1Field> acc = lincomb_term<G1Field>(p, k, tab);
    // the segmented tree: after step s the lane at offset 0 mod 2 s of its segment holds the sum of its 2 s lanes
    uint32_t* red = lds;                                               // entry 0 of every lane's table, reused
    __syncthreads();
    tab.put(0, acc);
#pragma unroll 1
    for (uint32_t s = 1; s < 64; s <<= 1) {
        __syncthreads();
        const bool act = (((g - s_lo) & (2 * s - 1)) == 0) && g + s < s_hi;
        if (act) {
            ZkLdsTab other{red + lane + s};
            acc = xyzz_add<G1Field>(acc, other.get(0));
        }
        __syncthreads();
        if (act) tab.put(0, acc);
    }
    if (seg < n_seg && g == s_lo) {
        aff_store16<G1Field>(out_aff, seg, xyzz_to_affine<G1Field>(acc));
        out_inf[seg] = xyzz_is_inf<G1Field>(acc) ? 1u : 0u;
    }
}

// what both test hooks refuse
bool diag_args_ok(const zk_g1_affine* points, size_t n_points, const uint32_t* point_index, const uint32_t* scalars, const uint32_t* seg_offsets,
                  size_t n_segments, const zk_g1_affine* out) {
    if (!points || !point_index || !scalars || !seg_offsets || !out || !n_points || n_points > ((size_t)1 << 20) || !n_segments ||
        n_segments > ((size_t)1 << 20) || seg_offsets[0] != 0)
        return false;
    for (size_t s = 0; s < n_segments; s++)
        if (seg_offsets[s + 1] < seg_offsets[s] || seg_offsets[s + 1] - seg_offsets[s] > (uint32_t)LINCOMB_MAX_TERMS) return false;
    if (seg_offsets[n_segments] > (1u << 22)) return false;
    for (size_t t = 0; t < seg_offsets[n_segments]; t++)
        if (point_index[t] >= n_points) return false;
    for (size_t i = 0; i < n_points; i++)
        if (!zk_words_below_q((const uint64_t*)&points[i], 2)) return false;
    return true;
}

}  // namespace

bool ZkLincombPack::add(const uint32_t* idx, const uint32_t* k8, size_t len) {
    if (len > (size_t)LINCOMB_MAX_TERMS) return false;
    const size_t need = len ? len : 1, used = lanes() % 64;
    if (used + need > 64) {                                            // the rest of this wave joins the segment before, scalar 0
        point_index.resize(lanes() + (64 - used), 0u);
        scalars.resize(point_index.size() * 8, 0u);
    }
    seg_off.push_back((uint32_t)lanes());
    for (size_t t = 0; t < len; t++) {
        point_index.push_back(idx[t]);
        scalars.insert(scalars.end(), k8 + 8 * t, k8 + 8 * t + 8);
    }
    if (!len) {                                                        // an empty sum: one idle lane
        point_index.push_back(0u);
        scalars.resize(point_index.size() * 8, 0u);
    }
    return true;
}

int zk_g1_lincomb_launch(zk_ctx* ctx, const uint32_t* points_dev, size_t n_points, const uint32_t* point_index_dev, const uint32_t* scalars_dev,
                         const uint32_t* seg_offsets_dev, size_t n_segments, size_t n_lanes, uint32_t* out_affine_dev, uint32_t* out_is_inf_dev,
                         hipStream_t st) {
    if (!n_segments || !n_lanes || n_lanes > ((size_t)1 << 30) || n_segments > n_lanes || n_points > ((size_t)1 << 30)) return ZK_ERR_ARG;
    if (!ctx->lds_attr_done[ZK_LDS_LINCOMB]) {
        ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_g1_lincomb, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LINCOMB_LDS));
        ctx->lds_attr_done[ZK_LDS_LINCOMB] = true;
    }
    hipLaunchKernelGGL(k_g1_lincomb, zk_blocks64(n_lanes), 64, LINCOMB_LDS, st ? st : ctx->stream, points_dev, (uint32_t)n_points, point_index_dev,
                       scalars_dev, seg_offsets_dev, (uint32_t)n_segments, (uint32_t)n_lanes, out_affine_dev, out_is_inf_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

// what the GLV hook refuses
static bool glv_diag_args_ok(const zk_g1_affine* pts, const uint32_t* halves, size_t n, const zk_g1_projective* sum_out) {
    if (!pts || !halves || !sum_out || !n || n > ((size_t)1 << 22)) return false;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&pts[i], 2)) return false;
    return true;
}

extern "C" int zk_diag_g1_glv_sum_host(const zk_g1_affine* pts, const uint32_t* halves, size_t n, zk_g1_affine* scaled_out, zk_g1_projective* sum_out) {
    ZK_API_BEGIN_NOCTX
    if (!glv_diag_args_ok(pts, halves, n, sum_out)) return ZK_ERR_ARG;
    using H = Fq64Field;
    XYZZ<H> sum = xyzz_inf<H>();
    for (size_t i = 0; i < n; i++) {
        uint32_t w[24];
        memcpy(w, &pts[i], 96);
        HostTab tab;
        const XYZZ<H> t = lincomb_term_glv<H>(Affine<H>{H::load(w), H::load(w + 12)}, halves + 8 * i, halves + 8 * i + 4, tab);
        sum = xyzz_add<H>(sum, t);
        if (scaled_out) {
            const Affine<H> a = xyzz_to_affine<H>(t);
            H::store(w, a.x);
            H::store(w + 12, a.y);
            memcpy(&scaled_out[i], w, 96);
        }
    }
    host64_write_projective<H>(xyzz_to_affine<H>(sum), (uint64_t*)sum_out);
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_diag_g1_lincomb_host(const zk_g1_affine* points, size_t n_points, const uint32_t* point_index, const uint32_t* scalars,
                                       const uint32_t* seg_offsets, size_t n_segments, zk_g1_affine* out) {
    ZK_API_BEGIN_NOCTX
    if (!diag_args_ok(points, n_points, point_index, scalars, seg_offsets, n_segments, out)) return ZK_ERR_ARG;
    using H = Fq64Field;
    for (size_t s = 0; s < n_segments; s++) {
        XYZZ<H> sum = xyzz_inf<H>();
        for (uint32_t t = seg_offsets[s]; t < seg_offsets[s + 1]; t++) {
            uint32_t w[24];
            memcpy(w, &points[point_index[t]], 96);
            HostTab tab;
            sum = xyzz_add<H>(sum, lincomb_term<H>(Affine<H>{H::load(w), H::load(w + 12)}, scalars + 8 * (size_t)t, tab));
        }
        const Affine<H> a = xyzz_to_affine<H>(sum);
        uint32_t w[24];
        H::store(w, a.x);
        H::store(w + 12, a.y);
        memcpy(&out[s], w, 96);
    }
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_diag_g1_lincomb_dev(zk_ctx* ctx, const zk_g1_affine* points, size_t n_points, const uint32_t* point_index, const uint32_t* scalars,
                                      const uint32_t* seg_offsets, size_t n_segments, zk_g1_affine* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !diag_args_ok(points, n_points, point_index, scalars, seg_offsets, n_segments, out)) return ZK_ERR_ARG;
    ZkLincombPack pk;
    for (size_t s = 0; s < n_segments; s++)
        if (!pk.add(point_index + seg_offsets[s], scalars + 8 * (size_t)seg_offsets[s], seg_offsets[s + 1] - seg_offsets[s])) return ZK_ERR_ARG;
    pk.finish();
    std::vector<uint32_t> pts(n_points * 24);
    for (size_t i = 0; i < n_points; i++) aff_store<G1Field>(&pts[24 * i], host_aff_from_abi<G1Field>((const uint64_t*)&points[i]));
    uint32_t *d_pts, *d_idx, *d_k, *d_off, *d_out, *d_inf;
    ZK_TRY(zk_scratch(ctx, "lc_diag_pts", pts.size() * 4, (void**)&d_pts));
    ZK_TRY(zk_scratch(ctx, "lc_diag_idx", pk.point_index.size() * 4, (void**)&d_idx));
    ZK_TRY(zk_scratch(ctx, "lc_diag_k", pk.scalars.size() * 4, (void**)&d_k));
    ZK_TRY(zk_scratch(ctx, "lc_diag_off", pk.seg_off.size() * 4, (void**)&d_off));
    ZK_TRY(zk_scratch(ctx, "lc_diag_out", n_segments * 96, (void**)&d_out));
    ZK_TRY(zk_scratch(ctx, "lc_diag_inf", n_segments * 4, (void**)&d_inf));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_pts, pts.data(), pts.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_idx, pk.point_index.data(), pk.point_index.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_k, pk.scalars.data(), pk.scalars.size() * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_off, pk.seg_off.data(), pk.seg_off.size() * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(zk_g1_lincomb_launch(ctx, d_pts, n_points, d_idx, d_k, d_off, n_segments, pk.lanes(), d_out, d_inf));
    std::vector<uint32_t> res(n_segments * 24), inf(n_segments);
    ZK_HIP(ctx, hipMemcpyAsync(res.data(), d_out, res.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(inf.data(), d_inf, inf.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    for (size_t s = 0; s < n_segments; s++) {
        const Affine<G1Field> a = aff_load<G1Field>(&res[24 * s]);
        if ((inf[s] != 0) != aff_is_inf<G1Field>(a)) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_diag_g1_lincomb_dev: the infinity flag and the point disagree");
        host_aff_to_abi<G1Field>((uint64_t*)&out[s], a);
    }
    return ZK_OK;
    ZK_API_END
}
