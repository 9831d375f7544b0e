// g1_ntt.hip -- a radix-2 transform over G1 POINTS: out[j] = sum_i w^(ij) P_i for 2^k points, `count` vectors under the same twiddles.
//
// No counterpart in the reference: it transforms scalars only.  zk_pk_derive_eval_h (groth16_key.hip) uses it to carry h_query through
// the transposes of coset_ifft and of ifft without the trapdoor -- the tables a loaded key needs for "H over coset values" (DESIGN 5).
//   * decimation in time: one launch loads the affine input into XYZZ form at its bit-reversed place (and, for the derive call, multiplies
//     point i by its pre-scale first); then one launch per level, one butterfly per lane (g1_ntt.cuh), the points staying in XYZZ form
//     in HBM between the levels; zk_g1_batch_affine_launch normalises once at the end;
//   * a butterfly is ~260 doublings and ~90 complete additions against two 192-byte loads and stores: compute-bound by three orders of
//     magnitude, so a level is not fused with its neighbours and a lane's accesses are plain 16-byte ones;
//   * the multiplication's table (four XYZZ entries per lane) is in LDS, word-interleaved across the wave (devutil.cuh: ZkLdsTab).
//     48 KiB per block of one wave: three blocks per CU.
//   * twiddles are 2^(k-1) raw 256-bit scalars (canonical Fr) computed on the host once per size and direction.
#include "../../include/zkmpc_hip.h"
#include "hostfr.hpp"
#include "g1_ntt.cuh"
#include "hostfield64.hpp"
#include "hostgroup.hpp"
#include "internal.hpp"
#include <string.h>
#include <vector>

using namespace zk;

namespace {

constexpr uint32_t DIAG_MAX_LOG = 12, DIAG_MAX_COUNT = 16;

struct HostTab {
    XYZZ<Fq64Field> t[G1NTT_TAB];
    void put(int e, const XYZZ<Fq64Field>& p) { t[e] = p; }
    XYZZ<Fq64Field> get(int e) const { return t[e]; }
};

__device__ __forceinline__ void load_scalar(uint32_t k[8], const uint32_t* base, size_t i) {
    const uint4* kp = reinterpret_cast<const uint4*>(base) + 2 * i;
    const uint4 a = kp[0], b = kp[1];
    k[0] = a.x; k[1] = a.y; k[2] = a.z; k[3] = a.w; k[4] = b.x; k[5] = b.y; k[6] = b.z; k[7] = b.w;
}

// lane g < count 2^log_n holds point i = g mod 2^log_n of vector v = g / 2^log_n: work[v 2^log_n + bitrev(i)] = (scale) in[v in_vstride + i]
template <bool SCALE>
__global__ void __launch_bounds__(64) k_g1_ntt_load(const uint32_t* __restrict__ in, uint32_t n_in, size_t in_vstride, ZkG1NttScale scale,
                                                    uint32_t log_n, size_t total, uint32_t* __restrict__ work) {
    __shared__ uint32_t lds[SCALE ? G1NTT_TAB * XW * 64 : 64];
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    if (g >= total) return;                                            // (no barrier below: a lane's table column is its own)
    const uint32_t i = (uint32_t)(g & (((size_t)1 << log_n) - 1));
    const size_t v = g >> log_n;
    XYZZ<G1Field> p = xyzz_inf<G1Field>();
    if (i < n_in) p = xyzz_from_affine<G1Field>(aff_load16<G1Field>(in, v * in_vstride + i));
    if (SCALE) {
        uint32_t k[8];
        load_scalar(k, scale.k, (size_t)scale.base[v] + (size_t)i * scale.step[v]);
        ZkLdsTab tab{lds + threadIdx.x};
        p = g1_ntt_mul<G1Field>(p, k, tab);
    }
    xyzz_store16<G1Field>(work, (v << log_n) + g1_ntt_bitrev(i, log_n), p);
}

// lane g < count 2^(log_n - 1) holds butterfly j = g mod 2^(log_n - 1) of level s of vector v
__global__ void __launch_bounds__(64) k_g1_ntt_level(uint32_t* __restrict__ work, const uint32_t* __restrict__ tw, uint32_t log_n, uint32_t s, size_t total) {
    __shared__ uint32_t lds[G1NTT_TAB * XW * 64];
    const size_t g = blockIdx.x * (size_t)64 + threadIdx.x;
    if (g >= total) return;
    const uint32_t j = (uint32_t)(g & (((size_t)1 << (log_n - 1)) - 1));
    const size_t v = g >> (log_n - 1);
    uint32_t lo, t, w[8];
    g1_ntt_pair(j, s, log_n, &lo, &t);
    const size_t ia = (v << log_n) + lo, ib = ia + ((size_t)1 << s);
    load_scalar(w, tw, t);
    XYZZ<G1Field> a = xyzz_load16<G1Field>(work, ia), b = xyzz_load16<G1Field>(work, ib);
    ZkLdsTab tab{lds + threadIdx.x};
    g1_ntt_butterfly<G1Field>(a, b, w, tab);
    xyzz_store16<G1Field>(work, ia, a);
    xyzz_store16<G1Field>(work, ib, b);
}

__global__ void __launch_bounds__(256) k_g1_sub(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t* __restrict__ out, size_t n) {
    const size_t i = blockIdx.x * (size_t)256 + threadIdx.x;
    if (i >= n) return;
    xyzz_store16<G1Field>(out, i, xyzz_madd<G1Field>(xyzz_from_affine<G1Field>(aff_load16<G1Field>(a, i)), aff_neg<G1Field>(aff_load16<G1Field>(b, i))));
}

// w^t for t < 2^(log_n - 1) as raw scalars (canonical integers, 8 words each); w the domain generator of ntt.hip or its inverse
std::vector<uint32_t> twiddle_words(uint32_t log_n, int inverse_root) {
    Fr w = HF::domain_root(log_n).v;
    if (inverse_root) w = fp_inv<FrParams>(w);
    const size_t half = log_n ? (size_t)1 << (log_n - 1) : 1;
    std::vector<uint32_t> out(half * 8);
    Fr p = fp_one<FrParams>();
    for (size_t t = 0; t < half; t++) {
        fp_pack<FrParams>(&out[8 * t], fp_int_to_canon<FrParams>(p));
        p = fp_mul<FrParams>(p, w);
    }
    return out;
}

// what both test hooks refuse
bool diag_args_ok(const zk_g1_affine* points, uint32_t log_n, size_t count, const zk_g1_affine* out) {
    if (!points || !out || log_n > DIAG_MAX_LOG || !count || count > DIAG_MAX_COUNT) return false;
    for (size_t i = 0; i < count << log_n; i++)
        if (!zk_words_below_q((const uint64_t*)&points[i], 2)) return false;
    return true;
}

}  // namespace

int zk_g1_ntt_twiddles(zk_ctx* ctx, uint32_t log_n, int inverse_root, const uint32_t** twiddles_dev) {
    if (log_n > (uint32_t)FR_TWO_ADICITY) return ZK_ERR_ARG;
    const std::vector<uint32_t> tw = twiddle_words(log_n, inverse_root);
    void* d;
    ZK_TRY(zk_scratch(ctx, "g1ntt_tw", tw.size() * 4, &d));
    ZK_HIP(ctx, hipMemcpyAsync(d, tw.data(), tw.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));                     // (tw is a local)
    *twiddles_dev = (const uint32_t*)d;
    return ZK_OK;
}

int zk_g1_ntt_launch(zk_ctx* ctx, const uint32_t* in_dev, size_t n_in, size_t in_vstride, const ZkG1NttScale* scale, uint32_t log_n, size_t count,
                     const uint32_t* twiddles_dev, uint32_t* work_xyzz_dev) {
    const size_t n = (size_t)1 << log_n, total = count * n;
    if (!in_dev || !twiddles_dev || !work_xyzz_dev || log_n > 26 || !count || total > ((size_t)1 << 28) || n_in > n || (scale && (count > 2 || !scale->k)))
        return ZK_ERR_ARG;
    const unsigned blocks = zk_blocks64(total);
    if (scale) hipLaunchKernelGGL(k_g1_ntt_load<true>, blocks, 64, 0, ctx->stream, in_dev, (uint32_t)n_in, in_vstride, *scale, log_n, total, work_xyzz_dev);
    else hipLaunchKernelGGL(k_g1_ntt_load<false>, blocks, 64, 0, ctx->stream, in_dev, (uint32_t)n_in, in_vstride, ZkG1NttScale{}, log_n, total, work_xyzz_dev);
    for (uint32_t s = 0; s < log_n; s++)
        hipLaunchKernelGGL(k_g1_ntt_level, zk_blocks64(total / 2), 64, 0, ctx->stream, work_xyzz_dev, twiddles_dev, log_n, s, total / 2);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int zk_g1_sub_launch(zk_ctx* ctx, const uint32_t* a, const uint32_t* b, uint32_t* out, size_t n) {
    if (!n) return ZK_OK;
    hipLaunchKernelGGL(k_g1_sub, (unsigned)((n + 255) / 256), 256, 0, ctx->stream, a, b, out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

extern "C" int zk_diag_g1_ntt_host(const zk_g1_affine* points, uint32_t log_n, size_t count, int inverse_root, zk_g1_affine* out) {
    ZK_API_BEGIN_NOCTX
    if (!diag_args_ok(points, log_n, count, out)) return ZK_ERR_ARG;
    using H = Fq64Field;
    const size_t n = (size_t)1 << log_n;
    const std::vector<uint32_t> tw = twiddle_words(log_n, inverse_root);
    std::vector<XYZZ<H>> work(n);
    for (size_t v = 0; v < count; v++) {
        for (size_t i = 0; i < n; i++) {
            uint32_t w[24];
            memcpy(w, &points[v * n + i], 96);
            work[g1_ntt_bitrev((uint32_t)i, log_n)] = xyzz_from_affine<H>(Affine<H>{H::load(w), H::load(w + 12)});
        }
        for (uint32_t s = 0; s < log_n; s++)
            for (uint32_t j = 0; j < n / 2; j++) {
                uint32_t lo, t;
                g1_ntt_pair(j, s, log_n, &lo, &t);
                HostTab tab;
                g1_ntt_butterfly<H>(work[lo], work[lo + ((size_t)1 << s)], &tw[8 * (size_t)t], tab);
            }
        for (size_t i = 0; i < n; i++) {
            const Affine<H> a = xyzz_to_affine<H>(work[i]);
            uint32_t w[24];
            H::store(w, a.x);
            H::store(w + 12, a.y);
            memcpy(&out[v * n + i], w, 96);
        }
    }
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_diag_g1_ntt_dev(zk_ctx* ctx, const zk_g1_affine* points, uint32_t log_n, size_t count, int inverse_root, zk_g1_affine* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !diag_args_ok(points, log_n, count, out)) return ZK_ERR_ARG;
    const size_t n = (size_t)1 << log_n, total = count * n;
    std::vector<uint32_t> pts(total * 24);
    for (size_t i = 0; i < total; i++) aff_store<G1Field>(&pts[24 * i], host_aff_from_abi<G1Field>((const uint64_t*)&points[i]));
    uint32_t *d_in, *d_work, *d_scr, *d_out;
    const uint32_t* d_tw;
    ZK_TRY(zk_scratch(ctx, "g1ntt_diag_in", total * 96, (void**)&d_in));
    ZK_TRY(zk_scratch(ctx, "g1ntt_diag_work", total * 192, (void**)&d_work));
    ZK_TRY(zk_scratch(ctx, "g1ntt_diag_scr", total * 48, (void**)&d_scr));
    ZK_TRY(zk_scratch(ctx, "g1ntt_diag_out", total * 96, (void**)&d_out));
    ZK_TRY(zk_g1_ntt_twiddles(ctx, log_n, inverse_root, &d_tw));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_in, pts.data(), pts.size() * 4, hipMemcpyHostToDevice, st));
    ZK_TRY(zk_g1_ntt_launch(ctx, d_in, n, n, nullptr, log_n, count, d_tw, d_work));
    ZK_TRY(zk_g1_batch_affine_launch(ctx, d_work, d_out, d_scr, total));
    ZK_HIP(ctx, hipMemcpyAsync(pts.data(), d_out, pts.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    for (size_t i = 0; i < total; i++) host_aff_to_abi<G1Field>((uint64_t*)&out[i], aff_load<G1Field>(&pts[24 * i]));
    return ZK_OK;
    ZK_API_END
}
