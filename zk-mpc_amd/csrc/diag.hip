// diag.hip -- diagnostics a measurement needs from the device it runs on (not on any proving path).
//
// zk_diag_int_mad_peak: the issue rate of v_mad_u64_u32 on THIS device, measured when asked -- the roof the MSM kernels are
// priced against ("achieved int-mul-add/s vs measured peak of a pure v_mad_u64_u32 microbenchmark").  Eight
// independent 64-bit accumulator chains per lane, 32 768 rounds, 2 048 blocks of 256 lanes (two blocks per SIMD's worth of
// wave slots on 256 CUs): 1.4e11 lane multiply-adds per launch, ~4.4 ms -- long enough for the clocks to settle.  Same kernel as tools/ubench_int.hip::k_mad64.
//
// zk_diag_fq_pow_dev / zk_diag_fr_pow_dev: base^e as a square-and-multiply chain of DEVICE products -- hundreds of dependent
// Montgomery products through the same fp29.cuh templates the kernels run, in the exact or in the lazy domain.  They exist so that
// the two long-chain known answers the reference's own tests hold (GENERATOR^T == TWO_ADIC_ROOT_OF_UNITY:
// arkworks/curves/bls12_377/src/fields/tests.rs:352-370 for Fq, the same relation from fr.rs's constants for Fr) run on the GPU.
//
// zk_diag_fq_lazy_dev / zk_diag_fr_lazy_dev / zk_diag_fq2_pair_dev / zk_diag_f7l_dev: the lazy-domain arithmetic of the kernels as the
// device code object compiles it (fp29.cuh's PIN is on only there), a batch of cases in one small launch, raw 29-bit limbs in and
// out -- the device counterparts of hostapi.hip's zk_fq_lazy_raw / zk_fr_lazy_raw, for tests that put every range end through it.
// Every case array is padded to whole waves of 64 lanes with all-zero cases: the lane-pair and lane-quad forms exchange operands by
// DPP, and a pair or quad whose partner were an inactive lane would read nothing from it.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "ec.cuh"
#include "frlazy.cuh"
#include "internal.hpp"
#include <algorithm>
#include <vector>

using namespace zk;

namespace {

struct DiagExp { uint32_t w[12]; };

// lane 0 of one wave walks the exponent from its top bit down (Field::pow, ff/src/fields/mod.rs: square, then multiply on a set
// bit); in / out in the reference's Montgomery form.  lazy: products without the final subtraction (fp_mul_lazy: what the
// accumulate kernels run), one canonicalisation at the end.
__global__ void __launch_bounds__(64) k_diag_fq_pow(const uint32_t* base12, DiagExp e, int nbits, int lazy, uint32_t* out12) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    using F = FqField;
    const Fq b = F::ext_to_int(F::load(base12));
    Fq r = F::one();
    bool started = false;
    for (int i = nbits - 1; i >= 0; i--) {
        if (started) r = lazy ? F::sqr_l(r) : F::sqr(r);
        if ((e.w[i >> 5] >> (i & 31)) & 1) { r = started ? (lazy ? F::mul_l(r, b) : F::mul(r, b)) : b; started = true; }
    }
    if (lazy) r = F::canon(r);
    F::store(out12, F::int_to_ext(r));
}
__global__ void __launch_bounds__(64) k_diag_fr_pow(const uint32_t* base8, DiagExp e, int nbits, int lazy, uint32_t* out8) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    const Fr b = fp_ext_to_int<FrParams>(fr_load(base8, 0));
    Fr r = fp_one<FrParams>();
    bool started = false;
    for (int i = nbits - 1; i >= 0; i--) {
        if (started) r = lazy ? frl_mul(r, frl_canon(r)) : fp_sqr<FrParams>(r);     // frl_mul takes a table entry (< r) on the right
        if ((e.w[i >> 5] >> (i & 31)) & 1) { r = started ? (lazy ? frl_mul(r, b) : fr_mul(r, b)) : b; started = true; }
    }
    if (lazy) r = frl_canon(r);
    fr_store(out8, 0, fp_int_to_ext<FrParams>(r));
}

constexpr int DIAG_ITERS = 32768;
constexpr int DIAG_CH = 8;

__global__ void __launch_bounds__(256) k_diag_mad64(uint64_t* out, uint32_t a, uint32_t b) {
    uint64_t acc[DIAG_CH];
    const uint32_t x = a + threadIdx.x, y = b + blockIdx.x;
#pragma unroll
    for (int c = 0; c < DIAG_CH; c++) acc[c] = threadIdx.x + c;
    for (int i = 0; i < DIAG_ITERS; i++) {
#pragma unroll
        for (int c = 0; c < DIAG_CH; c++)
            asm volatile("v_mad_u64_u32 %0, vcc, %1, %2, %0" : "+v"(acc[c]) : "v"(x), "v"(y) : "vcc");
    }
    uint64_t s = 0;
#pragma unroll
    for (int c = 0; c < DIAG_CH; c++) s += acc[c];
    out[blockIdx.x * blockDim.x + threadIdx.x] = s;
}

}  // namespace

extern "C" int zk_diag_int_mad_peak(zk_ctx* ctx, int launches, double* best_mads_per_s, double* median_mads_per_s) {
    ZK_API_BEGIN(ctx)
    if (!ctx || launches < 1 || launches > 1000 || (!best_mads_per_s && !median_mads_per_s)) return ZK_ERR_ARG;
    const unsigned blocks = (unsigned)ctx->n_cu * 8, threads = 256;
    uint64_t* out;
    ZK_TRY(zk_scratch(ctx, "diag_out", (size_t)blocks * threads * 8, (void**)&out));
    hipStream_t st = ctx->stream;
    ZkEvent e0(0), e1(0);                                          // (flags 0: events that keep time)
    const double mads = (double)blocks * threads * DIAG_ITERS * DIAG_CH;
    std::vector<double> rate;
    int rc = ZK_OK;
    for (int i = -2; i < launches && rc == ZK_OK; i++) {           // two untimed launches first (clocks, code upload)
        if (e0.record(st) != hipSuccess) rc = ZK_ERR_HIP;
        hipLaunchKernelGGL(k_diag_mad64, blocks, threads, 0, st, out, 3u, 5u);
        if (e1.record(st) != hipSuccess || hipEventSynchronize(e1.get()) != hipSuccess) rc = ZK_ERR_HIP;
        float ms = 0;
        if (rc == ZK_OK && hipEventElapsedTime(&ms, e0.get(), e1.get()) != hipSuccess) rc = ZK_ERR_HIP;
        if (rc == ZK_OK && i >= 0 && ms > 0) rate.push_back(mads / (ms * 1e-3));
    }
    if (rc != ZK_OK || rate.empty()) ZK_FAIL(ctx, ZK_ERR_HIP, "zk_diag_int_mad_peak: timing failed");
    std::sort(rate.begin(), rate.end());
    if (best_mads_per_s) *best_mads_per_s = rate.back();
    if (median_mads_per_s) *median_mads_per_s = rate[rate.size() / 2];
    return ZK_OK;
    ZK_API_END
}

namespace {
template <int WORDS64>
int diag_pow(zk_ctx* ctx, const uint64_t* base, const uint64_t* exp, int lazy, uint64_t* out) {
    if (!ctx || !base || !exp || !out) return ZK_ERR_ARG;
    uint32_t* buf;
    ZK_TRY(zk_scratch(ctx, "diag_pow", 2 * WORDS64 * 8, (void**)&buf));
    DiagExp e;
    for (int i = 0; i < 12; i++) e.w[i] = i < 2 * WORDS64 ? (uint32_t)(exp[i / 2] >> (32 * (i & 1))) : 0u;
    ZK_HIP(ctx, hipMemcpyAsync(buf, base, WORDS64 * 8, hipMemcpyHostToDevice, ctx->stream));
    if (WORDS64 == 6) hipLaunchKernelGGL(k_diag_fq_pow, 1, 64, 0, ctx->stream, (const uint32_t*)buf, e, 64 * WORDS64, lazy, buf + 2 * WORDS64);
    else hipLaunchKernelGGL(k_diag_fr_pow, 1, 64, 0, ctx->stream, (const uint32_t*)buf, e, 64 * WORDS64, lazy, buf + 2 * WORDS64);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(out, buf + 2 * WORDS64, WORDS64 * 8, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}
}  // namespace

extern "C" int zk_diag_fq_pow_dev(zk_ctx* ctx, const zk_fq* base, const uint64_t exp[6], int lazy, zk_fq* out) {
    ZK_API_BEGIN(ctx)
    return diag_pow<6>(ctx, base ? base->l : nullptr, exp, lazy, out ? out->l : nullptr);
    ZK_API_END
}
extern "C" int zk_diag_fr_pow_dev(zk_ctx* ctx, const zk_fr* base, const uint64_t exp[4], int lazy, zk_fr* out) {
    ZK_API_BEGIN(ctx)
    return diag_pow<4>(ctx, base ? base->l : nullptr, exp, lazy, out ? out->l : nullptr);
    ZK_API_END
}

// ---- the lazy-domain test hooks --------------------------------------------------------------------------------------------------
namespace {

// Fq, op numbering of zk_fq_lazy_raw, each with the template arguments the kernels use (the products with PIN: FqField::mul_l /
// sqr_l, mulsub_l and msm_g2pair.hip::mulp_l); element k of a case at words [13 k, +13)
template <int OP>
__global__ void __launch_bounds__(64) k_diag_fq_lazy(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int nin, int nout) {
    using F = FqField;
    constexpr int L = FqParams::L;
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* w = in + (size_t)c * nin * L;
    uint32_t* o = out + (size_t)c * nout * L;
    auto ld = [&](int k) { Fq a; for (int i = 0; i < L; i++) a.l[i] = w[k * L + i]; return a; };
    auto st = [&](int k, const Fq& a) { for (int i = 0; i < L; i++) o[k * L + i] = a.l[i]; };
    auto st8 = [&](const XYZZ<F>& r) {
        const XYZZ<F> cn = xyzz_canon_lazy<F>(r);
        st(0, r.x); st(1, r.y); st(2, r.zz); st(3, r.zzz); st(4, cn.x); st(5, cn.y); st(6, cn.zz); st(7, cn.zzz);
    };
    if constexpr (OP == 0) st(0, F::mul_l(ld(0), ld(1)));
    if constexpr (OP == 1) st(0, F::sqr_l(ld(0)));
    if constexpr (OP == 2) st(0, fp_mul2_lazy<FqParams, false, true>(ld(0), ld(1), ld(2), ld(3)));
    if constexpr (OP == 11) st(0, fp_mul2_lazy<FqParams, true, true>(ld(0), ld(1), ld(2), ld(3)));
    if constexpr (OP == 3) st(0, F::sub_kp<2>(ld(0), ld(1)));
    if constexpr (OP == 4) st(0, F::sub_kp<4>(ld(0), ld(1)));
    if constexpr (OP == 5) st(0, F::sub_kp<6>(ld(0), ld(1)));
    if constexpr (OP == 6) st(0, F::x3_l(ld(0), ld(1), ld(2)));
    if constexpr (OP == 7) st(0, F::canon(ld(0)));
    if constexpr (OP == 8) st(0, F::kp_minus<1>(ld(0)));
    if constexpr (OP == 9) st(0, fp_neg5_almost<FqParams>(ld(0)));
    if constexpr (OP == 10) st8(xyzz_madd_lazy<F>(XYZZ<F>{ld(0), ld(1), ld(2), ld(3)}, Affine<F>{ld(4), ld(5)}));
    if constexpr (OP == 12) st8(xyzz_add_lazy<F>(XYZZ<F>{ld(0), ld(1), ld(2), ld(3)}, XYZZ<F>{ld(4), ld(5), ld(6), ld(7)}));
}

// Fr, op numbering of zk_fr_lazy_raw; element k of a case at words [9 k, +9)
template <int OP>
__global__ void __launch_bounds__(64) k_diag_fr_lazy(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, int nin, int nout) {
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t* w = in + (size_t)c * nin * 9;
    uint32_t* o = out + (size_t)c * nout * 9;
    auto ld = [&](int k) { return limbs_get(w + k * 9); };
    auto st = [&](int k, const Fr& a) { limbs_put(o + k * 9, a); };
    if constexpr (OP == 0) st(0, frl_reduce(ld(0)));
    if constexpr (OP == 1) st(0, frl_norm(ld(0)));
    if constexpr (OP == 2) st(0, frl_sub<2>(ld(0), ld(1)));
    if constexpr (OP == 3) st(0, frl_sub<3>(ld(0), ld(1)));
    if constexpr (OP == 4) st(0, frl_sub<5>(ld(0), ld(1)));
    if constexpr (OP == 5) st(0, frl_mul(ld(0), ld(1)));
    if constexpr (OP == 6) st(0, frl_canon(ld(0)));
    if constexpr (OP == 7 || OP == 8) {
        Fr x0 = ld(0), x1 = ld(1), x2 = ld(2), x3 = ld(3);
        frl_radix4<OP == 7>(x0, x1, x2, x3, ld(4), ld(5), ld(6));
        st(0, x0); st(1, x1); st(2, x2); st(3, x3);
    }
    if constexpr (OP == 9) { Fr x0 = ld(0), x1 = ld(1); frl_radix2(x0, x1, ld(2)); st(0, x0); st(1, x1); }
    if constexpr (OP == 10) st(0, fr_mul32(ld(0)));
}

#define ZK_DIAG_CASE(KERN, N) case N: hipLaunchKernelGGL(KERN<N>, blocks, 64, 0, st, in, out, nin, nout); break;
void launch_fq_lazy(hipStream_t st, int op, const uint32_t* in, uint32_t* out, unsigned lanes, int nin, int nout) {
    const unsigned blocks = lanes / 64;
    switch (op) {
        ZK_DIAG_CASE(k_diag_fq_lazy, 0) ZK_DIAG_CASE(k_diag_fq_lazy, 1) ZK_DIAG_CASE(k_diag_fq_lazy, 2) ZK_DIAG_CASE(k_diag_fq_lazy, 3)
        ZK_DIAG_CASE(k_diag_fq_lazy, 4) ZK_DIAG_CASE(k_diag_fq_lazy, 5) ZK_DIAG_CASE(k_diag_fq_lazy, 6) ZK_DIAG_CASE(k_diag_fq_lazy, 7)
        ZK_DIAG_CASE(k_diag_fq_lazy, 8) ZK_DIAG_CASE(k_diag_fq_lazy, 9) ZK_DIAG_CASE(k_diag_fq_lazy, 10) ZK_DIAG_CASE(k_diag_fq_lazy, 11)
        ZK_DIAG_CASE(k_diag_fq_lazy, 12)
        default: break;
    }
}
void launch_fr_lazy(hipStream_t st, int op, const uint32_t* in, uint32_t* out, unsigned lanes, int nin, int nout) {
    const unsigned blocks = lanes / 64;
    switch (op) {
        ZK_DIAG_CASE(k_diag_fr_lazy, 0) ZK_DIAG_CASE(k_diag_fr_lazy, 1) ZK_DIAG_CASE(k_diag_fr_lazy, 2) ZK_DIAG_CASE(k_diag_fr_lazy, 3)
        ZK_DIAG_CASE(k_diag_fr_lazy, 4) ZK_DIAG_CASE(k_diag_fr_lazy, 5) ZK_DIAG_CASE(k_diag_fr_lazy, 6) ZK_DIAG_CASE(k_diag_fr_lazy, 7)
        ZK_DIAG_CASE(k_diag_fr_lazy, 8) ZK_DIAG_CASE(k_diag_fr_lazy, 9) ZK_DIAG_CASE(k_diag_fr_lazy, 10)
        default: break;
    }
}
#undef ZK_DIAG_CASE

// elements in / out per case and lanes per case, by op (0 0 = no such op)
struct DiagShape { int nin, nout, lanes; };
constexpr DiagShape FQ_SHAPES[] = {{2, 1, 1}, {1, 1, 1}, {4, 1, 1}, {2, 1, 1}, {2, 1, 1}, {2, 1, 1}, {3, 1, 1},
                                   {1, 1, 1}, {1, 1, 1}, {1, 1, 1}, {6, 8, 1}, {4, 1, 1}, {8, 8, 1}};
constexpr DiagShape FR_SHAPES[] = {{1, 1, 1}, {1, 1, 1}, {2, 1, 1}, {2, 1, 1}, {2, 1, 1}, {2, 1, 1}, {1, 1, 1},
                                   {7, 4, 1}, {7, 4, 1}, {3, 2, 1}, {1, 1, 1}};
// ops 0 - 6: Fq2 elements (two components of 13 words) on lane pairs / quads; 7, 8: G1 (Fq elements) on lane pairs
constexpr DiagShape PAIR_SHAPES[] = {{2, 1, 2}, {2, 1, 2}, {2, 1, 2}, {6, 8, 2}, {2, 4, 2}, {8, 8, 4}, {6, 8, 4}, {8, 8, 2}, {6, 8, 2}};
constexpr DiagShape F7_SHAPES[] = {{1, 1, 1}, {2, 1, 1}, {2, 1, 1}, {2, 1, 1}, {2, 1, 1}, {1, 1, 1}, {2, 2, 1}, {3, 2, 1}, {1, 1, 1}};
constexpr size_t DIAG_MAX_CASES = (size_t)1 << 20;

// pads the case array to whole waves (all-zero cases), runs one launch, copies the n_cases results back
template <class Launch>
int diag_batch(zk_ctx* ctx, const DiagShape& sh, int words, const uint32_t* in, uint32_t* out, size_t n_cases, Launch launch) {
    const size_t lanes = (n_cases * sh.lanes + 63) / 64 * 64, padded = lanes / sh.lanes;
    const size_t in_w = (size_t)sh.nin * words, out_w = (size_t)sh.nout * words;
    uint32_t *din, *dout;
    ZK_TRY(zk_scratch(ctx, "diag_lazy_in", padded * in_w * 4, (void**)&din));
    ZK_TRY(zk_scratch(ctx, "diag_lazy_out", padded * out_w * 4, (void**)&dout));
    ZK_HIP(ctx, hipMemsetAsync(din, 0, padded * in_w * 4, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(din, in, n_cases * in_w * 4, hipMemcpyHostToDevice, ctx->stream));
    launch(ctx->stream, din, dout, (unsigned)lanes);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(out, dout, n_cases * out_w * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

}  // namespace

extern "C" int zk_diag_fq_lazy_dev(zk_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n_cases) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in || !out || op < 0 || op > 12 || n_cases < 1 || n_cases > DIAG_MAX_CASES) return ZK_ERR_ARG;
    const DiagShape sh = FQ_SHAPES[op];
    return diag_batch(ctx, sh, FqParams::L, in, out, n_cases, [&](hipStream_t st, const uint32_t* i, uint32_t* o, unsigned lanes) {
        launch_fq_lazy(st, op, i, o, lanes, sh.nin, sh.nout);
    });
    ZK_API_END
}
extern "C" int zk_diag_fr_lazy_dev(zk_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n_cases) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in || !out || op < 0 || op > 10 || n_cases < 1 || n_cases > DIAG_MAX_CASES) return ZK_ERR_ARG;
    const DiagShape sh = FR_SHAPES[op];
    return diag_batch(ctx, sh, 9, in, out, n_cases, [&](hipStream_t st, const uint32_t* i, uint32_t* o, unsigned lanes) {
        launch_fr_lazy(st, op, i, o, lanes, sh.nin, sh.nout);
    });
    ZK_API_END
}
extern "C" int zk_diag_fq2_pair_dev(zk_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n_cases) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in || !out || op < 0 || op > 8 || n_cases < 1 || n_cases > DIAG_MAX_CASES) return ZK_ERR_ARG;
    const DiagShape sh = PAIR_SHAPES[op];
    return diag_batch(ctx, sh, op <= 6 ? 2 * FqParams::L : FqParams::L, in, out, n_cases,
                      [&](hipStream_t st, const uint32_t* i, uint32_t* o, unsigned lanes) {
                          if (op <= 6) zk_diag_launch_fq2_pair(st, op, i, o, lanes);
                          else zk_diag_launch_g1_dual(st, op, i, o, lanes);
                      });
    ZK_API_END
}
// The MSM jobs committed to the context's ring since the last call (msm.hip: msm_plan_commit), oldest first; no device work.
extern "C" int zk_diag_msm_plans(zk_ctx* ctx, zk_msm_plan* out, size_t cap, size_t* n_out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || (cap && !out)) return ZK_ERR_ARG;
    zk_ctx::PlanRing& r = ctx->plans;
    if (r.written - r.read > ZK_MSM_PLAN_RING) r.read = r.written - ZK_MSM_PLAN_RING;      // the oldest were overwritten
    size_t k = 0;
    for (; r.read < r.written && k < cap; r.read++) out[k++] = r.rec[r.read % ZK_MSM_PLAN_RING];
    r.read = r.written;
    if (n_out) *n_out = k;
    return ZK_OK;
    ZK_API_END
}
extern "C" int zk_diag_f7l_dev(zk_ctx* ctx, int op, const uint32_t* in, uint32_t* out, size_t n_cases) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in || !out || op < 0 || op > 8 || n_cases < 1 || n_cases > DIAG_MAX_CASES) return ZK_ERR_ARG;
    return diag_batch(ctx, F7_SHAPES[op], 26, in, out, n_cases, [&](hipStream_t st, const uint32_t* i, uint32_t* o, unsigned lanes) {
        zk_diag_launch_f7l(st, op, i, o, lanes);
    });
    ZK_API_END
}
