// vec_ops.hip -- element-wise Fr kernels on device vectors in the reference's layout.
// Replaces: Field::batch_product_in_place (ff/src/fields/mod.rs:216-220), the `ab -= c` loop and
// divide_by_vanishing_poly_on_coset_in_place of witness_map (src/groth16.rs:285-302,
// poly/src/domain/mod.rs:183-190), AdditiveFieldShare::{add,sub,scale} on vectors
// (mpc-algebra/src/share/additive.rs:133-152), batch_open's sum and batch_mul's tail
// (share/additive.rs:124-131, share/field.rs:118-128).
// HBM-bound: 96 B of traffic per element for a binary op (2 x 32 B in, 32 B out).
#include "../../include/zkmpc_hip.h"
#include "hostfr.hpp"
#include "frlazy.cuh"
#include "internal.hpp"
#include <algorithm>

using namespace zk;

namespace {

template <int OP>
__global__ void __launch_bounds__(256) k_vec_op(const void* a, const void* b, void* out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr x = fr_load(a, i), y = fr_load(b, i), z;
        if (OP == ZK_OP_MUL) z = fr_mul32(fr_mul(x, y));     // ext * ext = a b 2^251: times 2^5 (frlazy.cuh), not a second product
        else if (OP == ZK_OP_ADD) z = fr_add(x, y);
        else z = fr_sub(x, y);
        fr_store(out, i, z);
    }
}

__global__ void __launch_bounds__(256) k_vec_scale(const void* a, FrK k, void* out, size_t n) {
    const Fr kk = frk(k);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        fr_store(out, i, fr_mul(fr_load(a, i), kk));
}

// out[i] = sum_t k_t * p_t[i] over the terms with i < n_t (a linear combination of polynomials of different lengths:
// open_combinations, poly-commit/src/lib.rs:~390-460 / marlin_pc/mod.rs:245-340 builds it with one scaled addition per term --
// two launches and five vector passes each; here one launch reads every term once)
constexpr int LINCOMB_MAX = 16;
struct LinComb { const void* p[LINCOMB_MAX]; size_t n[LINCOMB_MAX]; FrK k[LINCOMB_MAX]; int terms; };
__global__ void __launch_bounds__(256) k_lincomb(LinComb c, void* out, size_t n_out, int accumulate) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n_out; i += (size_t)gridDim.x * blockDim.x) {
        Fr acc = accumulate ? fr_load(out, i) : fp_zero<FrParams>();
        for (int t = 0; t < c.terms; t++)
            if (i < c.n[t]) acc = fr_add(acc, fr_mul(fr_load(c.p[t], i), frk(c.k[t])));
        fr_store(out, i, acc);
    }
}

// out = rp * (kc s + ka a + kb b) - z * tp, element-wise (the outer sum-check's q_1 over the multiplication domain,
// arkworks/marlin/src/ahp/prover.rs:517-541: eight launches and seventeen vector passes as separate operations)
__global__ void __launch_bounds__(256) k_outer_q1(const void* s, const void* a, const void* b, const void* z, const void* rp, const void* tp,
                                                  FrK ka, FrK kb, FrK kc, void* out, size_t n) {
    const Fr fa = frk(ka), fb = frk(kb), fc = frk(kc);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr t = fr_add(fr_add(fr_mul(fr_load(s, i), fc), fr_mul(fr_load(a, i), fa)), fr_mul(fr_load(b, i), fb));
        t = fr_mul32(fr_mul(fr_load(rp, i), t));
        const Fr u = fr_mul32(fr_mul(fr_load(z, i), fr_load(tp, i)));
        fr_store(out, i, fr_sub(t, u));
    }
}

// out = (a - b) * k
__global__ void __launch_bounds__(256) k_vec_sub_scale(const void* a, const void* b, FrK k, void* out, size_t n) {
    const Fr kk = frk(k);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        fr_store(out, i, fr_mul(fr_sub(fr_load(a, i), fr_load(b, i)), kk));
}

__global__ void __launch_bounds__(256) k_sum_parties(const void* g, size_t np, size_t n, void* out) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        Fr acc = fr_load(g, i);
        for (size_t p = 1; p < np; p++) acc = fr_add(acc, fr_load(g, p * n + i));
        fr_store(out, i, acc);
    }
}

// out = tz - sx*ty - oy*tx (+ sx*oy if leader).  DUMMY: tx=ty=tz = (leader ? 1 : 0).
template <bool DUMMY>
__global__ void __launch_bounds__(256) k_beaver(const void* sx, const void* oy, const void* tx, const void* ty,
                                                const void* tz, void* out, size_t n, int leader) {
    // 1 in external form = 2^256 mod r = mmul(ONE_internal, INT_TO_EXT)
    const Fr one_ext = fr_mul(fp_one<FrParams>(), fp_const<FrParams>(FrParams::INT_TO_EXT));
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const Fr a = fr_load(sx, i), b = fr_load(oy, i);
        // the 2^5 that a product of two elements in the reference's form lacks goes in ONCE per opened value (fr_mul32), not
        // as a second Montgomery product behind each of the three products
        const Fr a32 = fr_mul32(a);
        Fr z;
        if (DUMMY) {
            if (leader) {
                // 1 - a - b + ab
                z = fr_add(fr_sub(fr_sub(one_ext, a), b), fr_mul(a32, b));
            } else {
                z = fp_zero<FrParams>();
            }
        } else {
            const Fr x = fr_load(tx, i), y = fr_load(ty, i);
            z = fr_load(tz, i);
            z = fr_sub(z, fr_mul(a32, y));
            z = fr_sub(z, fr_mul(fr_mul32(b), x));
            if (leader) z = fr_add(z, fr_mul(a32, b));
        }
        fr_store(out, i, z);
    }
}

// flag |= (any word of v non-zero)
__global__ void __launch_bounds__(256) k_any_nonzero(const void* v, size_t n, uint32_t* flag) {
    const uint4* p = reinterpret_cast<const uint4*>(v);
    uint32_t acc = 0;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < 2 * n; i += (size_t)gridDim.x * blockDim.x) {
        uint4 w = p[i];
        acc |= w.x | w.y | w.z | w.w;
    }
    if (acc) atomicOr(flag, 1u);
}

}  // namespace

int zk_vec_op_launch(zk_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n) {
    if (n == 0) return ZK_OK;
    unsigned g = zk_grid(n, 256);
    switch (op) {
        case ZK_OP_MUL: hipLaunchKernelGGL(k_vec_op<ZK_OP_MUL>, g, 256, 0, ctx->stream, a, b, out, n); break;
        case ZK_OP_ADD: hipLaunchKernelGGL(k_vec_op<ZK_OP_ADD>, g, 256, 0, ctx->stream, a, b, out, n); break;
        case ZK_OP_SUB: hipLaunchKernelGGL(k_vec_op<ZK_OP_SUB>, g, 256, 0, ctx->stream, a, b, out, n); break;
        default: ZK_FAIL(ctx, ZK_ERR_ARG, "zk_fr_vec_op_dev: unknown op");
    }
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int zk_vec_scale_launch(zk_ctx* ctx, const void* a, const Fr& k, void* out, size_t n) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(k_vec_scale, zk_grid(n, 256), 256, 0, ctx->stream, a, to_frk(k), out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int zk_fr_lincomb_launch(zk_ctx* ctx, int terms, const void* const* ps, const size_t* ns, const Fr* k, void* out, size_t n_out) {
    if (n_out == 0) return ZK_OK;
    for (int t0 = 0; t0 < terms || t0 == 0; t0 += LINCOMB_MAX) {
        LinComb c{};
        c.terms = std::min(LINCOMB_MAX, terms - t0);
        for (int t = 0; t < c.terms; t++) {
            c.p[t] = ps[t0 + t];
            c.n[t] = std::min(ns[t0 + t], n_out);
            c.k[t] = to_frk(k[t0 + t]);
        }
        hipLaunchKernelGGL(k_lincomb, zk_grid(n_out, 256), 256, 0, ctx->stream, c, out, n_out, t0 ? 1 : 0);
        ZK_HIP(ctx, hipGetLastError());
    }
    return ZK_OK;
}

int zk_fr_outer_q1_launch(zk_ctx* ctx, const void* s, const void* a, const void* b, const void* z, const void* rp, const void* tp,
                          const Fr& ka, const Fr& kb, const Fr& kc, void* out, size_t n) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(k_outer_q1, zk_grid(n, 256), 256, 0, ctx->stream, s, a, b, z, rp, tp, to_frk(ka), to_frk(kb), to_frk(kc), out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

int zk_vec_sub_scale_launch(zk_ctx* ctx, const void* a, const void* b, const Fr& k, void* out, size_t n) {
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(k_vec_sub_scale, zk_grid(n, 256), 256, 0, ctx->stream, a, b, to_frk(k), out, n);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

extern "C" int zk_fr_vec_op_dev(zk_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n) {
    ZK_API_BEGIN(ctx)
    if (!ctx || (n && (!a || !b || !out))) return ZK_ERR_ARG;
    return zk_vec_op_launch(ctx, op, a, b, out, n);
    ZK_API_END
}

extern "C" int zk_fr_vec_scale_dev(zk_ctx* ctx, const void* a, const zk_fr* k, void* out, size_t n) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !k || (n && (!a || !out))) return ZK_ERR_ARG;
    return zk_vec_scale_launch(ctx, a, HF::from_abi(*k).v, out, n);
    ZK_API_END
}

extern "C" int zk_fr_batch_product_in_place(zk_ctx* ctx, zk_fr* selfs, const zk_fr* others, size_t n) {
    ZK_API_BEGIN(ctx)
    if (!ctx || (n && (!selfs || !others))) return ZK_ERR_ARG;
    if (n == 0) return ZK_OK;
    void *da, *db;
    ZK_TRY(zk_scratch(ctx, "bp_a", n * 32, &da));
    ZK_TRY(zk_scratch(ctx, "bp_b", n * 32, &db));
    ZK_TRY(zk_xfer_h2d(ctx, da, selfs, n * 32));
    ZK_TRY(zk_xfer_h2d(ctx, db, others, n * 32));
    ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_MUL, da, db, da, n));
    ZK_TRY(zk_xfer_d2h(ctx, selfs, da, n * 32));
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_fr_sum_parties_dev(zk_ctx* ctx, const void* g, size_t np, size_t n, void* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || np == 0 || (n && (!g || !out))) return ZK_ERR_ARG;
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(k_sum_parties, zk_grid(n, 256), 256, 0, ctx->stream, g, np, n, out);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_beaver_combine_dev(zk_ctx* ctx, const void* sx, const void* oy, const void* tx, const void* ty,
                                     const void* tz, void* out, size_t n) {
    ZK_API_BEGIN(ctx)
    if (!ctx || (n && (!sx || !oy || !out))) return ZK_ERR_ARG;
    if (n == 0) return ZK_OK;
    int leader = ctx->party_id == 0;
    bool dummy = !tx && !ty && !tz;
    if (!dummy && (!tx || !ty || !tz)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_beaver_combine_dev: give all of tx,ty,tz or none");
    if (dummy)
        hipLaunchKernelGGL(k_beaver<true>, zk_grid(n, 256), 256, 0, ctx->stream, sx, oy, tx, ty, tz, out, n, leader);
    else
        hipLaunchKernelGGL(k_beaver<false>, zk_grid(n, 256), 256, 0, ctx->stream, sx, oy, tx, ty, tz, out, n, leader);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
    ZK_API_END
}

// The same test without the wait: the verdict (0 = every element is zero) lands in a page-locked word once the context stream has
// passed this point; up to 8 tests in flight (slot).  For a prover whose next step does not depend on the verdict (Marlin's
// divisibility checks: the round's commitments are enqueued first, the verdict is read behind them).
int zk_fr_vec_is_zero_launch(zk_ctx* ctx, const void* v, size_t n, int slot, const uint32_t** verdict) {
    if (slot < 0 || slot >= 8) return ZK_ERR_ARG;
    uint32_t* flag;
    ZK_TRY(zk_scratch(ctx, "vec_flag_async", 8 * 16, (void**)&flag));
    uint32_t* h;
    ZK_TRY(zk_pinned(ctx, {ZK_PIN_ZERO_VERDICTS, 0}, 8 * 16, (void**)&h));
    h += 4 * slot;
    ZK_HIP(ctx, hipMemsetAsync(flag + 4 * slot, 0, 4, ctx->stream));
    if (n) hipLaunchKernelGGL(k_any_nonzero, zk_grid(2 * n, 256), 256, 0, ctx->stream, v, n, flag + 4 * slot);
    ZK_HIP(ctx, hipMemcpyAsync(h, flag + 4 * slot, 4, hipMemcpyDeviceToHost, ctx->stream));
    *verdict = h;
    return ZK_OK;
}

extern "C" int zk_fr_vec_is_zero_dev(zk_ctx* ctx, const void* v, size_t n, int* is_zero) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !is_zero || (n && !v)) return ZK_ERR_ARG;
    uint32_t* flag;
    ZK_TRY(zk_scratch(ctx, "vec_flag", 16, (void**)&flag));
    ZK_HIP(ctx, hipMemsetAsync(flag, 0, 4, ctx->stream));
    if (n) hipLaunchKernelGGL(k_any_nonzero, zk_grid(2 * n, 256), 256, 0, ctx->stream, v, n, flag);
    uint32_t h = 0;
    ZK_HIP(ctx, hipMemcpyAsync(&h, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *is_zero = h == 0;
    return ZK_OK;
    ZK_API_END
}
