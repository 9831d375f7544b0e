// marlin_batch.hip -- the Marlin rounds' polynomial arithmetic for count proofs of ONE index whose challenges differ
// (marlin_prove_batch.hip sequences them).
//
// Every kernel here computes, element for element, what its single form computes for one proof -- marlin.hip (k_gather, k_denoms_k,
// k_f_vals, k_ab_on_b), vec_ops.hip (k_vec_op, k_vec_scale, k_lincomb, k_outer_q1) and the copies, fills and the `blind` step that
// the single prover issues as memcpy / memset calls -- over count vectors of one length: proof y = blockIdx.y, its vector at
// base + y * stride elements.  The constants that differ per proof (alpha, beta, eta, v_H(alpha) v_H(beta), the opening's
// coefficients) come from a small device table, `tab` + y * tab_stride entries of nine limbs (FrK), written once per step; the
// internal / external forms and the EXT_TO_INT repairs are those of the single forms.  The division kernels' batched forms are in
// poly.hip beside the recurrences they share, the sparse product's in r1cs.hip.
// All element-wise and HBM-bound.  The index vectors of round 3 are the same for every proof: count proofs re-read them through the
// cache (the 2-D form; DESIGN 5b'-m says what a loop over the proofs inside the thread would save and that it was not measured).
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "frlazy.cuh"
#include "hostfr.hpp"
#include "internal.hpp"
#include <algorithm>

using namespace zk;

namespace {

#define ZK_B_LOOP(i, n) for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < (n); i += (size_t)gridDim.x * blockDim.x)
__device__ __forceinline__ const char* vec_of(const void* base, size_t stride) { return (const char*)base + blockIdx.y * stride * 32; }
__device__ __forceinline__ char* vec_of(void* base, size_t stride) { return (char*)base + blockIdx.y * stride * 32; }
__device__ __forceinline__ Fr tab_of(const FrK* tab, size_t tab_stride, int k) { return frk(tab[blockIdx.y * tab_stride + k]); }
// The forms over shares (LANES = true): a launch covers lanes * proofs vectors, lane after lane (marlin_prove_batch.hip lays the lanes of a
// witness-dependent region next to each other at one stride), and vector y reads the constants' row and the public operands of proof
// y mod proofs.  LANES = false is the plain batch's kernel: y is the proof.
template <bool LANES> __device__ __forceinline__ unsigned proof_of(unsigned proofs) { return LANES ? blockIdx.y % proofs : blockIdx.y; }
__device__ __forceinline__ const char* vec_at(const void* base, size_t stride, unsigned y) { return (const char*)base + y * stride * 32; }
__device__ __forceinline__ Fr tab_at(const FrK* tab, size_t tab_stride, unsigned y, int k) { return frk(tab[y * tab_stride + k]); }

__global__ void __launch_bounds__(256) k_b_copy(void* dst, size_t ds, const void* src, size_t ss, size_t n) {
    const uint4* s = reinterpret_cast<const uint4*>(vec_of(src, ss));
    uint4* d = reinterpret_cast<uint4*>(vec_of(dst, ds));
    ZK_B_LOOP(i, 2 * n) d[i] = s[i];
}
__global__ void __launch_bounds__(256) k_b_zero(void* dst, size_t ds, size_t n) {
    uint4* d = reinterpret_cast<uint4*>(vec_of(dst, ds));
    ZK_B_LOOP(i, 2 * n) d[i] = make_uint4(0, 0, 0, 0);
}
template <int OP>
__global__ void __launch_bounds__(256) k_b_op(const void* a, size_t sa, const void* b, size_t sb, void* out, size_t so, size_t n) {
    const char *av = vec_of(a, sa), *bv = vec_of(b, sb);
    char* ov = vec_of(out, so);
    ZK_B_LOOP(i, n) {
        Fr x = fr_load(av, i), y = fr_load(bv, i), z;
        if (OP == ZK_OP_MUL) z = fr_mul32(fr_mul(x, y));
        else if (OP == ZK_OP_ADD) z = fr_add(x, y);
        else z = fr_sub(x, y);
        fr_store(ov, i, z);
    }
}
// out_y = a_y * tab_y[0] (the constant in internal form)
template <bool LANES>
__global__ void __launch_bounds__(256) k_b_scale(const void* a, size_t sa, const FrK* tab, size_t ts, void* out, size_t so, size_t n, unsigned proofs) {
    const Fr kk = tab_at(tab, ts, proof_of<LANES>(proofs), 0);
    const char* av = vec_of(a, sa);
    char* ov = vec_of(out, so);
    ZK_B_LOOP(i, n) fr_store(ov, i, fr_mul(fr_load(av, i), kk));
}
// out_y[i] = idx[i] == 0xFFFFFFFF ? 0 : src_y[idx[i]]
__global__ void __launch_bounds__(256) k_b_gather(const void* src, size_t ss, const uint32_t* idx, size_t n, void* out, size_t so) {
    const char* sv = vec_of(src, ss);
    char* ov = vec_of(out, so);
    ZK_B_LOOP(i, n) {
        const uint32_t j = idx[i];
        fr_store(ov, i, j == 0xFFFFFFFFu ? fp_zero<FrParams>() : fr_load(sv, j));
    }
}
// p + r (X^n - 1) for deg p < n: out_y = p_y[0] - r_y | p_y[1 .. n) | r_y
__global__ void __launch_bounds__(256) k_b_blind(const void* p, size_t sp, size_t n, const void* r, size_t sr, void* out, size_t so) {
    const char *pv = vec_of(p, sp), *rv = vec_of(r, sr);
    char* ov = vec_of(out, so);
    ZK_B_LOOP(i, n + 1) {
        Fr x = i < n ? fr_load(pv, i) : fr_load(rv, 0);
        if (i == 0) x = fr_sub(x, fr_load(rv, 0));
        fr_store(ov, i, x);
    }
}
// out_y[i] = tab_y[0] - e[i] (the constant as the bits of its external form; e: one vector for every proof)
__global__ void __launch_bounds__(256) k_b_const_minus(const FrK* tab, size_t ts, const void* e, size_t n, void* out, size_t so) {
    const Fr c = tab_of(tab, ts, 0);
    char* ov = vec_of(out, so);
    ZK_B_LOOP(i, n) fr_store(ov, i, fr_sub(c, fr_load(e, i)));
}
// k_outer_q1 with tab_y = eta_a, eta_b, eta_c; the six vectors of a proof stride elements apart each.  LANES: r(alpha, X) and t are
// public, one vector per proof
template <bool LANES>
__global__ void __launch_bounds__(256) k_b_outer_q1(const void* s, const void* a, const void* b, const void* z, const void* rp, const void* tp,
                                                    size_t stride, const FrK* tab, size_t ts, void* out, size_t n, unsigned proofs) {
    const unsigned pr = proof_of<LANES>(proofs);
    const Fr fa = tab_at(tab, ts, pr, 0), fb = tab_at(tab, ts, pr, 1), fc = tab_at(tab, ts, pr, 2);
    const char *sv = vec_of(s, stride), *av = vec_of(a, stride), *bv = vec_of(b, stride), *zv = vec_of(z, stride), *rv = vec_at(rp, stride, pr),
               *tv = vec_at(tp, stride, pr);
    char* ov = vec_of(out, stride);
    ZK_B_LOOP(i, n) {
        Fr t = fr_add(fr_add(fr_mul(fr_load(sv, i), fc), fr_mul(fr_load(av, i), fa)), fr_mul(fr_load(bv, i), fb));
        t = fr_mul32(fr_mul(fr_load(rv, i), t));
        const Fr u = fr_mul32(fr_mul(fr_load(zv, i), fr_load(tv, i)));
        fr_store(ov, i, fr_sub(t, u));
    }
}
// k_lincomb with tab_y[t] = the coefficient of term t; a term with stride 0 is one vector for every proof (an index oracle).  LANES: a
// term whose bit is set in per_proof is public, one vector per proof (the leader's public oracles in a shared combination)
constexpr int B_LINCOMB_MAX = 16;
struct BLinComb { const void* p[B_LINCOMB_MAX]; size_t stride[B_LINCOMB_MAX]; size_t n[B_LINCOMB_MAX]; int terms; unsigned per_proof; };
template <bool LANES>
__global__ void __launch_bounds__(256) k_b_lincomb(BLinComb c, const FrK* tab, size_t ts, void* out, size_t so, size_t n_out, unsigned proofs) {
    const unsigned pr = proof_of<LANES>(proofs);
    char* ov = vec_of(out, so);
    ZK_B_LOOP(i, n_out) {
        Fr acc = fp_zero<FrParams>();
        for (int t = 0; t < c.terms; t++)
            if (i < c.n[t])
                acc = fr_add(acc, fr_mul(fr_load(vec_at(c.p[t], c.stride[t], LANES && (c.per_proof >> t & 1) ? pr : blockIdx.y), i), tab_at(tab, ts, pr, t)));
        fr_store(ov, i, acc);
    }
}

// ---- round 3: tab_y = alpha_ext, beta_ext, kf[3] | alpha_int, beta_int, ba_ext, kab[3]  (ZK_B_R3_ROW entries; the constants as
// zk_marlin_round3_f_evals_dev / _ab_evals_dev prepare them) ----
struct Mats { const void* row[3]; const void* col[3]; const void* val[3]; const void* row_col[3]; };
// den_y[m][i] = (beta - row_m[i]) * (alpha - col_m[i])
__global__ void __launch_bounds__(256) k_b_denoms_k(Mats M, const FrK* tab, size_t ts, size_t n, void* den) {
    const Fr fix = fp_const<FrParams>(FrParams::EXT_TO_INT), a = tab_of(tab, ts, 0), b = tab_of(tab, ts, 1);
    char* dv = vec_of(den, 3 * n);
    ZK_B_LOOP(i, n) {
#pragma unroll
        for (int m = 0; m < 3; m++) {
            Fr x = fr_sub(b, fr_load(M.row[m], i)), y = fr_sub(a, fr_load(M.col[m], i));
            fr_store(dv, (size_t)m * n + i, fr_mul(fr_mul(x, y), fix));
        }
    }
}
// f_y[i] = sum_m k_m * val_m[i] * inv_y[m][i]
__global__ void __launch_bounds__(256) k_b_f_vals(Mats M, const void* inv, const FrK* tab, size_t ts, size_t n, void* f, size_t sf) {
    const Fr k[3] = {tab_of(tab, ts, 2), tab_of(tab, ts, 3), tab_of(tab, ts, 4)};
    const char* iv = vec_of(inv, 3 * n);
    char* fv = vec_of(f, sf);
    ZK_B_LOOP(i, n) {
        Fr acc = fp_zero<FrParams>();
#pragma unroll
        for (int m = 0; m < 3; m++) acc = fr_add(acc, fr_mul(fr_mul(fr_load(M.val[m], i), fr_load(iv, (size_t)m * n + i)), k[m]));
        fr_store(fv, i, acc);
    }
}
// den_m = beta alpha - alpha row_m - beta col_m + row_col_m ;  b = den_a den_b den_c ;  a = sum_m k_m val_m prod_{m' != m} den_m'
__global__ void __launch_bounds__(256) k_b_ab_on_b(Mats M, const FrK* tab, size_t ts, FrK fix2, size_t n, void* a_out, void* b_out, size_t so) {
    const Fr al = tab_of(tab, ts, 5), be = tab_of(tab, ts, 6), ba = tab_of(tab, ts, 7), f2 = frk(fix2);
    const Fr k[3] = {tab_of(tab, ts, 8), tab_of(tab, ts, 9), tab_of(tab, ts, 10)};
    char *av = vec_of(a_out, so), *bv = vec_of(b_out, so);
    ZK_B_LOOP(i, n) {
        Fr d[3];
#pragma unroll
        for (int m = 0; m < 3; m++) {
            Fr t = fr_sub(ba, fr_mul(fr_load(M.row[m], i), al));
            t = fr_sub(t, fr_mul(fr_load(M.col[m], i), be));
            d[m] = fr_add(t, fr_load(M.row_col[m], i));
        }
        Fr bc = fr_mul(d[1], d[2]), ac = fr_mul(d[0], d[2]), ab = fr_mul(d[0], d[1]);   // ext * RE / RI
        Fr a = fr_mul(fr_mul(fr_load(M.val[0], i), bc), k[0]);
        a = fr_add(a, fr_mul(fr_mul(fr_load(M.val[1], i), ac), k[1]));
        a = fr_add(a, fr_mul(fr_mul(fr_load(M.val[2], i), ab), k[2]));
        fr_store(av, i, a);
        fr_store(bv, i, fr_mul(fr_mul(ab, d[2]), f2));
    }
}

int load_mats(zk_ctx* ctx, const zk_marlin_matrix_evals* e, bool need_row_col, Mats* M) {
    for (int m = 0; m < 3; m++) {
        if (!e[m].row || !e[m].col || !e[m].val || (need_row_col && !e[m].row_col)) ZK_FAIL(ctx, ZK_ERR_ARG, "marlin: missing matrix evaluation vector");
        M->row[m] = e[m].row; M->col[m] = e[m].col; M->val[m] = e[m].val; M->row_col[m] = e[m].row_col;
    }
    return ZK_OK;
}

// the grid of a launch over count vectors of n items (blockIdx.y: at most 65 535 proofs, far above what a chunk holds)
bool grid_of(size_t n, size_t count, dim3* g) {
    if (!n || !count || count > 65535) return false;
    *g = dim3(zk_grid(n, 256), (unsigned)count);
    return true;
}
int launched(zk_ctx* ctx) {
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}

}  // namespace

int zk_b_copy(zk_ctx* ctx, void* dst, size_t ds, const void* src, size_t ss, size_t n, size_t count) {
    dim3 g;
    if (!grid_of(2 * n, count, &g)) return n ? (int)ZK_ERR_ARG : (int)ZK_OK;
    hipLaunchKernelGGL(k_b_copy, g, 256, 0, ctx->stream, dst, ds, src, ss, n);
    return launched(ctx);
}
int zk_b_zero(zk_ctx* ctx, void* dst, size_t ds, size_t n, size_t count) {
    dim3 g;
    if (!grid_of(2 * n, count, &g)) return n ? (int)ZK_ERR_ARG : (int)ZK_OK;
    hipLaunchKernelGGL(k_b_zero, g, 256, 0, ctx->stream, dst, ds, n);
    return launched(ctx);
}
int zk_b_op(zk_ctx* ctx, int op, const void* a, size_t sa, const void* b, size_t sb, void* out, size_t so, size_t n, size_t count) {
    dim3 g;
    if (!grid_of(n, count, &g)) return n ? (int)ZK_ERR_ARG : (int)ZK_OK;
    switch (op) {
        case ZK_OP_MUL: hipLaunchKernelGGL(k_b_op<ZK_OP_MUL>, g, 256, 0, ctx->stream, a, sa, b, sb, out, so, n); break;
        case ZK_OP_ADD: hipLaunchKernelGGL(k_b_op<ZK_OP_ADD>, g, 256, 0, ctx->stream, a, sa, b, sb, out, so, n); break;
        case ZK_OP_SUB: hipLaunchKernelGGL(k_b_op<ZK_OP_SUB>, g, 256, 0, ctx->stream, a, sa, b, sb, out, so, n); break;
        default: return ZK_ERR_ARG;
    }
    return launched(ctx);
}
// proofs = 0: count proofs, one vector each; otherwise count = lanes * proofs vectors, lane after lane
int zk_b_scale(zk_ctx* ctx, const void* a, size_t sa, const FrK* tab, size_t ts, void* out, size_t so, size_t n, size_t count, size_t proofs) {
    dim3 g;
    if (!grid_of(n, count, &g)) return n ? (int)ZK_ERR_ARG : (int)ZK_OK;
    if (proofs && count % proofs) return ZK_ERR_ARG;
    if (proofs) hipLaunchKernelGGL(k_b_scale<true>, g, 256, 0, ctx->stream, a, sa, tab, ts, out, so, n, (unsigned)proofs);
    else hipLaunchKernelGGL(k_b_scale<false>, g, 256, 0, ctx->stream, a, sa, tab, ts, out, so, n, 0u);
    return launched(ctx);
}
int zk_b_gather(zk_ctx* ctx, const void* src, size_t ss, const uint32_t* idx, size_t n, void* out, size_t so, size_t count) {
    dim3 g;
    if (!grid_of(n, count, &g)) return n ? (int)ZK_ERR_ARG : (int)ZK_OK;
    hipLaunchKernelGGL(k_b_gather, g, 256, 0, ctx->stream, src, ss, idx, n, out, so);
    return launched(ctx);
}
int zk_b_blind(zk_ctx* ctx, const void* p, size_t sp, size_t n, const void* r, size_t sr, void* out, size_t so, size_t count) {
    dim3 g;
    if (!grid_of(n + 1, count, &g) || so < n + 1) return ZK_ERR_ARG;
    hipLaunchKernelGGL(k_b_blind, g, 256, 0, ctx->stream, p, sp, n, r, sr, out, so);
    return launched(ctx);
}
int zk_b_const_minus(zk_ctx* ctx, const FrK* tab, size_t ts, const void* e, size_t n, void* out, size_t so, size_t count) {
    dim3 g;
    if (!grid_of(n, count, &g)) return ZK_ERR_ARG;
    hipLaunchKernelGGL(k_b_const_minus, g, 256, 0, ctx->stream, tab, ts, e, n, out, so);
    return launched(ctx);
}
int zk_b_outer_q1(zk_ctx* ctx, const void* s, const void* a, const void* b, const void* z, const void* rp, const void* tp, size_t stride,
                  const FrK* tab, size_t ts, void* out, size_t n, size_t count, size_t proofs) {
    dim3 g;
    if (!grid_of(n, count, &g) || stride < n || (proofs && count % proofs)) return ZK_ERR_ARG;
    if (proofs) hipLaunchKernelGGL(k_b_outer_q1<true>, g, 256, 0, ctx->stream, s, a, b, z, rp, tp, stride, tab, ts, out, n, (unsigned)proofs);
    else hipLaunchKernelGGL(k_b_outer_q1<false>, g, 256, 0, ctx->stream, s, a, b, z, rp, tp, stride, tab, ts, out, n, 0u);
    return launched(ctx);
}
int zk_b_lincomb(zk_ctx* ctx, int terms, const void* const* ps, const size_t* strides, const size_t* ns, const FrK* tab, size_t ts, void* out, size_t so,
                 size_t n_out, size_t count, size_t proofs, unsigned per_proof) {
    dim3 g;
    if (terms < 1 || terms > B_LINCOMB_MAX || !grid_of(n_out, count, &g) || so < n_out || (proofs && count % proofs)) return ZK_ERR_ARG;
    BLinComb c{};
    c.terms = terms;
    c.per_proof = per_proof;
    for (int t = 0; t < terms; t++) { c.p[t] = ps[t]; c.stride[t] = strides[t]; c.n[t] = std::min(ns[t], n_out); }
    if (proofs) hipLaunchKernelGGL(k_b_lincomb<true>, g, 256, 0, ctx->stream, c, tab, ts, out, so, n_out, (unsigned)proofs);
    else hipLaunchKernelGGL(k_b_lincomb<false>, g, 256, 0, ctx->stream, c, tab, ts, out, so, n_out, 0u);
    return launched(ctx);
}

void zk_b_round3_row(const Fr& alpha, const Fr& beta, const Fr eta[3], const Fr& vv, FrK* row) {
    const Fr e2i = fp_const<FrParams>(FrParams::EXT_TO_INT), i2e = fp_const<FrParams>(FrParams::INT_TO_EXT);
    const Fr fix2 = fp_mul<FrParams>(e2i, e2i);
    row[0] = to_frk(fp_int_to_ext<FrParams>(alpha));
    row[1] = to_frk(fp_int_to_ext<FrParams>(beta));
    for (int m = 0; m < 3; m++) row[2 + m] = to_frk(fp_mul<FrParams>(fp_mul<FrParams>(eta[m], vv), e2i));
    row[5] = to_frk(alpha);
    row[6] = to_frk(beta);
    row[7] = to_frk(fp_mul<FrParams>(fp_mul<FrParams>(alpha, beta), i2e));
    for (int m = 0; m < 3; m++) row[8 + m] = to_frk(fp_mul<FrParams>(fp_mul<FrParams>(eta[m], vv), fix2));
}
int zk_b_round3_denoms(zk_ctx* ctx, const zk_marlin_matrix_evals on_k[3], size_t k_size, const FrK* tab, void* den, size_t count) {
    Mats M;
    dim3 g;
    ZK_TRY(load_mats(ctx, on_k, false, &M));
    if (!grid_of(k_size, count, &g)) return ZK_ERR_ARG;
    hipLaunchKernelGGL(k_b_denoms_k, g, 256, 0, ctx->stream, M, tab, (size_t)ZK_B_R3_ROW, k_size, den);
    return launched(ctx);
}
int zk_b_round3_f(zk_ctx* ctx, const zk_marlin_matrix_evals on_k[3], size_t k_size, const FrK* tab, const void* inv, void* f, size_t f_stride, size_t count) {
    Mats M;
    dim3 g;
    ZK_TRY(load_mats(ctx, on_k, false, &M));
    if (!grid_of(k_size, count, &g) || f_stride < k_size) return ZK_ERR_ARG;
    hipLaunchKernelGGL(k_b_f_vals, g, 256, 0, ctx->stream, M, inv, tab, (size_t)ZK_B_R3_ROW, k_size, f, f_stride);
    return launched(ctx);
}
int zk_b_round3_ab(zk_ctx* ctx, const zk_marlin_matrix_evals on_b[3], size_t b_size, const FrK* tab, void* a_out, void* b_out, size_t stride, size_t count) {
    Mats M;
    dim3 g;
    ZK_TRY(load_mats(ctx, on_b, true, &M));
    if (!grid_of(b_size, count, &g) || stride < b_size) return ZK_ERR_ARG;
    const Fr e2i = fp_const<FrParams>(FrParams::EXT_TO_INT);
    hipLaunchKernelGGL(k_b_ab_on_b, g, 256, 0, ctx->stream, M, tab, (size_t)ZK_B_R3_ROW, to_frk(fp_mul<FrParams>(e2i, e2i)), b_size, a_out, b_out, stride);
    return launched(ctx);
}
