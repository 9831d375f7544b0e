// pairing.hip -- the BLS12-377 pairing on the device: Miller loops, products of Miller values, the final exponentiation.
//
// Replaces (reference):
//   PairingEngine::product_of_pairings / miller_loop / final_exponentiation      arkworks/algebra/ec/src/lib.rs:80-130, models/bls12/mod.rs
// The arithmetic is pairing.cuh, instantiated over Fq2Field here for the kernels and over Fq264Field for the host forms.  The
// verifiers that run on these kernels are groth16_verify.hip and marlin_verify.hip (internal.hpp and pairing.cuh declare what they call).
//
//   k_miller          one pairing per lane: (G1 affine, G2 affine) -> the Miller value, an Fq12 of 144 packed words
//   k_pairing_finish  one product per lane: the product of its `pairs` Miller values, the final exponentiation, then the GT value
//                     in the ABI's form and / or the verdict against a given GT value
//   k_fq12_fold       n packed Miller values -> ceil(n / FOLD_SPAN) partial products.  One wave per block; a lane multiplies its
//                     FOLD_PER_LANE values serially (value b SPAN + 64 j + lane in round j: the wave reads 64 neighbours), then six
//                     tree steps through LDS, words interleaved across the lanes (word i of lane l at 64 i + l: a wave's access to
//                     one word is 64 distinct banks); lane 0 writes.  Lanes past n hold the Fq12 one.  The product is exact and
//                     commutative: which lane multiplies which values does not show in the words that come out.
//   k_diag_fq12       the tower operations, one case per lane (tests)
// Lanes of a wave never part on data inside the pairing: the bits of x are compile-time constants, infinity is a select at the end.
// Registers: an Fq12 is 156 limb words, and a product of two needs three of them live: the tower functions are calls and their
// temporaries live in scratch (DESIGN 5 has the figures from the compiler's metadata).
// A product of MANY Miller values (zk_miller_product) re-launches the fold on its partials until at most 64 are left and finishes
// those on the host: the product and final_exponentiation<Fq264Field> (0.6 ms; k_pairing_finish over the same partials, one lane,
// was measured at 18 ms).
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "pairing.cuh"
#include <string.h>

using namespace zk;

namespace {

using D2 = Fq2Field;
using H2 = Fq264Field;
constexpr int FOLD_PER_LANE = 4;
constexpr size_t FOLD_SPAN = 64 * (size_t)FOLD_PER_LANE;
constexpr size_t PAIRING_MAX_LANES = ZK_PAIRING_MAX_LANES;

// an Fq12 at FQ12_WORDS words by 16-byte accesses.  ext: the ABI's form (a test hook's input and output); else packed internal
// words as k_miller writes them
__device__ __forceinline__ Fq12<D2> fq12_load16(const uint32_t* w, bool ext) {
    Fq12<D2> f;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) f.c[i].c[j] = felt_load16<D2>(w + 24 * (3 * i + j));
    if (ext)      // (behind the loads: with a constant `false` the kernels compile as they did with a loader that had no switch)
        for (int i = 0; i < 2; i++)
            for (int j = 0; j < 3; j++) f.c[i].c[j] = D2::ext_to_int(f.c[i].c[j]);
    return f;
}
__device__ __forceinline__ void fq12_store16(uint32_t* w, const Fq12<D2>& f, bool ext) {
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) felt_store16<D2>(w + 24 * (3 * i + j), ext ? D2::int_to_ext(f.c[i].c[j]) : f.c[i].c[j]);
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
    fq12_store16(out + i * FQ12_WORDS, f, false);
}

// gt (or NULL): count GT values in the ABI's form.  ok (or NULL): ok[k] = the product equals `want` (packed, internal form) and
// bad[k] (or NULL) is clear.  want_slot (or NULL): product k is held to value want_slot[k] of `want` (several keys: each proof
// against its key's e(alpha, beta)); without, every product to value 0.
__global__ void __launch_bounds__(64) k_pairing_finish(const uint32_t* __restrict__ ml, size_t pairs, size_t count, uint32_t* __restrict__ gt,
                                                       const uint32_t* __restrict__ want, const uint32_t* __restrict__ bad, int* __restrict__ ok,
                                                       const uint32_t* __restrict__ want_slot) {
    const size_t k = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (k >= count) return;
    Fq12<D2> acc = fq12_load16(ml + k * pairs * FQ12_WORDS, false);
    for (size_t j = 1; j < pairs; j++) {
        const Fq12<D2> f = fq12_load16(ml + (k * pairs + j) * FQ12_WORDS, false);
        fq12_mul<D2>(acc, acc, f);
    }
    Fq12<D2> r;
    final_exponentiation<D2>(r, acc);
    if (gt) fq12_to_ext<D2>(gt + k * FQ12_WORDS, r);
    if (ok) {
        const Fq12<D2> w = fq12_load16(want + (want_slot ? (size_t)want_slot[k] * FQ12_WORDS : 0), false);
        ok[k] = (fq12_eq<D2>(r, w) && !(bad && bad[k])) ? 1 : 0;
    }
}

// ---- k_fq12_fold ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void fold_lds_put(uint32_t* lds, uint32_t lane, const Fq12<D2>& f) {
    for (int c = 0; c < 6; c++) {
        uint32_t w[24];
        D2::store(w, f.c[c / 3].c[c % 3]);
#pragma unroll
        for (int i = 0; i < 24; i++) lds[(24 * c + i) * 64 + lane] = w[i];
    }
}
__device__ __forceinline__ Fq12<D2> fold_lds_get(const uint32_t* lds, uint32_t lane) {
    Fq12<D2> f;
    for (int c = 0; c < 6; c++) {
        uint32_t w[24];
#pragma unroll
        for (int i = 0; i < 24; i++) w[i] = lds[(24 * c + i) * 64 + lane];
        f.c[c / 3].c[c % 3] = D2::load(w);
    }
    return f;
}

// block b: out[b] = the product of in[b SPAN .. min(n, (b + 1) SPAN)); the grid is ceil(n / SPAN) blocks of one wave
__global__ void __launch_bounds__(64) k_fq12_fold(const uint32_t* __restrict__ in, size_t n, uint32_t* __restrict__ out, int in_ext, int out_ext) {
    __shared__ uint32_t lds[FQ12_WORDS * 64];
    const uint32_t lane = threadIdx.x;
    const size_t base = blockIdx.x * FOLD_SPAN;
    const size_t have = n - base < FOLD_SPAN ? n - base : FOLD_SPAN;      // this block's values: the same on every lane
    const int rounds = (int)((have + 63) / 64);
    Fq12<D2> acc = fq12_one<D2>();
#pragma unroll 1
    for (int j = 0; j < rounds; j++) {
        const size_t i = base + (size_t)j * 64 + lane;
        Fq12<D2> f = fq12_one<D2>();
        if (i < n) f = fq12_load16(in + i * FQ12_WORDS, in_ext != 0);
        if (j == 0) acc = f; else fq12_mul<D2>(acc, acc, f);
    }
    // after step s the lanes at 0 mod 2 s hold the product of their 2 s lanes; lanes from `have` on hold one: steps beyond are skipped
#pragma unroll 1
    for (uint32_t s = 1; s < 64 && s < have; s <<= 1) {
        const uint32_t pos = lane & (2 * s - 1);
        if (pos == s) fold_lds_put(lds, lane, acc);
        __syncthreads();
        if (pos == 0) {
            const Fq12<D2> f = fold_lds_get(lds, lane + s);
            fq12_mul<D2>(acc, acc, f);
        }
        __syncthreads();
    }
    if (lane == 0) fq12_store16(out + (size_t)blockIdx.x * FQ12_WORDS, acc, out_ext != 0);
}

// ---- the tower operations as a test hook: op 0 a b, 1 a^2, 2 a times the line (b.c[0].c[0], b.c[1].c[0], b.c[1].c[1]), 3 1 / a,
// 4 - 6 a^(q^1..3), 7 the cyclotomic squaring of a.  A case is (a, b) in the ABI's form; one result per case. ----------------------------
template <class F2>
__host__ __device__ void diag_fq12_op(int op, const uint32_t* in, uint32_t* out) {
    const Fq12<F2> a = fq12_from_ext<F2>(in), b = fq12_from_ext<F2>(in + FQ12_WORDS);
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
    diag_fq12_op<D2>(op, in + i * 2 * FQ12_WORDS, out + i * FQ12_WORDS);
}

inline size_t fold_count(size_t n) { return (n + FOLD_SPAN - 1) / FOLD_SPAN; }      // the partial products one fold launch leaves of n values
// the m packed Miller values in `in` folded down to at most `limit` through the buffers a, b (fold_scratch); *res says where they are
int fq12_fold_down(zk_ctx* ctx, const uint32_t* in, uint32_t* a, uint32_t* b, size_t* m, size_t limit, const uint32_t** res) {
    while (*m > limit) {
        hipLaunchKernelGGL(k_fq12_fold, (unsigned)fold_count(*m), 64, 0, ctx->stream, in, *m, a, 0, 0);
        ZK_HIP(ctx, hipGetLastError());
        *m = fold_count(*m);
        in = a;
        std::swap(a, b);
    }
    *res = in;
    return ZK_OK;
}
// FE(prod of the m packed values), on the host
Fq12<H2> host_finish(const uint32_t* packed, size_t m) {
    Fq12<H2> acc = fq12_one<H2>(), r;
    for (size_t i = 0; i < m; i++) fq12_mul<H2>(acc, acc, fq12_host_from_packed(packed + i * FQ12_WORDS));
    final_exponentiation<H2>(r, acc);
    return r;
}

}  // namespace

// ---- for every caller whose pairs are on the device already: this file's entry points, groth16_verify.hip, marlin_verify.hip
// (internal.hpp and pairing.cuh say what each takes); on ctx->stream ----------------------------------------------------------------
int zk_pair_scratch(zk_ctx* ctx, size_t n, uint32_t** p_dev, uint32_t** q_dev, uint32_t** ml_dev) {
    if (p_dev) ZK_TRY(zk_scratch(ctx, "pair_p", n * 96, (void**)p_dev));
    if (q_dev) ZK_TRY(zk_scratch(ctx, "pair_q", n * 192, (void**)q_dev));
    if (ml_dev) ZK_TRY(zk_scratch(ctx, "pair_ml", n * FQ12_WORDS * 4, (void**)ml_dev));
    return ZK_OK;
}
// the two buffers a fold of n values goes through: room for fold_count(n) values and for the level after it
int zk_fold_scratch(zk_ctx* ctx, size_t n, uint32_t** a_dev, uint32_t** b_dev) {
    void *a, *b;
    ZK_TRY(zk_scratch(ctx, "agg_fold_a", fold_count(n) * FQ12_WORDS * 4, &a));
    ZK_TRY(zk_scratch(ctx, "agg_fold_b", (fold_count(n) / FOLD_SPAN + 1) * FQ12_WORDS * 4, &b));
    if (a_dev) *a_dev = (uint32_t*)a;
    if (b_dev) *b_dev = (uint32_t*)b;
    return ZK_OK;
}
int zk_miller_launch(zk_ctx* ctx, const uint32_t* p_dev, const uint32_t* q_dev, size_t n, uint32_t* ml_dev, bool ext) {
    if (ext) hipLaunchKernelGGL(k_miller<true>, zk_blocks64(n), 64, 0, ctx->stream, p_dev, q_dev, n, ml_dev);
    else hipLaunchKernelGGL(k_miller<false>, zk_blocks64(n), 64, 0, ctx->stream, p_dev, q_dev, n, ml_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int zk_pairing_finish_launch(zk_ctx* ctx, const uint32_t* ml_dev, size_t pairs, size_t count, uint32_t* gt_dev, const uint32_t* want_dev,
                             const uint32_t* bad_dev, int* ok_dev, const uint32_t* want_slot_dev) {
    hipLaunchKernelGGL(k_pairing_finish, zk_blocks64(count), 64, 0, ctx->stream, ml_dev, pairs, count, gt_dev, want_dev, bad_dev, ok_dev, want_slot_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
int zk_miller_product(zk_ctx* ctx, const uint32_t* ml_dev, size_t n, Fq12<H2>* out, ZkPhaseTimer* tm, ZkHostLap* lap) {
    uint32_t *fold_a, *fold_b;
    ZK_TRY(zk_fold_scratch(ctx, n, &fold_a, &fold_b));      // (no growth, no wait, where the caller has reserved them)
    size_t m = n;
    const uint32_t* res;
    const bool timed = tm && lap && tm->enabled;
    if (timed) tm->begin((std::string(lap->prefix) + "k_fold").c_str());
    ZK_TRY(fq12_fold_down(ctx, ml_dev, fold_a, fold_b, &m, 64, &res));
    if (timed) tm->end();
    std::vector<uint32_t> h_ml(m * FQ12_WORDS);
    ZK_HIP(ctx, hipMemcpyAsync(h_ml.data(), res, h_ml.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (lap) lap->lap("wait_miller");
    *out = host_finish(h_ml.data(), m);
    if (lap) lap->lap("host_finish");
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
        zk_host_gt_out(&outs[k], r);
    }
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_pairing_products(zk_ctx* ctx, const zk_g1_affine* p, const zk_g2_affine* q, size_t pairs, size_t count, zk_gt* outs) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !p || !q || !outs || !pairs || !count || pairs > PAIRING_MAX_LANES / count) return ZK_ERR_ARG;
    const size_t n = pairs * count;
    uint32_t *dp, *dq, *ml, *gt;
    ZK_TRY(zk_pair_scratch(ctx, n, &dp, &dq, &ml));
    ZK_TRY(zk_scratch(ctx, "pair_gt", count * FQ12_WORDS * 4, (void**)&gt));
    ZK_HIP(ctx, hipMemcpyAsync(dp, p, n * 96, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(dq, q, n * 192, hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(zk_miller_launch(ctx, dp, dq, n, ml, true));
    ZK_TRY(zk_pairing_finish_launch(ctx, ml, pairs, count, gt, nullptr, nullptr, nullptr));
    ZK_HIP(ctx, hipMemcpyAsync(outs, gt, count * FQ12_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
    ZK_API_END
}

// one product of n pairs, n as large as a launch allows: the Miller loops, then zk_miller_product
extern "C" int zk_pairing_product_long(zk_ctx* ctx, const zk_g1_affine* p, const zk_g2_affine* q, size_t n, zk_gt* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !p || !q || !out || !n || n > PAIRING_MAX_LANES) return ZK_ERR_ARG;
    uint32_t *dp, *dq, *ml;
    ZK_TRY(zk_pair_scratch(ctx, n, &dp, &dq, &ml));
    ZK_TRY(zk_fold_scratch(ctx, n, nullptr, nullptr));
    ZK_HIP(ctx, hipMemcpyAsync(dp, p, n * 96, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(dq, q, n * 192, hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(zk_miller_launch(ctx, dp, dq, n, ml, true));
    Fq12<H2> r;
    ZK_TRY(zk_miller_product(ctx, ml, n, &r));
    zk_host_gt_out(out, r);
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_gt_is_one(const zk_gt* a) {
    ZK_API_BEGIN_NOCTX
    if (!a) return 0;
    zk_gt one;
    zk_host_gt_out(&one, fq12_one<H2>());
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
    fq12_mul<H2>(r, zk_host_gt(a), zk_host_gt(b));
    zk_host_gt_out(out, r);
    return ZK_OK;
    ZK_API_END
}

extern "C" size_t zk_diag_fq12_fold_span(void) { return FOLD_SPAN; }

extern "C" int zk_diag_fq12_fold_dev(zk_ctx* ctx, const zk_gt* in, size_t n, zk_gt* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in || !out || !n || n > PAIRING_MAX_LANES) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&in[i], 12)) return ZK_ERR_ARG;
    uint32_t *d_in, *a, *b;
    ZK_TRY(zk_pair_scratch(ctx, n, nullptr, nullptr, &d_in));
    ZK_TRY(zk_fold_scratch(ctx, n, &a, &b));
    ZK_HIP(ctx, hipMemcpyAsync(d_in, in, n * FQ12_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
    // the kernel alone, down to ONE value (n = 1: one launch all the same); the first launch reads, the last writes the ABI's form
    const uint32_t* src = d_in;
    size_t m = n;
    bool first = true;
    do {
        const size_t m_out = fold_count(m);
        hipLaunchKernelGGL(k_fq12_fold, (unsigned)m_out, 64, 0, ctx->stream, src, m, a, first ? 1 : 0, m_out == 1 ? 1 : 0);
        ZK_HIP(ctx, hipGetLastError());
        m = m_out;
        src = a;
        std::swap(a, b);
        first = false;
    } while (m > 1);
    ZK_HIP(ctx, hipMemcpyAsync(out, src, FQ12_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_diag_fq12_host(int op, const zk_gt* in_pairs, zk_gt* out, size_t n_cases) {
    ZK_API_BEGIN_NOCTX
    if (!in_pairs || !out || op < 0 || op > 7 || n_cases < 1 || n_cases > ((size_t)1 << 20)) return ZK_ERR_ARG;
    if (!zk_words_below_q((const uint64_t*)in_pairs, (int)(24 * n_cases))) return ZK_ERR_ARG;
    for (size_t i = 0; i < n_cases; i++) {
        uint32_t in[2 * FQ12_WORDS], o[FQ12_WORDS];
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
    ZK_TRY(zk_scratch(ctx, "diag_fq12_in", n_cases * 2 * FQ12_WORDS * 4, (void**)&din));
    ZK_TRY(zk_scratch(ctx, "diag_fq12_out", n_cases * FQ12_WORDS * 4, (void**)&dout));
    ZK_HIP(ctx, hipMemcpyAsync(din, in_pairs, n_cases * 2 * FQ12_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_diag_fq12, zk_blocks64(n_cases), 64, 0, ctx->stream, op, (const uint32_t*)din, dout, n_cases);
    ZK_HIP(ctx, hipGetLastError());
    ZK_HIP(ctx, hipMemcpyAsync(out, dout, n_cases * FQ12_WORDS * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
    ZK_API_END
}
