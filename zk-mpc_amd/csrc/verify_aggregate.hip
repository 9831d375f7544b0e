// verify_aggregate.hip -- count Groth16 proofs of one key as ONE folded pairing product, and the two building blocks it needs: the
// product of MANY Miller values and the sum of many G1 points that belong to no resident table.
//
// Replaces (reference): nothing the reference has for Groth16 (Groth16::verify, arkworks/groth16/src/verifier.rs:13-61, is one
// proof); the fold itself is the one of its KZG verifier (poly-commit/src/kzg10/mod.rs:345, batch_check: a random linear combination
// of the equations, one product of pairings).  With coefficients r_i the batch holds iff
//     prod_i e(r_i A_i, B_i) . e(sum_i r_i C_i, -delta) . e(sum_j s_j gamma_abc[j], -gamma) . e(s_0 alpha, -beta) = 1
//     s_0 = sum_i r_i,  s_j = sum_i r_i x_{i,j} (mod r)
// count + 3 Miller loops and ONE final exponentiation (pairing.hip's batch form: 3 count and count).
//
//   k_fq12_fold       n packed Miller values -> ceil(n / FOLD_SPAN) partial products.  One wave per block; a lane multiplies its
//                     FOLD_PER_LANE values serially (value b SPAN + 64 j + lane in round j: the wave reads 64 neighbours), then six
//                     tree steps through LDS, words interleaved across the lanes (word i of lane l at 64 i + l: a wave's access to
//                     one word is 64 distinct banks); lane 0 writes.  Lanes past n hold the Fq12 one.  The product is exact and
//                     commutative: which lane multiplies which values does not show in the words that come out.
//   k_g1_scale_fold   per lane an affine point and a 128-bit coefficient -> r P in XYZZ by g1_lincomb.cuh's fixed signed windows
//                     (32 windows; the digit selects a table entry in LDS and a sign, never the control flow), then either per
//                     lane the affine point (the Miller loop's P array) or a wave tree of complete additions through LDS and one
//                     XYZZ partial per block, or both.  Without coefficients it only sums (XYZZ partials or affine points).
// The host re-launches each fold on its partials until at most 64 are left and finishes those itself: the sum in 64-bit limbs,
// the product and final_exponentiation<Fq264Field> (0.6 ms; k_pairing_finish over the same partials, one lane, was measured at 18 ms).
// Not built: a multi-vector MSM over the gamma_abc table for keys with very many public inputs -- the ninp + 2 full-width
// multiplications of key points (s_0 alpha, s_j gamma_abc[j]) run on the context's helper threads under the device work.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "fsrng.hpp"
#include "g1_lincomb.cuh"
#include "groth16_int.hpp"
#include "pairing.cuh"
#include <string.h>

using namespace zk;

namespace {

using D2 = Fq2Field;
using H1 = Fq64Field;
using H2 = Fq264Field;
constexpr int GTW = 144;                                             // 32-bit words of a packed Fq12
constexpr int XW = 4 * G1Field::WORDS;                               // ... of a packed XYZZ point: 48
constexpr int FOLD_PER_LANE = 4;
constexpr size_t FOLD_SPAN = 64 * (size_t)FOLD_PER_LANE;
constexpr size_t MAX_LANES = ZK_PAIRING_MAX_LANES;
constexpr size_t SCALE_LDS = (size_t)LINCOMB_TAB * XW * 64 * 4;      // the window tables: 98 304 bytes
constexpr size_t SUM_LDS = (size_t)XW * 64 * 4;                      // the tree alone: 12 288 bytes

inline unsigned blocks_of(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

// ---- k_fq12_fold ------------------------------------------------------------------------------------------------------------------
// ext: the ABI's form (the test hook's input and output); else packed internal words as k_miller writes them
__device__ __forceinline__ Fq12<D2> fold_load(const uint32_t* w, bool ext) {
    Fq12<D2> f;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) {
            const Fq2 t = felt_load16<D2>(w + 24 * (3 * i + j));
            f.c[i].c[j] = ext ? D2::ext_to_int(t) : t;
        }
    return f;
}
__device__ __forceinline__ void fold_store(uint32_t* w, const Fq12<D2>& f, bool ext) {
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) felt_store16<D2>(w + 24 * (3 * i + j), ext ? D2::int_to_ext(f.c[i].c[j]) : f.c[i].c[j]);
}
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
    __shared__ uint32_t lds[GTW * 64];
    const uint32_t lane = threadIdx.x;
    const size_t base = blockIdx.x * FOLD_SPAN;
    const size_t have = n - base < FOLD_SPAN ? n - base : FOLD_SPAN;      // this block's values: the same on every lane
    const int rounds = (int)((have + 63) / 64);
    Fq12<D2> acc = fq12_one<D2>();
#pragma unroll 1
    for (int j = 0; j < rounds; j++) {
        const size_t i = base + (size_t)j * 64 + lane;
        Fq12<D2> f = fq12_one<D2>();
        if (i < n) f = fold_load(in + i * GTW, in_ext != 0);
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
    if (lane == 0) fold_store(out + (size_t)blockIdx.x * GTW, acc, out_ext != 0);
}

// ---- k_g1_scale_fold --------------------------------------------------------------------------------------------------------------
// g1_lincomb.hip's layout: word i of entry e of lane l at ((e 48 + i) 64 + l)
struct LdsTab {
    uint32_t* base;            // the wave's table + this lane
    __device__ __forceinline__ void put(int e, const XYZZ<G1Field>& p) {
        uint32_t w[XW];
        xyzz_store<G1Field>(w, p);
#pragma unroll
        for (int i = 0; i < XW; i++) base[(e * XW + i) * 64] = w[i];
    }
    __device__ __forceinline__ XYZZ<G1Field> get(int e) const {
        uint32_t w[XW];
#pragma unroll
        for (int i = 0; i < XW; i++) w[i] = base[(e * XW + i) * 64];
        return xyzz_load<G1Field>(w);
    }
};

// lane g < n: point g in_step of `in` (affine table form, or XYZZ with in_xyzz) times coeffs[4 g ..] (128 bits, low word first;
// coeffs = NULL: times one, and the launch needs SUM_LDS bytes of LDS only, else SCALE_LDS).  out_aff (or NULL): the n products as
// affine points.  out_part (or NULL): one XYZZ sum per block.
__global__ void __launch_bounds__(64) k_g1_scale_fold(const uint32_t* __restrict__ in, uint32_t in_step, int in_xyzz, const uint32_t* __restrict__ coeffs,
                                                      uint32_t n, uint32_t* __restrict__ out_aff, uint32_t* __restrict__ out_part) {
    extern __shared__ uint32_t lds[];
    const uint32_t lane = threadIdx.x, g = blockIdx.x * 64u + lane;
    LdsTab tab{lds + lane};
    XYZZ<G1Field> acc = xyzz_inf<G1Field>();
    if (coeffs) {
        Affine<G1Field> p = aff_inf<G1Field>();
        uint32_t k[4] = {0, 0, 0, 0};
        if (g < n) {
            p = aff_load16<G1Field>(in, (size_t)g * in_step);
            const uint4 c = reinterpret_cast<const uint4*>(coeffs)[g];
            k[0] = c.x; k[1] = c.y; k[2] = c.z; k[3] = c.w;
        }
        acc = lincomb_term<G1Field, LdsTab, 4>(p, k, tab);
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
            LdsTab other{lds + lane + s};
            acc = xyzz_add<G1Field>(acc, other.get(0));
        }
        __syncthreads();
    }
    if (lane == 0) xyzz_store16<G1Field>(out_part, blockIdx.x, acc);
}

// ---- launches -----------------------------------------------------------------------------------------------------------------------
int scale_fold_launch(zk_ctx* ctx, const uint32_t* in, uint32_t in_step, bool in_xyzz, const uint32_t* coeffs, size_t n, uint32_t* out_aff, uint32_t* out_part) {
    if (!ctx->lds_attr_done[ZK_LDS_SCALE_FOLD]) {
        ZK_HIP(ctx, hipFuncSetAttribute((const void*)k_g1_scale_fold, hipFuncAttributeMaxDynamicSharedMemorySize, (int)SCALE_LDS));
        ctx->lds_attr_done[ZK_LDS_SCALE_FOLD] = true;
    }
    hipLaunchKernelGGL(k_g1_scale_fold, blocks_of(n, 64), 64, coeffs ? SCALE_LDS : SUM_LDS, ctx->stream, in, in_step, in_xyzz ? 1 : 0, coeffs, (uint32_t)n,
                       out_aff, out_part);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
// the m XYZZ partials in a summed down to at most 64 (a and b: room for m and m / 64 + 1 points); *res says where they are
int g1_sum_down(zk_ctx* ctx, uint32_t* a, uint32_t* b, size_t* m, uint32_t** res) {
    while (*m > 64) {
        ZK_TRY(scale_fold_launch(ctx, a, 1, true, nullptr, *m, nullptr, b));
        *m = (*m + 63) / 64;
        std::swap(a, b);
    }
    *res = a;
    return ZK_OK;
}
// the m packed Miller values in `in` folded down to at most `limit` through the buffers a, b (room for m / SPAN + 1 values each)
int fq12_fold_down(zk_ctx* ctx, const uint32_t* in, uint32_t* a, uint32_t* b, size_t* m, size_t limit, const uint32_t** res) {
    while (*m > limit) {
        hipLaunchKernelGGL(k_fq12_fold, blocks_of(*m, FOLD_SPAN), 64, 0, ctx->stream, in, *m, a, 0, 0);
        ZK_HIP(ctx, hipGetLastError());
        *m = (*m + FOLD_SPAN - 1) / FOLD_SPAN;
        in = a;
        std::swap(a, b);
    }
    *res = in;
    return ZK_OK;
}

// ---- host halves --------------------------------------------------------------------------------------------------------------------
Fq12<H2> host_fq12_from_packed(const uint32_t* w) {
    Fq12<H2> f;
    for (int i = 0; i < 2; i++)
        for (int j = 0; j < 3; j++) f.c[i].c[j] = H2::from_dev(D2::load(w + 24 * (3 * i + j)));
    return f;
}
void host_gt_out(zk_gt* g, const Fq12<H2>& f) {
    uint32_t w[GTW];
    fq12_to_ext<H2>(w, f);
    memcpy(g, w, sizeof w);
}
// FE(prod of the m packed values): the end of every device path here
Fq12<H2> host_finish(const uint32_t* packed, size_t m) {
    Fq12<H2> acc = fq12_one<H2>(), r;
    for (size_t i = 0; i < m; i++) fq12_mul<H2>(acc, acc, host_fq12_from_packed(packed + i * GTW));
    final_exponentiation<H2>(r, acc);
    return r;
}

HF coeff_fr(const uint64_t* c) {      // lo + 2^64 hi
    static const HF two64 = HF::from_u64((uint64_t)1 << 32).sqr();
    return HF::from_u64(c[0]) + HF::from_u64(c[1]) * two64;
}
// s[0] = sum r_i, s[j + 1] = sum r_i x_{i,j} over the proofs [lo, hi)
void coeff_sums(const uint64_t* coeffs, const zk_fr* inputs, size_t ninp, size_t lo, size_t hi, HF* s) {
    for (size_t j = 0; j <= ninp; j++) s[j] = HF::zero();
    for (size_t i = lo; i < hi; i++) {
        const HF r = coeff_fr(coeffs + 2 * i);
        s[0] = s[0] + r;
        for (size_t j = 0; j < ninp; j++) s[j + 1] = s[j + 1] + r * HF::from_abi(inputs[i * ninp + j]);
    }
}
void coeff_words(const uint64_t* c, uint32_t k[8]) {
    k[0] = (uint32_t)c[0]; k[1] = (uint32_t)(c[0] >> 32); k[2] = (uint32_t)c[1]; k[3] = (uint32_t)(c[1] >> 32);
    k[4] = k[5] = k[6] = k[7] = 0;
}

struct HostLap {
    zk_ctx* ctx;
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* what) {                    // with zk_set_profiling: host wall-clock since the lap before into "verify_aggregate.<what>"
        if (!ctx->profiling) return;
        const auto now = std::chrono::steady_clock::now();
        auto& tm = ctx->timers[std::string("verify_aggregate.") + what];
        tm.ms += (float)std::chrono::duration<double, std::milli>(now - t).count();
        tm.count += 1;
        t = now;
    }
};

// what both aggregate forms refuse beyond their key's checks
bool agg_args_ok(size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const uint64_t* coeffs, const int* ok_all) {
    if (!count || !proofs || !coeffs || !ok_all || count > MAX_LANES - 3 || (ninp && !inputs)) return false;
    return true;
}

int aggregate_host(const zk_vk_host* vk, size_t count, const zk_fr* inputs, size_t ninp, const uint8_t* proofs, const uint64_t* coeffs, int* ok_all,
                   zk_gt* folded) {
    if (!vk || !agg_args_ok(count, inputs, ninp, proofs, coeffs, ok_all) || !vk->gamma_abc_g1 || vk->gamma_abc_len != ninp + 1) return ZK_ERR_ARG;
    if (!zk_words_below_q((const uint64_t*)&vk->alpha_g1, 2) || !zk_words_below_q((const uint64_t*)&vk->beta_g2, 4) ||
        !zk_words_below_q((const uint64_t*)&vk->gamma_g2, 4) || !zk_words_below_q((const uint64_t*)&vk->delta_g2, 4))
        return ZK_ERR_ARG;
    for (size_t i = 0; i <= ninp; i++)
        if (!zk_words_below_q((const uint64_t*)&vk->gamma_abc_g1[i], 2)) return ZK_ERR_ARG;
    for (size_t i = 0; i < count * ninp; i++)
        if (!zk_fr_words_valid(inputs[i].l)) return ZK_ERR_ARG;
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);
    std::vector<Affine<H1>> P(count + 3);
    std::vector<Affine<H2>> Q(count + 3);
    XYZZ<H1> c_sum = xyzz_inf<H1>();
    for (size_t i = 0; i < count; i++) {
        const uint8_t* pr = proofs + i * 192;
        Affine<G1Field> a, c;
        Affine<G2Field> b;
        if (!zk_host_decompress_g1(pr, &a) || !zk_host_decompress_g2(pr + 48, &b) || !zk_host_decompress_g1(pr + 144, &c)) return ZK_OK;
        if (!(zk_host_in_subgroup_g1(a) && zk_host_in_subgroup_g2(b) && zk_host_in_subgroup_g1(c))) return ZK_OK;
        uint32_t k[8];
        coeff_words(coeffs + 2 * i, k);
        P[i] = xyzz_to_affine<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(a)), k));
        Q[i] = aff_to_host64<G2Field>(b);
        c_sum = xyzz_add<H1>(c_sum, host64_scalar_mul<H1>(xyzz_from_affine<H1>(aff_to_host64<G1Field>(c)), k));
    }
    std::vector<HF> s(ninp + 1);
    coeff_sums(coeffs, inputs, ninp, 0, count, s.data());
    XYZZ<H1> pi = xyzz_inf<H1>();
    for (size_t j = 0; j <= ninp; j++) {
        uint32_t k[8];
        s[j].canon_words(k);
        pi = xyzz_add<H1>(pi, host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->gamma_abc_g1[j])), k));
    }
    uint32_t k0[8];
    s[0].canon_words(k0);
    P[count] = xyzz_to_affine<H1>(c_sum);
    Q[count] = aff_neg<H2>(zk_host_g2(&vk->delta_g2));
    P[count + 1] = xyzz_to_affine<H1>(pi);
    Q[count + 1] = aff_neg<H2>(zk_host_g2(&vk->gamma_g2));
    P[count + 2] = xyzz_to_affine<H1>(host64_scalar_mul<H1>(xyzz_from_affine<H1>(zk_host_g1(&vk->alpha_g1)), k0));
    Q[count + 2] = aff_neg<H2>(zk_host_g2(&vk->beta_g2));
    Fq12<H2> r;
    pairing_product<H2>(r, P.data(), Q.data(), count + 3);
    *ok_all = fq12_eq<H2>(r, fq12_one<H2>()) ? 1 : 0;
    if (folded) host_gt_out(folded, r);
    return ZK_OK;
}

int aggregate_dev(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t ninp, const uint8_t* proofs_host, const uint64_t* coeffs,
                  int* ok_all, zk_gt* folded) {
    if (!ctx || !pk || !agg_args_ok(count, inputs_host, ninp, proofs_host, coeffs, ok_all)) return ZK_ERR_ARG;
    if (!pk->gamma_abc || pk->gamma_abc->n == 0 || aff_is_inf<G2Field>(pk->gamma_g2))
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_verify_aggregate: the key has no verifying-key parts (gamma_g2, gamma_abc_g1)");
    if (pk->gamma_abc->n != ninp + 1) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_verify_aggregate: inputs_per_proof is not num_instance - 1");
    for (size_t i = 0; i < count * ninp; i++)
        if (!zk_fr_words_valid(inputs_host[i].l)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_groth16_verify_aggregate: a public input is not below r");
    *ok_all = 0;
    if (folded) memset(folded, 0, sizeof *folded);

    // host staging as zk_groth16_verify_batch: the compressed G1 points (A_k, C_k), the compressed B_k
    std::vector<uint8_t> g1c(count * 2 * 48), g2c(count * 96);
    for (size_t k = 0; k < count; k++) {
        const uint8_t* pr = proofs_host + k * 192;
        memcpy(&g1c[(2 * k) * 48], pr, 48);
        memcpy(&g2c[k * 96], pr + 48, 96);
        memcpy(&g1c[(2 * k + 1) * 48], pr + 144, 48);
    }
    std::vector<uint32_t> abc_w((ninp + 1) * 24);
    ZK_HIP(ctx, hipMemcpy(abc_w.data(), pk->gamma_abc->dev, abc_w.size() * 4, hipMemcpyDeviceToHost));

    const size_t n = count + 3, n_part = (count + 63) / 64, n_fold = (n + FOLD_SPAN - 1) / FOLD_SPAN;
    uint8_t *d_g1c, *d_g2c;
    uint32_t *d_coef, *ac, *b, *flags, *P, *Q, *ml, *part_a, *part_b, *fold_a, *fold_b;
    ZK_TRY(zk_scratch(ctx, "vfy_g1c", g1c.size(), (void**)&d_g1c));
    ZK_TRY(zk_scratch(ctx, "vfy_g2c", g2c.size(), (void**)&d_g2c));
    ZK_TRY(zk_scratch(ctx, "agg_coef", count * 16, (void**)&d_coef));
    ZK_TRY(zk_scratch(ctx, "vfy_ac", count * 2 * 96, (void**)&ac));
    ZK_TRY(zk_scratch(ctx, "vfy_b", count * 192, (void**)&b));
    ZK_TRY(zk_scratch(ctx, "agg_flags", 4, (void**)&flags));
    ZK_TRY(zk_scratch(ctx, "pair_p", n * 96, (void**)&P));
    ZK_TRY(zk_scratch(ctx, "pair_q", n * 192, (void**)&Q));
    ZK_TRY(zk_scratch(ctx, "pair_ml", n * GTW * 4, (void**)&ml));
    ZK_TRY(zk_scratch(ctx, "agg_part_a", n_part * XW * 4, (void**)&part_a));
    ZK_TRY(zk_scratch(ctx, "agg_part_b", (n_part / 64 + 1) * XW * 4, (void**)&part_b));
    ZK_TRY(zk_scratch(ctx, "agg_fold_a", n_fold * GTW * 4, (void**)&fold_a));
    ZK_TRY(zk_scratch(ctx, "agg_fold_b", (n_fold / FOLD_SPAN + 1) * GTW * 4, (void**)&fold_b));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_g1c, g1c.data(), g1c.size(), hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_g2c, g2c.data(), g2c.size(), hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(d_coef, coeffs, count * 16, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemsetAsync(flags, 0, 4, st));
    ZkPhaseTimer tm(ctx);                         // with zk_set_profiling: "verify_aggregate.<phase>", device time by events
    HostLap lap{ctx};
    tm.begin("verify_aggregate.k_decompress");
    ZK_TRY(zk_decompress_launch(ctx, 1, (const uint32_t*)d_g1c, 2 * count, ac, flags, nullptr));
    ZK_TRY(zk_decompress_launch(ctx, 2, (const uint32_t*)d_g2c, count, b, flags, nullptr));
    tm.end();
    // ALWAYS: the fold's soundness argument needs prime-order groups, and the Miller loop is not bilinear for a B outside G2
    tm.begin("verify_aggregate.k_subgroup");
    ZK_TRY(zk_subgroup_launch(ctx, 1, ac, 2 * count, flags, nullptr));
    ZK_TRY(zk_subgroup_launch(ctx, 2, b, count, flags, nullptr));
    tm.end();
    tm.begin("verify_aggregate.k_scale");
    ZK_TRY(scale_fold_launch(ctx, ac, 2, false, d_coef, count, P, nullptr));                    // r_i A_i -> P[0 .. count)
    ZK_HIP(ctx, hipMemcpyAsync(Q, b, count * 192, hipMemcpyDeviceToDevice, st));
    ZK_TRY(scale_fold_launch(ctx, ac + 24, 2, false, d_coef, count, nullptr, part_a));          // sum r_i C_i, a partial per wave
    size_t m_part = n_part;
    uint32_t* part;
    ZK_TRY(g1_sum_down(ctx, part_a, part_b, &m_part, &part));
    tm.end();

    // under the device work: the coefficient sums over ranges of proofs, then the ninp + 2 multiplications of key points side by side
    const size_t tasks = std::min<size_t>(8, (count + 4095) / 4096);
    std::vector<HF> part_s(tasks * (ninp + 1)), s(ninp + 1, HF::zero());
    const size_t per = (count + tasks - 1) / tasks;
    zk_over_ranges(ctx, tasks, tasks, [&](size_t lo, size_t hi) {
        for (size_t t = lo; t < hi; t++) coeff_sums(coeffs, inputs_host, ninp, std::min(count, t * per), std::min(count, (t + 1) * per), &part_s[t * (ninp + 1)]);
    });
    for (size_t t = 0; t < tasks; t++)
        for (size_t j = 0; j <= ninp; j++) s[j] = s[j] + part_s[t * (ninp + 1) + j];
    std::vector<XYZZ<H1>> key_mul(ninp + 2);      // s_j gamma_abc[j], then s_0 alpha
    auto mul_key = [&](size_t j) {
        uint32_t k[8];
        s[j <= ninp ? j : 0].canon_words(k);
        const Affine<G1Field> p = j <= ninp ? aff_load<G1Field>(&abc_w[24 * j]) : pk->alpha_g1;
        const XYZZ<H1> x = xyzz_from_affine<H1>(aff_to_host64<G1Field>(p));
        key_mul[j] = pk->points_in_subgroup ? host64_scalar_mul_glv(x, k) : host64_scalar_mul<H1>(x, k);
    };
    {
        std::vector<ZkTask<void>> ts;
        for (size_t j = 1; j < ninp + 2; j++) ts.push_back(zk_async(ctx, [&mul_key, j] { mul_key(j); }));
        mul_key(0);
    }
    lap.lap("host_sums");
    // (only now: a copy into pageable memory waits for the stream, and the host work above is meant to run under the kernels)
    std::vector<uint32_t> h_part(m_part * XW);
    uint32_t bad = 0;
    ZK_HIP(ctx, hipMemcpyAsync(h_part.data(), part, h_part.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipMemcpyAsync(&bad, flags, 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("wait_scale");
    if (bad) { tm.resolve(); return ZK_OK; }                       // a point off its curve or outside its subgroup: ok_all = 0, folded all-zero

    XYZZ<H1> c_sum = xyzz_inf<H1>(), pi = xyzz_inf<H1>();
    for (size_t i = 0; i < m_part; i++) c_sum = xyzz_add<H1>(c_sum, xyzz_to_host64<G1Field>(xyzz_load<G1Field>(&h_part[i * XW])));
    for (size_t j = 0; j <= ninp; j++) pi = xyzz_add<H1>(pi, key_mul[j]);
    struct Tail { uint32_t p[3 * 24]; uint32_t q[3 * 48]; } tail;
    aff_store<G1Field>(tail.p, aff_from_host64<G1Field>(xyzz_to_affine<H1>(c_sum)));
    aff_store<G1Field>(tail.p + 24, aff_from_host64<G1Field>(xyzz_to_affine<H1>(pi)));
    aff_store<G1Field>(tail.p + 48, aff_from_host64<G1Field>(xyzz_to_affine<H1>(key_mul[ninp + 1])));
    aff_store<G2Field>(tail.q, aff_neg<G2Field>(pk->delta_g2));
    aff_store<G2Field>(tail.q + 48, aff_neg<G2Field>(pk->gamma_g2));
    aff_store<G2Field>(tail.q + 96, aff_neg<G2Field>(pk->beta_g2));
    ZK_HIP(ctx, hipMemcpyAsync(P + count * 24, tail.p, sizeof tail.p, hipMemcpyHostToDevice, st));
    ZK_HIP(ctx, hipMemcpyAsync(Q + count * 48, tail.q, sizeof tail.q, hipMemcpyHostToDevice, st));
    tm.begin("verify_aggregate.k_miller");
    ZK_TRY(zk_miller_launch(ctx, P, Q, n, ml));
    tm.end();
    size_t m = n;
    const uint32_t* res;
    tm.begin("verify_aggregate.k_fold");
    ZK_TRY(fq12_fold_down(ctx, ml, fold_a, fold_b, &m, 64, &res));
    tm.end();
    std::vector<uint32_t> h_ml(m * GTW);
    ZK_HIP(ctx, hipMemcpyAsync(h_ml.data(), res, h_ml.size() * 4, hipMemcpyDeviceToHost, st));
    ZK_HIP(ctx, hipStreamSynchronize(st));
    lap.lap("wait_miller");
    const Fq12<H2> r = host_finish(h_ml.data(), m);
    lap.lap("host_finish");
    tm.resolve();
    *ok_all = fq12_eq<H2>(r, fq12_one<H2>()) ? 1 : 0;
    if (folded) host_gt_out(folded, r);
    return ZK_OK;
}

}  // namespace

extern "C" int zk_groth16_verify_aggregate_coeffs(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                                  const uint8_t* proofs_host, const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN(ctx)
    return aggregate_dev(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, coeffs, ok_all, folded);
    ZK_API_END
}

extern "C" int zk_groth16_verify_aggregate_host(const zk_vk_host* vk, size_t count, const zk_fr* inputs, size_t inputs_per_proof, const uint8_t* proofs,
                                                const uint64_t* coeffs, int* ok_all, zk_gt* folded) {
    ZK_API_BEGIN_NOCTX
    return aggregate_host(vk, count, inputs, inputs_per_proof, proofs, coeffs, ok_all, folded);
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

extern "C" int zk_groth16_verify_aggregate(zk_ctx* ctx, const zk_pk* pk, size_t count, const zk_fr* inputs_host, size_t inputs_per_proof,
                                           const uint8_t* proofs_host, const uint8_t seed[32], int* ok_all, int* ok_each) {
    ZK_API_BEGIN(ctx)
    if (!seed || !count || count > MAX_LANES - 3) return ZK_ERR_ARG;
    std::vector<uint64_t> coeffs(2 * count);
    ZK_TRY(zk_verify_aggregate_coeffs_from_seed(seed, count, coeffs.data()));
    ZK_TRY(aggregate_dev(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, coeffs.data(), ok_all, nullptr));
    if (!ok_each) return ZK_OK;
    if (*ok_all) {
        for (size_t i = 0; i < count; i++) ok_each[i] = 1;
        return ZK_OK;
    }
    return zk_groth16_verify_batch_checked(ctx, pk, count, inputs_host, inputs_per_proof, proofs_host, ok_each);
    ZK_API_END
}

extern "C" int zk_pairing_product_long(zk_ctx* ctx, const zk_g1_affine* p, const zk_g2_affine* q, size_t n, zk_gt* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !p || !q || !out || !n || n > MAX_LANES) return ZK_ERR_ARG;
    const size_t n_fold = (n + FOLD_SPAN - 1) / FOLD_SPAN;
    uint32_t *dp, *dq, *ml, *fold_a, *fold_b;
    ZK_TRY(zk_scratch(ctx, "pair_p", n * 96, (void**)&dp));
    ZK_TRY(zk_scratch(ctx, "pair_q", n * 192, (void**)&dq));
    ZK_TRY(zk_scratch(ctx, "pair_ml", n * GTW * 4, (void**)&ml));
    ZK_TRY(zk_scratch(ctx, "agg_fold_a", n_fold * GTW * 4, (void**)&fold_a));
    ZK_TRY(zk_scratch(ctx, "agg_fold_b", (n_fold / FOLD_SPAN + 1) * GTW * 4, (void**)&fold_b));
    ZK_HIP(ctx, hipMemcpyAsync(dp, p, n * 96, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync(dq, q, n * 192, hipMemcpyHostToDevice, ctx->stream));
    ZK_TRY(zk_miller_ext_launch(ctx, dp, dq, n, ml));
    size_t m = n;
    const uint32_t* res;
    ZK_TRY(fq12_fold_down(ctx, ml, fold_a, fold_b, &m, 64, &res));
    std::vector<uint32_t> h_ml(m * GTW);
    ZK_HIP(ctx, hipMemcpyAsync(h_ml.data(), res, h_ml.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    host_gt_out(out, host_finish(h_ml.data(), m));
    return ZK_OK;
    ZK_API_END
}

extern "C" size_t zk_diag_fq12_fold_span(void) { return FOLD_SPAN; }

extern "C" int zk_diag_fq12_fold_dev(zk_ctx* ctx, const zk_gt* in, size_t n, zk_gt* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !in || !out || !n || n > MAX_LANES) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&in[i], 12)) return ZK_ERR_ARG;
    const size_t n_fold = (n + FOLD_SPAN - 1) / FOLD_SPAN;
    uint32_t *d_in, *a, *b;
    ZK_TRY(zk_scratch(ctx, "pair_ml", n * GTW * 4, (void**)&d_in));
    ZK_TRY(zk_scratch(ctx, "agg_fold_a", n_fold * GTW * 4, (void**)&a));
    ZK_TRY(zk_scratch(ctx, "agg_fold_b", (n_fold / FOLD_SPAN + 1) * GTW * 4, (void**)&b));
    ZK_HIP(ctx, hipMemcpyAsync(d_in, in, n * GTW * 4, hipMemcpyHostToDevice, ctx->stream));
    // the kernel alone, down to ONE value (n = 1: one launch all the same); the first launch reads, the last writes the ABI's form
    const uint32_t* src = d_in;
    size_t m = n;
    bool first = true;
    do {
        const size_t m_out = (m + FOLD_SPAN - 1) / FOLD_SPAN;
        hipLaunchKernelGGL(k_fq12_fold, blocks_of(m, FOLD_SPAN), 64, 0, ctx->stream, src, m, a, first ? 1 : 0, m_out == 1 ? 1 : 0);
        ZK_HIP(ctx, hipGetLastError());
        m = m_out;
        src = a;
        std::swap(a, b);
        first = false;
    } while (m > 1);
    ZK_HIP(ctx, hipMemcpyAsync(out, src, GTW * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
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
    const size_t n_part = (n + 63) / 64;
    uint32_t *d_pts, *d_coef = nullptr, *d_aff = nullptr, *part_a, *part_b;
    ZK_TRY(zk_scratch(ctx, "agg_diag_pts", n * 96, (void**)&d_pts));
    if (coeffs) ZK_TRY(zk_scratch(ctx, "agg_coef", n * 16, (void**)&d_coef));
    if (scaled_out) ZK_TRY(zk_scratch(ctx, "agg_diag_aff", n * 96, (void**)&d_aff));
    ZK_TRY(zk_scratch(ctx, "agg_part_a", n_part * XW * 4, (void**)&part_a));
    ZK_TRY(zk_scratch(ctx, "agg_part_b", (n_part / 64 + 1) * XW * 4, (void**)&part_b));
    hipStream_t st = ctx->stream;
    ZK_HIP(ctx, hipMemcpyAsync(d_pts, w.data(), n * 96, hipMemcpyHostToDevice, st));
    if (coeffs) ZK_HIP(ctx, hipMemcpyAsync(d_coef, coeffs, n * 16, hipMemcpyHostToDevice, st));
    ZK_TRY(scale_fold_launch(ctx, d_pts, 1, false, d_coef, n, d_aff, part_a));
    size_t m = n_part;
    uint32_t* part;
    ZK_TRY(g1_sum_down(ctx, part_a, part_b, &m, &part));
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
