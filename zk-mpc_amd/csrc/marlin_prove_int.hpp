// marlin_prove_int.hpp -- what the Marlin provers share (marlin_prove.hip: one proof, plain or over shares; marlin_prove_batch.hip:
// count proofs of one index in lock-step, plain or over shares): the oracle table, the sum-checks' error texts, the host halves of the polynomial commitment's openings, the
// entry points' argument checks, the transcript's seed, the query set with its linear combinations, and Proof::serialize.
// Everything here is host code; nothing in it depends on how many proofs are in flight.
#pragma once
#include "../../include/zkmpc_hip.h"
#include "hostgroup.hpp"
#include "internal.hpp"
#include "marlin_bytes.hpp"
#include "marlin_lc.hpp"
#include <algorithm>
#include <string>
#include <utility>
#include <vector>

namespace zk {
namespace marlin {

struct Poly { char* p = nullptr; size_t n = 0; };        // n coefficients on the device

// ---- the oracles: the nine the prover sends, in the order their rounds commit (and serialise) them, then the index's twelve ----
enum Oracle : int {
    O_W, O_Z_A, O_Z_B, O_MASK_POLY, O_T, O_G_1, O_H_1, O_G_2, O_H_2,
    O_A_ROW, O_A_COL, O_A_VAL, O_A_ROW_COL, O_B_ROW, O_B_COL, O_B_VAL, O_B_ROW_COL, O_C_ROW, O_C_COL, O_C_VAL, O_C_ROW_COL,
    N_ORACLES, N_PROVER = O_A_ROW, O_NONE = -1
};
enum IndexPart : int { ROW, COL, VAL, ROW_COL };                        // the index oracles of matrix m = 0 (A), 1 (B), 2 (C)
constexpr Oracle index_of(int m, IndexPart part) { return Oracle(O_A_ROW + 4 * m + part); }
static_assert(index_of(0, ROW_COL) == O_A_ROW_COL && index_of(1, VAL) == O_B_VAL && index_of(2, COL) == O_C_COL, "Oracle lists row, col, val, row_col per matrix");
enum class Bound { None, H, K };            // degree bound: none, |H| - 2, |K| - 2
enum class EarlyMsm { No, Plain, Always };  // may its MSM start before the round's batch: never / not over shares / in every mode
// label: error texts | round that commits it, 1 - 3 (0: an index oracle) | hiding: committed with a blinding polynomial (bound 1) | shared:
// witness-dependent (mpc.py: Party.SHARED_POLYS; t, g_2, h_2 and the index are public) | early: see Marlin::start_early
struct OracleInfo { const char* label; int round; bool hiding; Bound bound; bool shared; EarlyMsm early; };
constexpr OracleInfo index_oracle(const char* label) { return {label, 0, false, Bound::None, false, EarlyMsm::No}; }
constexpr OracleInfo ORACLES[N_ORACLES] = {
    {"w", 1, true, Bound::None, true, EarlyMsm::No},
    {"z_a", 1, true, Bound::None, true, EarlyMsm::No},
    {"z_b", 1, true, Bound::None, true, EarlyMsm::No},
    {"mask_poly", 1, false, Bound::None, true, EarlyMsm::Plain},     // (over shares every lane's job stays in the batch)
    {"t", 2, false, Bound::None, false, EarlyMsm::Always},
    {"g_1", 2, true, Bound::H, true, EarlyMsm::No},
    {"h_1", 2, false, Bound::None, true, EarlyMsm::No},
    {"g_2", 3, false, Bound::K, false, EarlyMsm::Always},
    {"h_2", 3, false, Bound::None, false, EarlyMsm::No},
    index_oracle("a_row"), index_oracle("a_col"), index_oracle("a_val"), index_oracle("a_row_col"), index_oracle("b_row"), index_oracle("b_col"),
    index_oracle("b_val"), index_oracle("b_row_col"), index_oracle("c_row"), index_oracle("c_col"), index_oracle("c_val"), index_oracle("c_row_col"),
};
inline std::vector<Oracle> round_oracles(int round) {
    std::vector<Oracle> v;
    for (int o = 0; o < N_PROVER; o++) if (ORACLES[o].round == round) v.push_back((Oracle)o);
    return v;
}
inline bool oracle_bounded(Oracle o) { return ORACLES[o].bound != Bound::None; }

// The sum-checks' failures, as every prover words them (a batch puts "proof <k>: " in front)
constexpr const char* OUTER_NOT_ZERO = "zk_marlin_prove: outer sum-check: the sum over H is not zero (unsatisfied constraint system)";
constexpr const char* INNER_NOT_DIVISIBLE = "zk_marlin_prove: inner sum-check: a - b f is not divisible by v_K";

inline HF host_eval(const std::vector<HF>& c, const HF& x) {
    HF acc = HF::zero();
    for (size_t i = c.size(); i-- > 0;) acc = acc * x + c[i];
    return acc;
}
inline std::vector<HF> host_div_linear(const std::vector<HF>& c, const HF& z) {   // quotient of p / (X - z)
    std::vector<HF> q(c.size() > 1 ? c.size() - 1 : 0, HF::zero());
    HF acc = HF::zero();
    for (size_t i = c.size(); i-- > 1;) { acc = c[i] + acc * z; q[i - 1] = acc; }
    return q;
}
inline void acc_scaled(std::vector<HF>& dst, const std::vector<HF>& src, const HF& k) {
    if (dst.size() < src.size()) dst.resize(src.size(), HF::zero());
    for (size_t i = 0; i < src.size(); i++) dst[i] = dst[i] + src[i] * k;
}

struct Term { HF c; Oracle o; };                // o = O_NONE: the constant term (LCTerm::One)
using LinComb = std::vector<Term>;
struct Blinds { std::vector<HF> plain, shifted; };      // commit: an oracle's blinding polynomials (index oracles: none)

// ---- the entry points' argument checks (Marlin::prove's own errors, lib.rs:152-170, and what this library adds) ----
inline int check_index_and_srs(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g) {
    if (powers_g->group != 1 || powers_gamma_g->group != 1 || powers_gamma_g->n < 3) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: SRS tables");
    if (ix->num_constraints != ix->num_variables) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: NonSquareMatrix");
    if (ix->num_instance == 0 || (ix->num_instance & (ix->num_instance - 1))) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: InvalidPublicInputLength");
    return ZK_OK;
}
// n = |H|, k = |K|, b = |B| (the domain of 3|K| - 3 coefficients), max_degree of the SRS
inline int check_sizes(zk_ctx* ctx, size_t max_degree, size_t n, size_t k, size_t b) {
    const size_t need = std::max(std::max(2 * n - 1, 3 * n - 1), std::max(n, 3 * k - 3));   // AHPForR1CS::max_degree (ahp/mod.rs:75-97)
    if (max_degree < need) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: IndexTooLarge for this SRS");
    if (b < 4 * k - 3) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: |K| < 4 is not supported by this entry point");
    return ZK_OK;
}

// The transcript seed: PROTOCOL_NAME | index_vk | public_input (lib.rs:161-164); pub = the public input, its leading 1 included
inline std::vector<uint8_t> transcript_seed(const zk_marlin_index* ix, const std::vector<HF>& pub) {
    std::vector<uint8_t> seed;
    const char* name = "MARLIN-2019";
    seed.insert(seed.end(), name, name + 11);
    seed.insert(seed.end(), ix->ivk_bytes, ix->ivk_bytes + ix->ivk_len);
    for (size_t i = 1; i < pub.size(); i++) pub[i].bytes(seed);
    return seed;
}

// ---- the query set and its linear combinations ----
// What the prover evaluates: z_b, g_1, t at beta; g_2 and row, col, row_col of A, B, C at gamma
struct QueryValues { HF z_b_beta, g_1_beta, t_beta, g_2_gamma, row[3], col[3], row_col[3]; };
struct QuerySet {
    std::vector<HF> evaluations;                  // in the proof's (alphabetic) order
    std::vector<LinComb> queries[2];              // the combinations opened at beta / at gamma, in query-set order
};
// construct_linear_combinations (ahp/mod.rs:112-290): the coefficients are marlin_lc.hpp's, shared with the verifier
inline QuerySet query_set(const Dom& H, const Dom& K, const Dom& X, const HF& alpha, const HF eta[3], const HF& beta, const HF& gamma,
                          const QueryValues& v, const HF* pub) {
    const HF ba = beta * alpha, one = HF::one();
    HF d[3];                                                                  // a_denom, b_denom, c_denom
    for (int m = 0; m < 3; m++) d[m] = ba - alpha * v.row[m] - beta * v.col[m] + v.row_col[m];
    MarlinLcIn in{alpha, {eta[0], eta[1], eta[2]}, beta, gamma, v.z_b_beta, v.t_beta, v.g_1_beta, v.g_2_gamma, {d[0], d[1], d[2]}, pub};
    const MarlinLc c = marlin_lc(H, K, X, in);
    const HF da = d[0], db = d[1], dc = d[2];
    const LinComb outer = {{one, O_MASK_POLY}, {c.z_a, O_Z_A}, {c.outer_c_zb, O_NONE}, {c.w, O_W}, {c.outer_c_x, O_NONE}, {c.h_1, O_H_1},
                           {c.outer_c_g1, O_NONE}};
    const LinComb inner = {{c.val[0], O_A_VAL}, {c.val[1], O_B_VAL}, {c.val[2], O_C_VAL}, {c.inner_c, O_NONE}, {c.h_2, O_H_2}};
    auto denom_lc = [&](int m) {
        return LinComb{{ba, O_NONE}, {alpha.neg(), index_of(m, ROW)}, {beta.neg(), index_of(m, COL)}, {one, index_of(m, ROW_COL)}};
    };
    QuerySet q;
    // the query set, labels in alphabetic order: {g_1, outer_sumcheck, t, z_b} at beta, {a_denom, b_denom, c_denom, g_2, inner_sumcheck} at gamma
    q.queries[0] = {{{one, O_G_1}}, outer, {{one, O_T}}, {{one, O_Z_B}}};
    q.queries[1] = {denom_lc(0), denom_lc(1), denom_lc(2), {{one, O_G_2}}, inner};
    q.evaluations = {da, db, dc, v.g_1_beta, v.g_2_gamma, v.t_beta, v.z_b_beta};      // a_denom, b_denom, c_denom, g_1, g_2, t, z_b
    return q;
}
// the opening challenge: u128::rand(&mut fs_rng).into()  (lib.rs:300)
inline int opening_challenge(zk_rng* fs, HF* xi) {
    uint64_t w[2];
    ZK_TRY(zk_rng_next_u128(fs, w));
    *xi = HF::from_u64(w[0]) + HF::from_u64(w[1]) * HF::from_u64((uint64_t)1 << 32) * HF::from_u64((uint64_t)1 << 32);
    return ZK_OK;
}

// open_combinations for ONE query point (marlin/mod.rs:213-306, marlin_pc/mod.rs:245-340), its host half: which polynomials enter
// the combination with which accumulated coefficient (first-use order), which degree-bounded oracles are opened shifted with which
// power of xi, and the same combinations of the blinding polynomials
struct OpenPlan {
    std::vector<std::pair<Oracle, HF>> terms, shifted;
    std::vector<HF> r_comb, sr;
};
inline OpenPlan open_plan(const std::vector<LinComb>& queries, const HF& xi, const Blinds* rands) {
    OpenPlan p;
    HF cj = HF::one();                                                   // xi^j
    for (const LinComb& lc : queries) {
        const HF c0 = cj;
        cj = cj * xi;
        for (const Term& t : lc) {
            if (t.o == O_NONE) continue;
            auto it = std::find_if(p.terms.begin(), p.terms.end(), [&](const std::pair<Oracle, HF>& e) { return e.first == t.o; });
            if (it == p.terms.end()) p.terms.push_back({t.o, t.c * c0}); else it->second = it->second + t.c * c0;
            acc_scaled(p.r_comb, rands[t.o].plain, t.c * c0);
        }
        if (lc.size() == 1 && oracle_bounded(lc[0].o)) {                 // a degree-bounded oracle queried by itself
            const HF c1 = cj;
            cj = cj * xi;
            p.shifted.push_back({lc[0].o, c1});
            acc_scaled(p.sr, rands[lc[0].o].shifted, c1);
        }
    }
    return p;
}
// ... and what the blinding polynomials contribute at the point z: the coefficients of the witness's blinding term over
// powers_of_gamma_g (plain / shifted; empty: none) and random_v
struct OpenBlinds { bool hiding = false; std::vector<HF> plain_w, shifted_w; HF rv; };
inline OpenBlinds open_blinds(const OpenPlan& p, const HF& z, const Blinds* rands) {
    OpenBlinds b;
    for (auto& v : p.r_comb) b.hiding = b.hiding || !v.is_zero();
    if (b.hiding) {
        b.plain_w = host_div_linear(p.r_comb, z);
        b.rv = host_eval(p.r_comb, z);
    }
    for (auto& sh : p.shifted) {
        const std::vector<HF>& sb = rands[sh.first].shifted;
        if (!sb.empty()) acc_scaled(b.shifted_w, host_div_linear(sb, z), sh.second);
    }
    if (!p.shifted.empty() && b.hiding) b.rv = b.rv + host_eval(p.sr, z);
    return b;
}

// Proof::serialize (data_structures.rs:99-110, derive order)
inline std::vector<uint8_t> proof_bytes(const Comm* comms, const std::vector<HF>& evaluations, const Affine<G1Field> wit[2], const bool has_rv[2],
                                        const HF rvs[2]) {
    std::vector<uint8_t> out;
    auto u64 = [&](uint64_t v) { for (int i = 0; i < 8; i++) out.push_back((uint8_t)(v >> (8 * i))); };
    auto g1c = [&](const Affine<G1Field>& p) { uint8_t b[48]; g1_serialize(p, b); out.insert(out.end(), b, b + 48); };
    u64(3);
    for (int round = 1; round <= 3; round++) {
        const std::vector<Oracle> os = round_oracles(round);
        u64(os.size());
        for (Oracle o : os) {
            const Comm& c = comms[o];
            g1c(c.c);
            out.push_back(c.has_shift ? 1 : 0);
            if (c.has_shift) g1c(c.s);
        }
    }
    u64(evaluations.size());
    for (auto& e : evaluations) e.bytes(out);
    u64(3); out.push_back(0); out.push_back(0); out.push_back(0);           // three EmptyMessage
    u64(2);
    for (int q = 0; q < 2; q++) {
        g1c(wit[q]);
        out.push_back(has_rv[q] ? 1 : 0);
        if (has_rv[q]) rvs[q].bytes(out);
    }
    out.push_back(0);                                                        // BatchLCProof.evals = None
    return out;
}

}  // namespace marlin
}  // namespace zk
