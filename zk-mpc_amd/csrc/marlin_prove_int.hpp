// marlin_prove_int.hpp -- what the Marlin provers share (marlin_prove.hip: one proof, plain or over shares; marlin_prove_batch.hip:
// count proofs of one index in lock-step, plain or over shares): the oracle table, the sum-checks' error texts, the entry points'
// argument checks, the sizes of a proof (Shape), the query set with its linear combinations, the host halves of the polynomial
// commitment's openings, Proof::serialize, and ProofState: one proof's host state with its host steps -- the transcript
// (marlin_transcript.hpp), the blinding scalars, the commitments, the challenges, the opening plans, the proof's bytes.
// Everything here is host code; nothing in it depends on how many proofs are in flight.
#pragma once
#include "../../include/zkmpc_hip.h"
#include "hostgroup.hpp"
#include "internal.hpp"
#include "marlin_bytes.hpp"
#include "marlin_lc.hpp"
#include "marlin_transcript.hpp"
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

// The sizes every step reads
struct Shape {
    const Dom H, K, X, B;
    const size_t n, ni, md, nwq;                  // |H|, |X|, the mask polynomial's degree (zk_bound = 1), coefficients of w
    const Dom MUL;                                // the multiplication domain of round 2
    const size_t h1n, h2n, max_degree, nv;        // coefficients of h_1 and h_2; of the SRS; the padded assignment's length
    size_t index_n[12], cn[2];                    // the index polynomials' lengths; the longest polynomial opened at beta / at gamma
    Shape(const zk_marlin_index* ix, const zk_bases* powers_g)
        : H(ix->num_constraints), K(ix->num_non_zero), X(ix->num_instance), B(3 * K.size - 3), n(H.size), ni(ix->num_instance), md(3 * n + 2 - 3),
          nwq(n + 1 - X.size), MUL(std::max(std::max(md + 1, n + 2 * n + 1), n + n + 1)), h1n(std::min(MUL.size - n, 2 * n + 2 - 1)), h2n(B.size - K.size),
          max_degree(powers_g->n - 1), nv(ix->num_variables) {
        for (int i = 0; i < 12; i++) index_n[i] = ix->index_polys[i].n;
        cn[0] = std::max(std::max(md + 1, h1n), n + 1);
        cn[1] = std::max(h2n, K.size - 1);
        for (int i = 0; i < 12; i++) cn[1] = std::max(cn[1], index_n[i]);
    }
    size_t bound(Oracle o) const { return (ORACLES[o].bound == Bound::H ? n : K.size) - 2; }
    size_t oracle_n(Oracle o) const {
        switch (o) {
            case O_W: return nwq;
            case O_Z_A: case O_Z_B: return n + 1;
            case O_MASK_POLY: return md + 1;
            case O_T: return n;
            case O_G_1: return n - 1;
            case O_H_1: return h1n;
            case O_G_2: return K.size - 1;
            case O_H_2: return h2n;
            default: return index_n[o - O_A_ROW];
        }
    }
};

// ---- the query set and its linear combinations ----
// What the prover evaluates, in the order both provers ask for it: z_b, g_1, t at beta; g_2 and row, col, row_col of A, B, C at gamma
// (over shares z_b and g_1 are the two that are opened: they come first)
struct QueryValue { Oracle o; bool at_gamma; };
enum : int { QV_Z_B, QV_G_1, QV_T, QV_G_2, QV_INDEX, N_QUERY_VALUES = QV_INDEX + 9 };      // QV_INDEX + 3 m: row, col, row_col of matrix m
constexpr QueryValue QUERY_VALUES[N_QUERY_VALUES] = {
    {O_Z_B, false}, {O_G_1, false}, {O_T, false}, {O_G_2, true},
    {O_A_ROW, true}, {O_A_COL, true}, {O_A_ROW_COL, true}, {O_B_ROW, true}, {O_B_COL, true}, {O_B_ROW_COL, true},
    {O_C_ROW, true}, {O_C_COL, true}, {O_C_ROW_COL, true},
};
static_assert(QUERY_VALUES[QV_G_1].o == O_G_1 && QUERY_VALUES[QV_G_2].o == O_G_2 && QUERY_VALUES[QV_INDEX + 3 * 2 + 1].o == index_of(2, COL), "the order QV_* names");
struct QuerySet {
    std::vector<HF> evaluations;                  // in the proof's (alphabetic) order
    std::vector<LinComb> queries[2];              // the combinations opened at beta / at gamma, in query-set order
};
// construct_linear_combinations (ahp/mod.rs:112-290): the coefficients are marlin_lc.hpp's, shared with the verifier
inline QuerySet query_set(const Dom& H, const Dom& K, const Dom& X, const HF& alpha, const HF eta[3], const HF& beta, const HF& gamma,
                          const HF v[N_QUERY_VALUES], const HF* pub) {
    const HF ba = beta * alpha, one = HF::one();
    HF d[3];                                                                  // a_denom, b_denom, c_denom
    for (int m = 0; m < 3; m++) d[m] = ba - alpha * v[QV_INDEX + 3 * m] - beta * v[QV_INDEX + 3 * m + 1] + v[QV_INDEX + 3 * m + 2];
    MarlinLcIn in{alpha, {eta[0], eta[1], eta[2]}, beta, gamma, v[QV_Z_B], v[QV_T], v[QV_G_1], v[QV_G_2], {d[0], d[1], d[2]}, pub};
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
    q.evaluations = {da, db, dc, v[QV_G_1], v[QV_G_2], v[QV_T], v[QV_Z_B]};      // a_denom, b_denom, c_denom, g_1, g_2, t, z_b
    return q;
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

// ---- one proof's host state: what crosses the steps, and the steps' host halves.  The provers differ in where the points and the
// values come from (one proof: early MSMs, named scratch; a chunk: strided kernels over one Layout), not in what happens to them here ----
struct ProofState {
    Transcript fs;
    std::vector<HF> pub;                          // seed: the public input, its leading 1 included
    Blinds rands[N_ORACLES];                      // draw_blinds: the blinding polynomials (index oracles: none)
    Comm comms[N_PROVER];                         // commitments
    HF alpha, eta[3], v_h_alpha;                  // challenges(1): alpha, eta (a, b, c), v_H(alpha)
    HF beta, vv, gamma, xi;                       // challenges(2): beta, v_H(alpha) v_H(beta); challenges(3): gamma; evaluated: xi
    QuerySet qs;                                  // evaluated
    OpenPlan plan[2];                             // evaluated: the openings at beta / at gamma
    Affine<G1Field> wit[2];                       // witnesses: per query point the witness, and random_v if hiding (blinds_at)
    bool has_rv[2] = {false, false}; HF rvs[2];
    int rc = ZK_OK; std::string err;              // a batch's: the first failure of this proof
    ProofState() = default;
    ProofState(const ProofState&) = delete; ProofState& operator=(const ProofState&) = delete;

    // x: the ni opened values of the assignment's instance part (x[0], the constant 1, is not read)
    void seed(const zk_marlin_index* ix, const zk_fr* x, size_t ni) {
        pub.assign(ni, HF::one());
        for (size_t i = 1; i < ni; i++) pub[i] = HF::from_abi(x[i]);
        fs = Transcript(ix->ivk_bytes, ix->ivk_len, pub);
    }
    // MarlinKZG10::commit's blinding polynomials for one round, in the reference's rng order (marlin_pc/mod.rs:172-243, hiding bound 1)
    int draw_blinds(int round, zk_rng* rng) {
        for (Oracle o : round_oracles(round)) {
            if (!ORACLES[o].hiding) continue;
            zk_fr f;
            for (int i = 0; i < 3; i++) { ZK_TRY(zk_rng_next_fr(rng, &f)); rands[o].plain.push_back(HF::from_abi(f)); }
            for (int i = 0; i < 3 && oracle_bounded(o); i++) { ZK_TRY(zk_rng_next_fr(rng, &f)); rands[o].shifted.push_back(HF::from_abi(f)); }
        }
        return ZK_OK;
    }
    // pts: the round's (opened) commitments in the round's order, a degree-bounded oracle's shifted commitment behind its own
    void commitments(int round, const std::vector<zk_g1_projective>& pts) {
        const std::vector<Affine<G1Field>> aff = batch_to_aff(pts);
        size_t ai = 0;
        for (Oracle o : round_oracles(round)) {
            Comm& c = comms[o];
            c.c = aff[ai++];
            c.has_shift = oracle_bounded(o);
            c.s = c.has_shift ? aff[ai++] : aff_inf<G1Field>();
        }
    }
    // the round's commitments into the transcript; the round's challenges and what follows from them alone
    void challenges(int round, const Shape& s) {
        const std::vector<Oracle> os = round_oracles(round);
        const Comm* first = &comms[os.front()];                                  // (ORACLES lists a round's oracles side by side)
        if (round == 1) {
            const Transcript::Round1 c = fs.round1(first, os.size(), s.H);
            alpha = c.alpha;
            for (int m = 0; m < 3; m++) eta[m] = c.eta[m];
            v_h_alpha = s.H.vanishing(alpha);
        } else if (round == 2) {
            beta = fs.round2(first, os.size(), s.H);
            vv = v_h_alpha * s.H.vanishing(beta);
        } else {
            gamma = fs.round3(first, os.size());
        }
    }
    // vals: the (opened) values QUERY_VALUES lists.  Out: qs, absorbed; xi; the opening plans
    void evaluated(const zk_fr vals[N_QUERY_VALUES], const Shape& s) {
        HF v[N_QUERY_VALUES];
        for (int i = 0; i < N_QUERY_VALUES; i++) v[i] = HF::from_abi(vals[i]);
        qs = query_set(s.H, s.K, s.X, alpha, eta, beta, gamma, v, pub.data());
        xi = fs.evaluations(qs.evaluations);
        for (int q = 0; q < 2; q++) plan[q] = open_plan(qs.queries[q], xi, rands);
    }
    const HF& point(int q) const { return q ? gamma : beta; }
    // what the blinding polynomials contribute to the opening at query point q; has_rv, rvs (over shares: this party's, until opened)
    OpenBlinds blinds_at(int q) {
        OpenBlinds ob = open_blinds(plan[q], point(q), rands);
        has_rv[q] = ob.hiding;
        if (ob.hiding) rvs[q] = ob.rv;
        return ob;
    }
    void witnesses(const zk_g1_projective pts[2]) {
        const std::vector<Affine<G1Field>> wa = batch_to_aff({pts[0], pts[1]});
        wit[0] = wa[0]; wit[1] = wa[1];
    }
    // Proof::serialize (data_structures.rs:99-110, derive order) into dst[0 .. cap); false: it does not fit
    bool write(uint8_t* dst, size_t cap, size_t* len) const {
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
        u64(qs.evaluations.size());
        for (auto& e : qs.evaluations) e.bytes(out);
        u64(3); out.push_back(0); out.push_back(0); out.push_back(0);           // three EmptyMessage
        u64(2);
        for (int q = 0; q < 2; q++) {
            g1c(wit[q]);
            out.push_back(has_rv[q] ? 1 : 0);
            if (has_rv[q]) rvs[q].bytes(out);
        }
        out.push_back(0);                                                        // BatchLCProof.evals = None
        if (out.size() > cap) return false;
        memcpy(dst, out.data(), out.size());
        *len = out.size();
        return true;
    }
};

}  // namespace marlin
}  // namespace zk
