// marlin_agg_plan.hpp -- every size of the device form of the aggregated Marlin check (marlin_verify.hip: aggregate_dev) and of the
// sum of many G1 terms behind it (g1_term_fold.hip), as plain integer arithmetic: no HIP, no library types.  The entry point and the
// test hook take ALL their launch and buffer sizes from here, and tests/marlin_agg_plan_main.cpp checks, for the counts at which a size
// changes its shape, that every lane a launch can touch lies inside its buffer -- so an access out of bounds on the device is ruled
// out by arithmetic before anything runs there.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zk {

constexpr size_t AGG_WAVE = 64;                    // lanes per block of every kernel here: one wave
constexpr size_t AGG_AFF_BYTES = 96;               // a G1 point in affine table form: 24 words
constexpr size_t AGG_XYZZ_BYTES = 192;             // an XYZZ partial: 48 words
constexpr size_t AGG_MAX_PASSES = 4;               // 2^22 lanes: 65 536 partials -> 1 024 -> 16

// One sum of `lanes` terms: a fold launch of `blocks` waves leaves one XYZZ partial per block in buffer A; pass p of the sum-down
// (groth16_verify.hip: zk_g1_sum_down) reads in[p] partials from A (p even) or B (p odd) and writes out[p] = ceil(in[p] / 64) into the
// other, until at most 64 are left -- `left` of them, in A if `passes` is even, else in B.
struct ZkSumPlan {
    size_t lanes, blocks;
    size_t part_a, part_b;                         // points of room in A and B: m and m / 64 + 1 for m = blocks
    size_t passes, in[AGG_MAX_PASSES], out[AGG_MAX_PASSES];
    size_t left;
};
inline size_t zk_plan_blocks(size_t n) { return (n + AGG_WAVE - 1) / AGG_WAVE; }
inline ZkSumPlan zk_sum_plan(size_t lanes) {
    ZkSumPlan s = {};
    s.lanes = lanes;
    s.blocks = zk_plan_blocks(lanes);
    s.part_a = s.blocks;
    s.part_b = s.blocks / AGG_WAVE + 1;
    size_t m = s.blocks;
    while (m > AGG_WAVE && s.passes < AGG_MAX_PASSES) {
        s.in[s.passes] = m;
        m = zk_plan_blocks(m);
        s.out[s.passes++] = m;
    }
    s.left = m;
    return s;
}

// The batch of `count` proofs.  Lane = point in ONE buffer of 13 count + 16 affine points:
//   [0, 11 count)              proof k's eleven commitment points, 11 k + i          (i < 11: ProofPoint order)
//   [11 count, 13 count)       its two opening witnesses, 11 count + 2 k + q          (q = 0: at beta, 1: at gamma)
//   [13 count, 13 count + 16)  the key's sixteen
// so the witnesses of the whole batch are adjacent and coefficient 2 k + q of the second sum meets its point with no copy.
constexpr size_t AGG_PROOF_POINTS = 13, AGG_COMM_POINTS = 11, AGG_KEY_POINTS = 16;
constexpr size_t AGG_MAX_COUNT = (size_t)1 << 18;  // 13 count + 16 lanes below 2^22, the lane limit of the sum kernels
struct ZkMarlinAggPlan {
    size_t count;
    size_t proof_lanes, wit_first, key_first;      // 13 count; 11 count; 13 count
    ZkSumPlan term, wit;                           // the long sum over 13 count + 16 lanes; the witnesses' over 2 count
    size_t comp_bytes;                             // the compressed proof points: 48 bytes each
    size_t pts_bytes;                              // the point buffer: 96 bytes per lane of the long sum
    size_t words_bytes;                            // the scalars of the long sum: 8 words per lane
    size_t coef_bytes;                             // the 128-bit coefficients: 4 words per witness
    size_t flags_bytes;                            // one word: any point off the curve or outside the subgroup
    size_t lane_of(size_t k, size_t i) const { return i < AGG_COMM_POINTS ? AGG_COMM_POINTS * k + i : wit_first + 2 * k + (i - AGG_COMM_POINTS); }
    size_t key_lane(size_t j) const { return key_first + j; }
};
inline ZkMarlinAggPlan zk_marlin_agg_plan(size_t count) {
    ZkMarlinAggPlan p = {};
    p.count = count;
    p.proof_lanes = AGG_PROOF_POINTS * count;
    p.wit_first = AGG_COMM_POINTS * count;
    p.key_first = p.proof_lanes;
    p.term = zk_sum_plan(p.proof_lanes + AGG_KEY_POINTS);
    p.wit = zk_sum_plan(2 * count);
    p.comp_bytes = p.proof_lanes * 48;
    p.pts_bytes = p.term.lanes * AGG_AFF_BYTES;
    p.words_bytes = p.term.lanes * 32;
    p.coef_bytes = p.wit.lanes * 16;
    p.flags_bytes = 4;
    return p;
}

}  // namespace zk
