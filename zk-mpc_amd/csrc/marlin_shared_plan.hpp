// marlin_shared_plan.hpp -- what the parties of zk_marlin_prove_shared[_spdz]_batch must agree on before any of them touches its device, as
// pure functions: no HIP, no context, no transport (tests/marlin_shared_plan_main.cpp runs them on the host under sanitizers).
//
//   * The chunk.  Each party computes how many proofs its device holds at once (its bound; 0: not even one), publishes the 8 bytes, and
//     all take the minimum: the exchanges of a chunk carry C items per kind, so parties with different chunks would wait for each other
//     in exchanges of different sizes.  A minimum of 0 fails every party alike.
//   * The items of the four small opens of a chunk of C proofs.  An open carries, per lane, scalars then G1 points (sharednet.hpp: fr | g1
//     at 4 / 18 words per item); within a kind the items are ordered by proof, and within a proof as listed here.  Lane 0 (the shares)
//     travels in the open itself, lane 1 (the MAC shares, SPDZ) enters the MAC exchange behind it at the same slot.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zk {
namespace marlin_plan {

// ---- the chunk ----
// The bound every party proceeds with: the minimum of the parties' bounds.  0: some party cannot hold one proof -- ZK_ERR_NOMEM for all.
inline uint64_t agreed_bound(const uint64_t* bounds, size_t parties) {
    uint64_t m = parties ? bounds[0] : 0;
    for (size_t p = 1; p < parties; p++) if (bounds[p] < m) m = bounds[p];
    return m;
}
// count proofs in chunks of at most cap (>= 1): chunk i holds the proofs [first, first + size), the last one what is left
inline size_t chunks_of(size_t count, size_t cap) { return cap ? (count + cap - 1) / cap : 0; }
struct Span { size_t first, size; };
inline Span chunk_at(size_t count, size_t cap, size_t i) {
    const size_t first = i * cap;
    if (!cap || first >= count) return Span{count, 0};
    return Span{first, count - first < cap ? count - first : cap};
}
// the exchanges of a call: the plan's one, then every chunk makes those of a single proof
inline size_t exchanges(size_t count, size_t cap, size_t single) { return 1 + chunks_of(count, cap) * single; }

// ---- the small opens ----
enum Open : int { OPEN_ROUND1, OPEN_ROUND2, OPEN_EVALS, OPEN_WITNESS, N_OPENS };
enum Kind : int { KIND_FR, KIND_G1, N_KINDS };
// the items of one proof, in wire order
enum Round1Item : int { R1_W, R1_Z_A, R1_Z_B, R1_MASK_POLY, R1_ITEMS };             // G1: the commitments of round 1
enum Round2Item : int { R2_G_1, R2_G_1_SHIFTED, R2_H_1, R2_ITEMS };                 // G1: the commitments of round 2 that depend on the witness (t is public)
enum EvalItem : int { EV_Z_B_BETA, EV_G_1_BETA, EV_ITEMS };                         // scalars
enum WitnessItem : int { WI_WITNESS_BETA = 0, WI_RANDOM_V = 0, WI_ITEMS = 1 };      // G1: the opening witness at beta; scalar: random_v
inline size_t per_proof(Open o, Kind k) {
    switch (o) {
        case OPEN_ROUND1: return k == KIND_G1 ? R1_ITEMS : 0;
        case OPEN_ROUND2: return k == KIND_G1 ? R2_ITEMS : 0;
        case OPEN_EVALS: return k == KIND_FR ? EV_ITEMS : 0;
        case OPEN_WITNESS: return WI_ITEMS;
        default: return 0;
    }
}
// where item `item` of proof k (counted within the chunk) stands among the open's items of its kind
inline size_t slot(Open o, Kind k, size_t proof, size_t item) { return proof * per_proof(o, k) + item; }
// ... and the 64-bit word of a party's message at which it starts, for a chunk of C proofs: scalars first, then points
inline size_t wire_word(Open o, Kind k, size_t C, size_t proof, size_t item) {
    const size_t at = slot(o, k, proof, item);
    return k == KIND_FR ? 4 * at : 4 * C * per_proof(o, KIND_FR) + 18 * at;
}
// Which message of the open carries lane l's item, and where: lane 0 (the share) travels in the open's own exchange, lane 1 (the MAC
// share, SPDZ) enters the MAC exchange right behind it -- as [leader ? opened : 0] - MAC share -- at the same word
struct Place { int exchange; size_t word; };      // exchange: 0 = the open, 1 = its MAC exchange
inline Place place(Open o, Kind k, size_t C, size_t proof, size_t item, int lane) { return Place{lane, wire_word(o, k, C, proof, item)}; }
inline size_t wire_words(Open o, size_t C) { return C * (4 * per_proof(o, KIND_FR) + 18 * per_proof(o, KIND_G1)); }

}  // namespace marlin_plan
}  // namespace zk
