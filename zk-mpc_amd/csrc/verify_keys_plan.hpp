// verify_keys_plan.hpp -- every index of Groth16 verification over SEVERAL keys in one call (groth16_verify_keys.hip): which proofs
// belong to which key, where a key's proofs and inputs lie once they are grouped, how many lanes the forms take, and the levels of
// the keyed sum (k_g1_scale_fold_keyed) with the place of every partial it writes.  Pure C++, no HIP: the device form, the host
// form and tests/verify_keys_plan_main.cpp read the plan; none of them derives any of it again.
//
// A batch: n_keys keys, count proofs, key_of[i] < n_keys the key of proof i (any order), the public inputs concatenated in proof
// order -- proof i contributes ninp[key_of[i]] elements.  GROUPED order is the stable sort of the proofs by key: position g holds
// proof perm[g], and the proofs of one key keep the caller's order.  A key with at least one proof is USED and gets a SLOT (slots
// ascend with the key's index); slot s owns the grouped positions seg_off[s] .. seg_off[s + 1] - 1.
//
// The keyed sum.  One term per lane in grouped order, one wave of 64 lanes per block.  A wave holds a PIECE of every slot whose
// segment meets it, sums each piece by a segmented tree and writes one partial per piece, in slot order.  Piece p of the launch is
// therefore at index
//     wave + mis[slot of the wave's first lane] + (slot - slot of the wave's first lane)
// where mis[s] counts the boundaries seg_off[1 .. s] that are no multiple of 64 (a boundary at a wave's edge cuts no wave in two).
// The partials of a level are the lanes of the next one, with their own seg_off; the levels end once no slot has more than 64
// partials, which the host adds.  The number of levels depends on the longest segment alone -- never on the number of keys.
//
// ONE key is the plan with one slot and the identity permutation: key_of = NULL puts every proof under key 0, and that plan does
// not materialise perm and pos (Plan::identity; Plan::proof_at reads either kind).  The single-key entry points plan so.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define ZKVK_HD __host__ __device__ __forceinline__
#else
#define ZKVK_HD inline
#endif

namespace zkvk {

constexpr size_t MAX_LANES = (size_t)1 << 22;      // one Miller launch (pairing.hip: ZK_PAIRING_MAX_LANES)
constexpr size_t MAX_INPUTS = (size_t)1 << 30;     // public inputs in one call (groth16_verify.hip: inputs_ok)
constexpr uint32_t WAVE = 64;
constexpr uint32_t NO_SLOT = 0xFFFFFFFFu;

// What lane g < n of a level does, written once for the kernel and for the host's replay of it.  seg_off: n_seg + 1 ascending
// offsets, seg_off[0] = 0, seg_off[n_seg] = n, no empty segment; mis as above.
struct KeyedLane {
    uint32_t slot;         // the segment of lane g
    uint32_t lo, hi;       // its piece: the lanes of this wave that belong to the segment, [lo, hi)
    uint32_t out;          // where the piece's partial goes (written by lane lo)
};
ZKVK_HD uint32_t keyed_slot_of(const uint32_t* seg_off, uint32_t n_seg, uint32_t g) {      // the last s with seg_off[s] <= g
    uint32_t lo = 0, hi = n_seg;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (seg_off[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}
ZKVK_HD KeyedLane keyed_lane(const uint32_t* seg_off, const uint32_t* mis, uint32_t n_seg, uint32_t g) {
    const uint32_t wave0 = g & ~(WAVE - 1u), first = keyed_slot_of(seg_off, n_seg, wave0);
    KeyedLane l;
    l.slot = keyed_slot_of(seg_off, n_seg, g);
    l.lo = seg_off[l.slot] > wave0 ? seg_off[l.slot] : wave0;
    l.hi = seg_off[l.slot + 1] < wave0 + WAVE ? seg_off[l.slot + 1] : wave0 + WAVE;
    l.out = wave0 / WAVE + mis[first] + (l.slot - first);
    return l;
}

enum Refusal { PLAN_OK = 0, PLAN_EMPTY, PLAN_KEY_OF, PLAN_INPUTS_LEN, PLAN_TOO_MANY };

struct Level {
    uint32_t n = 0;                        // lanes: the proofs (level 0) or the partials of the level before
    uint32_t n_out = 0;                    // partials written
    std::vector<uint32_t> seg_off, mis;    // slots + 1 words each
};

struct Plan {
    size_t n_keys = 0, count = 0;
    std::vector<uint32_t> used;            // slot -> key
    std::vector<uint32_t> slot_of_key;     // key -> slot, NO_SLOT for a key without a proof
    std::vector<uint32_t> perm;            // grouped position -> proof (empty in the identity plan)
    std::vector<uint32_t> pos;             // proof -> grouped position (empty in the identity plan)
    std::vector<uint32_t> seg_off;         // slots + 1, in grouped positions
    std::vector<size_t> in_off;            // count + 1: proof i's inputs are elements in_off[i] .. in_off[i + 1] - 1 of the caller's array
    std::vector<size_t> gin_off;           // slots + 1: the same per slot in the GROUPED input array (a slot's inputs are contiguous there)
    size_t mul_terms = 0;                  // sum over the used keys of ninp + 2: the full-width multiplications of key points
    std::vector<Level> levels;             // the keyed sum; at least one (level 0 scales)
    std::vector<uint32_t> fin_off;         // slots + 1: the partials of slot s behind the last level, at most 64 each
    size_t part_a = 0, part_b = 0;         // partials the two alternating buffers hold at most (even / odd levels)
    size_t meta_words = 0;                 // seg_off | mis of every level back to back: level l at 2 l (slots + 1)

    size_t slots() const { return used.size(); }
    bool identity() const { return perm.empty(); }                  // key_of = NULL: grouped position g holds proof g
    size_t proof_at(size_t g) const { return perm.empty() ? g : perm[g]; }
    size_t fold_lanes() const { return count + 3 * slots(); }      // one Miller lane per proof, three per used key
    size_t batch_lanes() const { return 3 * count; }
    bool fold_fits() const { return fold_lanes() <= MAX_LANES; }
    bool batch_fits() const { return batch_lanes() <= MAX_LANES; }
};

// the level behind `seg_off` over n lanes: its mis, its partial count, and (next) the seg_off of its partials
inline Level make_level(const std::vector<uint32_t>& seg_off, std::vector<uint32_t>* next) {
    Level lv;
    const size_t k = seg_off.size() - 1;
    lv.n = seg_off[k];
    lv.seg_off = seg_off;
    lv.mis.assign(k + 1, 0);
    next->assign(k + 1, 0);
    for (size_t s = 0; s < k; s++) {
        const uint32_t b = seg_off[s], e = seg_off[s + 1];
        (*next)[s + 1] = (*next)[s] + ((e + WAVE - 1) / WAVE - b / WAVE);
        lv.mis[s + 1] = lv.mis[s] + (e % WAVE != 0 ? 1u : 0u);
    }
    lv.n_out = (*next)[k];
    return lv;
}

// The plan of a batch.  ninp[k]: the public inputs of key k.  key_of = NULL: every proof under key 0, the identity plan.  *bad: the
// first offending proof (PLAN_KEY_OF) or the length the inputs should have (PLAN_INPUTS_LEN).  PLAN_TOO_MANY: count above MAX_LANES or more than MAX_INPUTS inputs -- no form takes that.
inline Refusal make_plan(size_t n_keys, size_t count, const uint32_t* key_of, const size_t* ninp, size_t inputs_len, Plan* p, size_t* bad) {
    *p = Plan();
    if (!n_keys || !count) return PLAN_EMPTY;
    if (count > MAX_LANES) return PLAN_TOO_MANY;
    for (size_t i = 0; key_of && i < count; i++)
        if (key_of[i] >= n_keys) { *bad = i; return PLAN_KEY_OF; }
    p->n_keys = n_keys;
    p->count = count;
    std::vector<uint32_t> per_key(n_keys, 0);
    if (!key_of) per_key[0] = (uint32_t)count;
    for (size_t i = 0; key_of && i < count; i++) per_key[key_of[i]]++;
    p->slot_of_key.assign(n_keys, NO_SLOT);
    p->seg_off.push_back(0);
    p->gin_off.push_back(0);
    for (size_t k = 0; k < n_keys; k++) {
        if (!per_key[k]) continue;
        if (ninp[k] > MAX_INPUTS || (size_t)per_key[k] * ninp[k] > MAX_INPUTS - p->gin_off.back()) return PLAN_TOO_MANY;
        p->slot_of_key[k] = (uint32_t)p->used.size();
        p->used.push_back((uint32_t)k);
        p->seg_off.push_back(p->seg_off.back() + per_key[k]);
        p->gin_off.push_back(p->gin_off.back() + (size_t)per_key[k] * ninp[k]);
        p->mul_terms += ninp[k] + 2;
    }
    if (p->gin_off.back() != inputs_len) { *bad = p->gin_off.back(); return PLAN_INPUTS_LEN; }
    std::vector<uint32_t> next(p->seg_off.begin(), p->seg_off.end() - 1);      // the next free grouped position of every slot
    p->in_off.resize(count + 1);
    p->in_off[0] = 0;
    if (key_of) {
        p->perm.resize(count);
        p->pos.resize(count);
    }
    for (size_t i = 0; i < count; i++) {
        p->in_off[i + 1] = p->in_off[i] + ninp[key_of ? key_of[i] : 0];
        if (!key_of) continue;
        const uint32_t g = next[p->slot_of_key[key_of[i]]]++;
        p->perm[g] = (uint32_t)i;
        p->pos[i] = g;
    }
    std::vector<uint32_t> seg = p->seg_off, nxt;
    for (;;) {
        p->levels.push_back(make_level(seg, &nxt));
        size_t& room = (p->levels.size() & 1) ? p->part_a : p->part_b;
        if (p->levels.back().n_out > room) room = p->levels.back().n_out;
        uint32_t longest = 0;
        for (size_t s = 0; s + 1 < nxt.size(); s++)
            if (nxt[s + 1] - nxt[s] > longest) longest = nxt[s + 1] - nxt[s];
        seg = nxt;
        if (longest <= WAVE) break;
    }
    p->fin_off = seg;
    p->meta_words = p->levels.size() * 2 * (p->slots() + 1);
    return PLAN_OK;
}

}  // namespace zkvk
