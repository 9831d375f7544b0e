// Drives zk-mpc_amd/csrc/verify_keys_plan.hpp alone (tests/test_verify_keys_plan.py builds it with g++, once under the address and
// undefined-behaviour sanitizers): the grouping of a batch by key, and a replay of every lane of every level of the keyed sum with
// integers for points -- the kernel's own lane function (keyed_lane), its tree step for step, buffers of exactly the plan's sizes --
// and the identity plan of one key without a key_of array against the plan of an all-zero key_of.
#include "verify_keys_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <numeric>

using namespace zkvk;

#define CHECK(c)                                                             \
    do {                                                                     \
        if (!(c)) {                                                          \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #c);       \
            std::exit(1);                                                    \
        }                                                                    \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 7;
    rng_state ^= rng_state << 17;
    return rng_state;
}

// one level as the kernel runs it: in[g] -> out[piece], tags[piece]; every LDS read checked against the lane's own piece
static void replay_level(const Level& lv, const std::vector<uint64_t>& in, std::vector<uint64_t>* out, std::vector<uint32_t>* tag) {
    const uint32_t n_seg = (uint32_t)lv.seg_off.size() - 1;
    CHECK(lv.mis.size() == lv.seg_off.size() && lv.seg_off[0] == 0 && lv.seg_off[n_seg] == lv.n && in.size() == lv.n);
    out->assign(lv.n_out, 0);
    tag->assign(lv.n_out, NO_SLOT);
    std::vector<int> written(lv.n_out, 0);
    for (uint32_t wave0 = 0; wave0 < lv.n; wave0 += WAVE) {
        uint64_t lds[WAVE];
        KeyedLane kl[WAVE];
        for (uint32_t lane = 0; lane < WAVE; lane++) {
            const uint32_t g = wave0 + lane;
            kl[lane] = KeyedLane{n_seg, g, g + 1, 0};
            lds[lane] = 0;
            if (g < lv.n) {
                kl[lane] = keyed_lane(lv.seg_off.data(), lv.mis.data(), n_seg, g);
                lds[lane] = in[g];
                CHECK(kl[lane].slot < n_seg && lv.seg_off[kl[lane].slot] <= g && g < lv.seg_off[kl[lane].slot + 1]);
                CHECK(kl[lane].lo <= g && g < kl[lane].hi && kl[lane].lo >= wave0 && kl[lane].hi <= wave0 + WAVE && kl[lane].hi <= lv.n);
            }
        }
        for (uint32_t s = 1; s < WAVE; s <<= 1) {
            uint64_t next[WAVE];
            for (uint32_t lane = 0; lane < WAVE; lane++) {
                const uint32_t g = wave0 + lane;
                next[lane] = lds[lane];
                const bool act = (((g - kl[lane].lo) & (2 * s - 1)) == 0) && g + s < kl[lane].hi;
                if (!act) continue;
                CHECK(lane + s < WAVE && kl[lane + s].slot == kl[lane].slot && g + s < lv.n);      // never across a boundary
                next[lane] = lds[lane] + lds[lane + s];
            }
            for (uint32_t lane = 0; lane < WAVE; lane++) lds[lane] = next[lane];
        }
        for (uint32_t lane = 0; lane < WAVE; lane++) {
            const uint32_t g = wave0 + lane;
            if (g >= lv.n || g != kl[lane].lo) continue;
            CHECK(kl[lane].out < lv.n_out);
            CHECK(!written[kl[lane].out]++);
            (*out)[kl[lane].out] = lds[lane];
            (*tag)[kl[lane].out] = kl[lane].slot;
        }
    }
    for (uint32_t i = 0; i < lv.n_out; i++) CHECK(written[i] == 1);
    for (uint32_t i = 1; i < lv.n_out; i++) CHECK((*tag)[i - 1] <= (*tag)[i]);      // partials stay in key order
}

static void check_batch(size_t n_keys, const std::vector<uint32_t>& key_of, const std::vector<size_t>& ninp, size_t want_levels) {
    const size_t count = key_of.size();
    size_t total = 0;
    for (uint32_t k : key_of) total += ninp[k];
    Plan p;
    size_t bad = 0;
    CHECK(make_plan(n_keys, count, key_of.data(), ninp.data(), total, &p, &bad) == PLAN_OK);
    const size_t K = p.slots();
    // the used keys ascend; an unused key has no slot
    std::vector<uint32_t> per_key(n_keys, 0);
    for (uint32_t k : key_of) per_key[k]++;
    size_t used = 0, terms = 0;
    for (size_t k = 0; k < n_keys; k++) {
        if (!per_key[k]) { CHECK(p.slot_of_key[k] == NO_SLOT); continue; }
        CHECK(p.slot_of_key[k] == used && p.used[used] == k);
        CHECK(p.seg_off[used + 1] - p.seg_off[used] == per_key[k]);
        CHECK(p.gin_off[used + 1] - p.gin_off[used] == per_key[k] * ninp[k]);
        terms += ninp[k] + 2;
        used++;
    }
    CHECK(used == K && p.seg_off[0] == 0 && p.seg_off[K] == count && p.gin_off[K] == total && p.mul_terms == terms);
    CHECK(p.fold_lanes() == count + 3 * K && p.batch_lanes() == 3 * count);
    // the permutation: a bijection, grouped by key, stable, and pos its inverse
    std::vector<int> seen(count, 0);
    for (size_t g = 0; g < count; g++) {
        CHECK(p.perm[g] < count && !seen[p.perm[g]]++ && p.pos[p.perm[g]] == g);
        const uint32_t s = keyed_slot_of(p.seg_off.data(), (uint32_t)K, (uint32_t)g);
        CHECK(p.used[s] == key_of[p.perm[g]]);
        if (g && keyed_slot_of(p.seg_off.data(), (uint32_t)K, (uint32_t)g - 1) == s) CHECK(p.perm[g - 1] < p.perm[g]);
    }
    // input offsets in the caller's order
    CHECK(p.in_off.size() == count + 1 && p.in_off[0] == 0 && p.in_off[count] == total);
    for (size_t i = 0; i < count; i++) CHECK(p.in_off[i + 1] - p.in_off[i] == ninp[key_of[i]]);
    // the levels with integers for points: value of proof i = a random word, coefficient folded in
    std::vector<uint64_t> val(count), direct(K, 0), cur(count), out;
    std::vector<uint32_t> tag;
    for (size_t i = 0; i < count; i++) val[i] = rnd();
    for (size_t g = 0; g < count; g++) {
        cur[g] = val[p.perm[g]];
        direct[p.slot_of_key[key_of[p.perm[g]]]] += cur[g];
    }
    CHECK(!p.levels.empty() && p.levels[0].n == count && p.levels[0].seg_off == p.seg_off);
    CHECK(want_levels == 0 || p.levels.size() == want_levels);
    size_t meta = 0;
    for (size_t l = 0; l < p.levels.size(); l++) {
        const Level& lv = p.levels[l];
        CHECK(lv.n_out <= ((l & 1) ? p.part_b : p.part_a));
        meta += lv.seg_off.size() + lv.mis.size();
        replay_level(lv, cur, &out, &tag);
        const std::vector<uint32_t>& nxt = l + 1 < p.levels.size() ? p.levels[l + 1].seg_off : p.fin_off;
        CHECK(nxt.size() == K + 1 && nxt[0] == 0 && nxt[K] == lv.n_out);
        for (size_t s = 0; s < K; s++) {
            CHECK(nxt[s] < nxt[s + 1]);
            for (uint32_t i = nxt[s]; i < nxt[s + 1]; i++) CHECK(tag[i] == s);
        }
        cur = out;
    }
    CHECK(meta == p.meta_words);
    for (size_t s = 0; s < K; s++) {
        CHECK(p.fin_off[s + 1] - p.fin_off[s] <= WAVE);
        uint64_t sum = 0;
        for (uint32_t i = p.fin_off[s]; i < p.fin_off[s + 1]; i++) sum += cur[i];
        CHECK(sum == direct[s]);
    }
}

static bool same_level(const Level& a, const Level& b) { return a.n == b.n && a.n_out == b.n_out && a.seg_off == b.seg_off && a.mis == b.mis; }

// the identity plan (key_of = NULL: what the single-key entry points build) against make_plan on an all-zero key_of, under n_keys
// listed keys: every field but perm and pos, which it does not materialise and proof_at stands in for
static void check_identity(size_t n_keys, size_t count, const std::vector<size_t>& ninp) {
    const std::vector<uint32_t> zeros(count, 0);
    Plan a, b;
    size_t bad = 0;
    CHECK(make_plan(n_keys, count, zeros.data(), ninp.data(), count * ninp[0], &a, &bad) == PLAN_OK);
    CHECK(make_plan(n_keys, count, nullptr, ninp.data(), count * ninp[0], &b, &bad) == PLAN_OK);
    CHECK(!a.identity() && b.identity() && b.perm.empty() && b.pos.empty() && b.slots() == 1);
    for (size_t g = 0; g < count; g++) CHECK(a.proof_at(g) == g && b.proof_at(g) == g && a.pos[g] == g);
    CHECK(a.n_keys == b.n_keys && a.count == b.count && a.used == b.used && a.slot_of_key == b.slot_of_key && a.seg_off == b.seg_off);
    CHECK(a.in_off == b.in_off && a.gin_off == b.gin_off && a.mul_terms == b.mul_terms && a.fin_off == b.fin_off);
    CHECK(a.part_a == b.part_a && a.part_b == b.part_b && a.meta_words == b.meta_words && a.levels.size() == b.levels.size());
    for (size_t l = 0; l < a.levels.size(); l++) CHECK(same_level(a.levels[l], b.levels[l]));
    CHECK(a.fold_lanes() == b.fold_lanes() && a.batch_lanes() == b.batch_lanes());
    // the refusals that do not read key_of
    CHECK(make_plan(n_keys, count, nullptr, ninp.data(), count * ninp[0] + 1, &b, &bad) == PLAN_INPUTS_LEN && bad == count * ninp[0]);
    CHECK(make_plan(n_keys, 0, nullptr, ninp.data(), 0, &b, &bad) == PLAN_EMPTY);
}

static std::vector<uint32_t> runs_to_keys(const std::vector<uint32_t>& runs, int order) {
    std::vector<uint32_t> g;
    for (size_t k = 0; k < runs.size(); k++)
        for (uint32_t i = 0; i < runs[k]; i++) g.push_back((uint32_t)k);
    if (order == 1) return std::vector<uint32_t>(g.rbegin(), g.rend());
    if (order == 2) {
        std::vector<uint32_t> left = runs, out;
        while (out.size() < g.size())
            for (size_t k = 0; k < left.size(); k++)
                if (left[k]) { left[k]--; out.push_back((uint32_t)k); }
        return out;
    }
    return g;
}

int main() {
    const std::vector<size_t> ninp4 = {0, 1, 3, 3};
    for (int order = 0; order < 3; order++) {
        check_batch(4, runs_to_keys({63, 1, 64, 2}, order), ninp4, 1);
        check_batch(4, runs_to_keys({1, 1, 1, 1}, order), ninp4, 1);
        check_batch(4, runs_to_keys({65, 0, 64, 1}, order), ninp4, 1);
        check_batch(4, runs_to_keys({64, 64, 64, 64}, order), ninp4, 1);
        check_batch(4, runs_to_keys({4097, 1, 4095, 70}, order), ninp4, 2);      // 65 and 64 partials: a second level
        check_batch(3, runs_to_keys({0, 0, 5}, order), {7, 7, 2}, 1);
    }
    {   // more keys than lanes in a wave
        std::vector<uint32_t> runs(71, 1);
        runs[70] = 3;
        check_batch(71, runs_to_keys(runs, 0), std::vector<size_t>(71, 2), 1);
        check_batch(71, runs_to_keys(runs, 1), std::vector<size_t>(71, 2), 1);
    }
    check_batch(1, std::vector<uint32_t>(1, 0), {0}, 1);
    check_batch(1, std::vector<uint32_t>(64, 0), {2}, 1);
    check_batch(1, std::vector<uint32_t>(65, 0), {2}, 1);
    check_batch(1, std::vector<uint32_t>(4097, 0), {2}, 2);                      // 65 partials, as the single-key form's sum-down
    check_batch(1, std::vector<uint32_t>((size_t)1 << 18, 0), {1}, 2);
    check_batch(2, runs_to_keys({(1u << 18) + 1, (1u << 12) + 65}, 2), {1, 0}, 3);
    for (size_t count : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4096, (size_t)4097, (size_t)1 << 18, ((size_t)1 << 18) + 1})
        for (size_t n : {(size_t)0, (size_t)2}) {                                // one key without key_of: the identity plan
            check_identity(1, count, {n});
            check_identity(3, count, {n, 5, 1});
        }
    {
        Plan p;
        size_t bad = 0;
        const size_t big[1] = {MAX_INPUTS / 2 + 1};
        CHECK(make_plan(1, MAX_LANES + 1, nullptr, big, 0, &p, &bad) == PLAN_TOO_MANY);
        CHECK(make_plan(1, 2, nullptr, big, 2 * big[0], &p, &bad) == PLAN_TOO_MANY);
        CHECK(make_plan(1, 1, nullptr, big, big[0], &p, &bad) == PLAN_OK && p.identity() && p.in_off[1] == big[0]);
    }
    for (int t = 0; t < 200; t++) {                                              // random batches
        const size_t n_keys = 1 + rnd() % 9, count = 1 + rnd() % 700;
        std::vector<uint32_t> ko(count);
        std::vector<size_t> ninp(n_keys);
        for (auto& n : ninp) n = rnd() % 5;
        const uint64_t skew = 1 + rnd() % 3;
        for (auto& k : ko) {
            uint64_t v = rnd() % n_keys;
            for (uint64_t i = 1; i < skew; i++) v = v * (rnd() % n_keys) / n_keys;
            k = (uint32_t)v;
        }
        check_batch(n_keys, ko, ninp, 0);
    }
    {   // the launches depend on the longest segment alone: 300 keys of 13 proofs need the one level that one key of 13 needs
        std::vector<uint32_t> runs(300, 13);
        Plan p;
        size_t bad = 0;
        const std::vector<uint32_t> ko = runs_to_keys(runs, 2);
        const std::vector<size_t> ninp(300, 2);
        CHECK(make_plan(300, ko.size(), ko.data(), ninp.data(), 2 * ko.size(), &p, &bad) == PLAN_OK && p.levels.size() == 1);
        check_batch(300, ko, ninp, 1);
    }
    {   // every refusal
        Plan p;
        size_t bad = 99;
        const uint32_t ko[3] = {1, 0, 2};
        const size_t ninp[3] = {2, 0, 5};
        CHECK(make_plan(0, 3, ko, ninp, 7, &p, &bad) == PLAN_EMPTY);
        CHECK(make_plan(3, 0, ko, ninp, 7, &p, &bad) == PLAN_EMPTY);
        CHECK(make_plan(3, 3, ko, ninp, 7, &p, &bad) == PLAN_OK);
        CHECK(make_plan(2, 3, ko, ninp, 7, &p, &bad) == PLAN_KEY_OF && bad == 2);
        CHECK(make_plan(3, 3, ko, ninp, 6, &p, &bad) == PLAN_INPUTS_LEN && bad == 7);
        CHECK(make_plan(3, 3, ko, ninp, 8, &p, &bad) == PLAN_INPUTS_LEN && bad == 7);
        const size_t huge[3] = {2, MAX_INPUTS + 1, 5};
        CHECK(make_plan(3, 3, ko, huge, 7, &p, &bad) == PLAN_TOO_MANY);
        std::vector<uint32_t> many(MAX_LANES + 1, 0);
        const size_t none[1] = {0};
        CHECK(make_plan(1, many.size(), many.data(), none, 0, &p, &bad) == PLAN_TOO_MANY);
        many.resize(MAX_LANES - 3);                                              // count + 3 K' = 2^22: the last batch that fits
        CHECK(make_plan(1, many.size(), many.data(), none, 0, &p, &bad) == PLAN_OK && p.fold_fits() && !p.batch_fits());
        many.resize(MAX_LANES - 2);
        CHECK(make_plan(1, many.size(), many.data(), none, 0, &p, &bad) == PLAN_OK && !p.fold_fits());
        many.assign(MAX_LANES / 3, 0);
        CHECK(make_plan(1, many.size(), many.data(), none, 0, &p, &bad) == PLAN_OK && p.batch_fits());
        many.assign(MAX_LANES / 3 + 1, 0);
        CHECK(make_plan(1, many.size(), many.data(), none, 0, &p, &bad) == PLAN_OK && !p.batch_fits());
    }
    std::printf("ok\n");
    return 0;
}
