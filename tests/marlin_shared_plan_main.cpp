// Drives zk-mpc_amd/csrc/marlin_shared_plan.hpp alone (tests/test_marlin_shared_plan.py builds it with g++ under the address and
// undefined-behaviour sanitizers): the rule by which the parties of a collaborative Marlin batch agree on their chunks, and the
// item layout of the chunk's small opens.
#include "marlin_shared_plan.hpp"
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

using namespace zk::marlin_plan;

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::printf("%s:%d: %s failed\n", __FILE__, __LINE__, #c);    \
            std::exit(1);                                                 \
        }                                                                 \
    } while (0)

static void the_bound_is_the_minimum_and_zero_means_no() {
    for (size_t parties : {(size_t)1, (size_t)2, (size_t)8}) {
        for (size_t low = 0; low < parties; low++) {              // the smallest bound at every position
            std::vector<uint64_t> b(parties);
            for (size_t p = 0; p < parties; p++) b[p] = 40 + 3 * p;
            b[low] = 7;
            CHECK(agreed_bound(b.data(), parties) == 7);
            b[low] = 0;                                           // one party cannot hold a proof: nobody proceeds
            CHECK(agreed_bound(b.data(), parties) == 0);
        }
        std::vector<uint64_t> same(parties, 64);
        CHECK(agreed_bound(same.data(), parties) == 64);
    }
    const uint64_t one = 5;
    CHECK(agreed_bound(&one, 1) == 5);                            // a single party: its own value
}

static void the_chunks_cover_every_proof_once() {
    for (size_t count : {(size_t)1, (size_t)2, (size_t)5, (size_t)64, (size_t)65})
        for (size_t cap : {(size_t)1, (size_t)2, (size_t)64}) {
            const size_t chunks = chunks_of(count, cap);
            CHECK(chunks == (count + cap - 1) / cap);
            std::vector<int> seen(count, 0);
            size_t next = 0;
            for (size_t i = 0; i < chunks; i++) {
                const Span sp = chunk_at(count, cap, i);
                CHECK(sp.first == next && sp.size >= 1 && sp.size <= cap);
                CHECK(i + 1 == chunks || sp.size == cap);         // only the last chunk may be short ...
                for (size_t k = 0; k < sp.size; k++) seen[sp.first + k]++;
                next = sp.first + sp.size;
            }
            CHECK(next == count);
            for (size_t k = 0; k < count; k++) CHECK(seen[k] == 1);
            const Span last = chunk_at(count, cap, chunks - 1);
            CHECK(last.size == (count % cap ? count % cap : cap));   // ... and it is what is left
            CHECK(chunk_at(count, cap, chunks).size == 0);
            CHECK(exchanges(count, cap, 8) == 1 + chunks * 8);
        }
    CHECK(chunk_at(65, 64, 1).first == 64 && chunk_at(65, 64, 1).size == 1);
    CHECK(chunk_at(5, 2, 2).first == 4 && chunk_at(5, 2, 2).size == 1);
    CHECK(chunks_of(5, 0) == 0 && chunk_at(5, 0, 0).size == 0);
}

// Every (proof, item, lane) of an open has a slot of its own; within a kind the order is by proof, then as the header lists the items;
// the message is scalars then points, and nothing overlaps or leaves a gap
static void the_items_of_an_open_have_distinct_slots_ordered_by_proof() {
    for (int lanes = 1; lanes <= 2; lanes++)
        for (size_t C : {(size_t)1, (size_t)2, (size_t)5, (size_t)64})
            for (int o = 0; o < N_OPENS; o++) {
                const Open open = (Open)o;
                std::set<std::pair<int, size_t>> words;           // (exchange, first word) as place() gives them
                size_t covered = 0;
                for (int k = 0; k < N_KINDS; k++) {
                    const Kind kind = (Kind)k;
                    const size_t per = per_proof(open, kind), width = kind == KIND_FR ? 4 : 18;
                    size_t want = 0;
                    for (size_t proof = 0; proof < C; proof++)
                        for (size_t item = 0; item < per; item++) {
                            CHECK(slot(open, kind, proof, item) == want++);          // by proof within the kind
                            for (int lane = 0; lane < lanes; lane++) {
                                const Place at = place(open, kind, C, proof, item, lane);
                                CHECK(at.exchange == lane && at.word == wire_word(open, kind, C, proof, item));   // the MAC lane: the next exchange, the same word
                                CHECK(at.word + width <= wire_words(open, C));
                                CHECK(words.insert({at.exchange, at.word}).second);
                            }
                            covered += width;
                        }
                    CHECK(want == C * per);
                }
                CHECK(covered == wire_words(open, C) && words.size() == (size_t)lanes * C * (per_proof(open, KIND_FR) + per_proof(open, KIND_G1)));
                // the scalars come first: the last scalar ends where the first point begins
                if (per_proof(open, KIND_FR) && per_proof(open, KIND_G1))
                    CHECK(wire_word(open, KIND_FR, C, C - 1, per_proof(open, KIND_FR) - 1) + 4 == wire_word(open, KIND_G1, C, 0, 0));
            }
    CHECK(per_proof(OPEN_ROUND1, KIND_G1) == 4 && per_proof(OPEN_ROUND2, KIND_G1) == 3 && per_proof(OPEN_EVALS, KIND_FR) == 2);
    CHECK(per_proof(OPEN_WITNESS, KIND_G1) == 1 && per_proof(OPEN_WITNESS, KIND_FR) == 1);
    CHECK(slot(OPEN_ROUND1, KIND_G1, 3, R1_MASK_POLY) == 15 && slot(OPEN_ROUND2, KIND_G1, 2, R2_G_1_SHIFTED) == 7);
    CHECK(slot(OPEN_EVALS, KIND_FR, 4, EV_G_1_BETA) == 9 && wire_word(OPEN_WITNESS, KIND_G1, 5, 2, WI_WITNESS_BETA) == 4 * 5 + 18 * 2);
}

int main() {
    the_bound_is_the_minimum_and_zero_means_no();
    the_chunks_cover_every_proof_once();
    the_items_of_an_open_have_distinct_slots_ordered_by_proof();
    std::printf("ok\n");
    return 0;
}
