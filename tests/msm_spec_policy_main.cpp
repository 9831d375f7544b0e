// The learning rule of the MSMs started ahead (zk-mpc_amd/csrc/msm_spec.hpp) on fake table keys: a self-checking driver for
// tests/test_msm_spec_policy.py.  Prints "ok" and returns 0, or names the first expectation that failed.
#include "msm_spec.hpp"
#include <stdio.h>
#include <stdlib.h>
#include <map>
#include <vector>

using P = ZkMsmSpecPolicy;
using Table = P::Table;

static char keys[8];                                        // addresses only: a table is never dereferenced
static const Table A = (Table)&keys[0], B = (Table)&keys[1], C = (Table)&keys[2], D = (Table)&keys[3];
static std::map<Table, size_t> len;                         // table lengths, as the library would answer `fits`
static bool fits(Table t, size_t n) { return n <= len.at(t); }

static std::vector<Table> after(const P& p, Table t, size_t n) {
    Table out[2] = {nullptr, nullptr};
    const int cnt = p.next(t, n, fits, out);
    return std::vector<Table>(out, out + cnt);
}
using V = std::vector<Table>;

#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) { printf("%s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); }  \
    } while (0)

static const size_t N1 = 1000;
static const uint64_t FP = 0xABCDEF;

// one round A, B, C over (n, fp), all eligible
static void round_abc(P& p, size_t n = N1, uint64_t fp = FP) {
    p.observe(A, n, fp, true);
    p.observe(B, n, fp, true);
    p.observe(C, n, fp, true);
}

int main() {
    len = {{A, 4096}, {B, 4096}, {C, 4096}, {D, 4096}};
    CHECK(P::eligible(true, 1, false, FP));
    CHECK(!P::eligible(false, 1, false, FP) && !P::eligible(true, 2, false, FP) && !P::eligible(true, 1, true, FP) && !P::eligible(true, 1, false, 0));

    {   // (a) A, B, C over one (n, fp)
        P p;
        CHECK(after(p, A, N1).empty());
        round_abc(p);
        CHECK(after(p, A, N1) == (V{B, C}));
        CHECK(after(p, B, N1) == (V{C}));
        CHECK(after(p, C, N1).empty());
        // n has to fit every table that is started
        len[C] = N1 - 1;
        CHECK(after(p, A, N1) == (V{B}));
        len[C] = 4096; len[B] = N1 - 1;
        CHECK(after(p, A, N1).empty());                      // the first does not qualify: nothing
        len[B] = 4096;
    }
    {   // (b) A -> B and B -> A
        P p;
        p.observe(A, N1, FP, true);
        p.observe(B, N1, FP, true);
        p.observe(A, N1, FP, true);
        CHECK(after(p, A, N1) == (V{B}));
        CHECK(after(p, B, N1) == (V{A}));
    }
    {   // (c) wrong guesses, (d) earn-back, (e) a right guess
        P p;
        round_abc(p);
        p.wrong_guess(B, D, true);
        CHECK(p.wrong_guesses(B) == 1 && after(p, A, N1) == (V{B, C}));
        p.wrong_guess(B, D, false);                          // an ineligible call that names another table counts
        CHECK(p.wrong_guesses(B) == 2);
        CHECK(after(p, A, N1).empty());                      // although B -> C is known
        CHECK(after(p, B, N1) == (V{C}));
        p.wrong_guess(B, B, false);                          // an ineligible call over the very table does not
        CHECK(p.wrong_guesses(B) == 2);
        p.wrong_guess(B, B, true);                           // an eligible one does (other scalars)
        CHECK(p.wrong_guesses(B) == 3);
        p.wrong_guess(B, D, true);
        CHECK(p.wrong_guesses(B) == 3);                      // the ceiling
        CHECK(p.wrong_guesses(C) == 0);                      // only the front job's table is charged
        // (d) from 3: one confirmation of A -> B is not enough, two are
        p.observe(D, 7, 1, false);
        p.observe(A, N1, FP, true);
        p.observe(B, N1, FP, true);
        CHECK(p.wrong_guesses(B) == 2 && after(p, A, N1).empty());
        p.observe(A, N1 + 1, FP + 1, true);
        p.observe(B, N1 + 1, FP + 1, true);
        CHECK(p.wrong_guesses(B) == 1 && after(p, A, N1) == (V{B, C}));
        p.observe(A, N1, FP, true);
        p.observe(B, N1, FP, true);
        CHECK(p.wrong_guesses(B) == 0);
        p.observe(D, 7, 1, false);                           // (or B -> A would be learned here)
        p.observe(A, N1, FP, true);
        p.observe(B, N1, FP, true);
        CHECK(p.wrong_guesses(B) == 0);                      // erased at 0, never below
        // a NEW succession is no confirmation
        p.wrong_guess(C, D, true);
        p.wrong_guess(C, D, true);
        p.observe(D, 7, 1, false);
        p.observe(D, N1, FP, true);
        p.observe(C, N1, FP, true);                          // D -> C: first seen
        CHECK(p.wrong_guesses(C) == 2);
        // (e) a right guess erases in one step
        p.wrong_guess(C, D, true);
        CHECK(p.wrong_guesses(C) == 3);
        p.right_guess(C);
        CHECK(p.wrong_guesses(C) == 0 && after(p, A, N1) == (V{B, C}));
    }
    {   // (f) what does not teach
        P p;
        p.observe(A, N1, FP, true);
        p.observe(B, N1 + 1, FP, true);                      // another n
        CHECK(after(p, A, N1).empty());
        p.observe(C, N1 + 1, FP + 1, true);                  // another fp
        CHECK(after(p, B, N1).empty());
        p.observe(A, N1, FP, true);
        p.observe(A, N1, FP, true);                          // the same table
        CHECK(after(p, A, N1).empty());
        p.observe(D, N1, FP, false);                         // an ineligible call in between: "the call before" is cleared
        p.observe(B, N1, FP, true);
        CHECK(after(p, A, N1).empty() && after(p, D, N1).empty());
        p.observe(D, N1, 0, P::eligible(true, 1, false, 0)); // fp == 0 is such a call
        p.observe(C, N1, FP, true);
        CHECK(after(p, B, N1).empty() && after(p, D, N1).empty());
        p.observe(D, N1, FP, true);                          // ... and the chain goes on from there
        CHECK(after(p, C, N1) == (V{D}));
    }
    {   // (g) after a transform
        P p;
        const size_t N = 1024;
        const uint64_t fN = 11, fN1 = 22;
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(A, N, 99, true);                           // not the transform's output: consumed all the same
        p.observe(B, N, fN, true);
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(B, N, fN, false);                          // ineligible: consumed, nothing learned
        p.observe(B, N, fN, true);
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(B, N, fN1, true);                          // n == N goes with fp(N)
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(B, N - 1, fN, true);                       // n + 1 == N goes with fp(N - 1)
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(B, N - 2, fN1, true);                      // neither length
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(B, N - 1, fN1, true);
        const P::AfterFft* a = p.after_transform(N, 3, fits);
        CHECK(a && a->table == B && a->n == N - 1);
        CHECK(!p.after_transform(N, 2, fits) && !p.after_transform(2 * N, 3, fits));     // the kind and the size are part of the key
        p.transform_done(N, 3, fN, fN1);
        p.observe(C, N, fN, true);                           // the latest pair replaces the entry
        a = p.after_transform(N, 3, fits);
        CHECK(a && a->table == C && a->n == N);
        // lookup refuses: two wrong guesses, n longer than the table, n > N
        p.wrong_guess(C, D, true);
        CHECK(p.after_transform(N, 3, fits));
        p.wrong_guess(C, D, true);
        CHECK(!p.after_transform(N, 3, fits));
        p.transform_done(N, 3, fN, fN1);
        p.observe(C, N, fN, true);                           // the recorded pair seen again: earn-back
        CHECK(p.wrong_guesses(C) == 1 && p.after_transform(N, 3, fits));
        len[C] = N - 1;
        CHECK(!p.after_transform(N, 3, fits));
        len[C] = 4096;
        // n > N: no valid kind (0 .. 3) records such an entry; kind -4 puts one with n = 64 under the key of (63, 0)
        p.transform_done(64, -4, fN, fN1);
        p.observe(D, 64, fN, true);
        CHECK(!p.after_transform(63, 0, fits));
        p.transform_done(64, 0, fN, fN1);
        p.observe(D, 63, fN1, true);
        CHECK(p.after_transform(64, 0, fits));               // (n + 1 == N is fine)
    }
    {   // (h) forget(B)
        P p;
        round_abc(p);
        p.observe(D, N1, FP, true);                          // C -> D
        p.wrong_guess(B, D, true);
        p.wrong_guess(C, D, true);
        p.transform_done(64, 3, 5, 6);
        p.observe(B, 64, 5, true);
        p.transform_done(128, 3, 7, 8);
        p.observe(C, 128, 7, true);
        p.observe(B, N1, FP, true);                          // "the call before" is B
        p.forget(B);
        CHECK(after(p, C, N1) == (V{D}));                    // C -> D stays
        CHECK(after(p, A, N1).empty());                      // A -> B
        CHECK(after(p, B, N1).empty());                      // B -> C
        CHECK(p.wrong_guesses(B) == 0);
        CHECK(!p.after_transform(64, 3, fits));
        CHECK(p.wrong_guesses(C) == 1);                      // C's entries stay
        CHECK(p.after_transform(128, 3, fits) && p.after_transform(128, 3, fits)->table == C);
        p.observe(D, N1, FP, true);                          // the call before was B and is forgotten: no B -> D
        CHECK(after(p, B, N1).empty());
        p.observe(C, N1, FP, true);
        p.observe(D, N1, FP, true);
        CHECK(after(p, C, N1) == (V{D}));
    }
    {   // (i) off
        P p;
        round_abc(p);
        p.wrong_guess(B, D, true);
        p.transform_done(64, 3, 5, 6);
        p.observe(C, 64, 5, true);
        p.observe(A, N1, FP, true);
        p.transform_done(64, 3, 5, 6);
        p.clear();
        CHECK(after(p, A, N1).empty() && after(p, B, N1).empty());
        CHECK(p.wrong_guesses(B) == 0);
        CHECK(!p.after_transform(64, 3, fits));
        p.observe(B, N1, FP, true);                          // "the call before" (A) went too
        CHECK(after(p, A, N1).empty());
        p.observe(C, 64, 5, true);                           // and the pending transform record
        CHECK(!p.after_transform(64, 3, fits));
    }
    printf("ok\n");
    return 0;
}
