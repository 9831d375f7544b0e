// msm_spec.hpp -- what a context has LEARNED about the order of a caller's host-slice MSM calls, and what to start ahead from it.
// Pure host logic over opaque table keys and integers: no HIP, no context (msm_host.hip owns the jobs, the streams and the scalar
// copy; tests/msm_spec_policy_main.cpp drives this file alone).  A table is never dereferenced: what the policy has to know about
// one -- whether n scalars fit it -- the caller answers through `fits(table, n)`.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <iterator>
#include <map>

struct zk_bases;

class ZkMsmSpecPolicy {
public:
    using Table = const zk_bases*;
    struct AfterFft { Table table; size_t n; };

    // Which calls take part: speculation on, ONE scalar vector, a table that outlives the call, a fingerprint to know the vector by.
    static bool eligible(bool speculation_on, int lanes, bool temporary_table, uint64_t fp) {
        return speculation_on && lanes == 1 && !temporary_table && fp != 0;
    }

    // A call over `t` with n scalars of fingerprint fp.  The transform record is consumed whatever the call is; an eligible call that
    // brings the transform's output (all N elements or N - 1: the min(len) rule) teaches "transform -> table".  An eligible call
    // that follows an eligible call over ANOTHER table with the same (n, fp) teaches "table -> table"; any other call ends the chain.
    void observe(Table t, size_t n, uint64_t fp, bool is_eligible) {
        if (fft_N) {
            if (is_eligible && (n == fft_N || n + 1 == fft_N) && fp == fft_fp[n == fft_N ? 0 : 1]) {
                const size_t key = fft_key(fft_N, fft_kind);
                auto it = after_fft.find(key);
                if (it != after_fft.end() && it->second.table == t && it->second.n == n) earn_back(t);
                after_fft[key] = AfterFft{t, n};
            }
            fft_N = 0;
        }
        if (!is_eligible) { last_table = nullptr; return; }
        if (last_table && last_table != t && last_n == n && last_fp == fp) {
            auto it = succ.find(last_table);
            if (it != succ.end() && it->second == t) earn_back(t);
            succ[last_table] = t;
        }
        last_table = t; last_n = n; last_fp = fp;
    }

    // The tables to start after a call over `t` with n scalars: its successor and that one's, each with fewer than two wrong guesses
    // and long enough; none if the first does not qualify.  Returns how many of out[2] are set.
    template <class Fits>
    int next(Table t, size_t n, Fits&& fits, Table out[2]) const {
        auto follower = [&](Table from) -> Table {
            auto it = succ.find(from);
            if (it == succ.end() || it->second == t || it->second == from) return nullptr;
            return wrong_guesses(it->second) < 2 && fits(it->second, n) ? it->second : nullptr;
        };
        int cnt = 0;
        if (Table a = follower(t)) {
            out[cnt++] = a;
            if (Table b = follower(a)) out[cnt++] = b;
        }
        return cnt;
    }

    // Jobs were in flight and the call did not take the front one (over `front`): a wrong guess for that table -- unless an ineligible
    // call named the very table, which says nothing about the guess.  Two in a row give a table up (next, after_transform); the
    // count stops at 3.
    void wrong_guess(Table front, Table called, bool is_eligible) {
        if (!is_eligible && called == front) return;
        int& w = wrong[front];
        if (w < 3) w++;
    }
    void right_guess(Table t) { wrong.erase(t); }
    int wrong_guesses(Table t) const {
        auto it = wrong.find(t);
        return it == wrong.end() ? 0 : it->second;
    }

    // A host-slice transform of N elements (kind = inverse * 2 + coset) has delivered its output, whose fingerprints as a scalar vector
    // of N and of N - 1 elements are fp_N and fp_N1: the next table call is measured against it (observe), once.
    void transform_done(size_t N, int kind, uint64_t fp_N, uint64_t fp_N1) {
        fft_N = N; fft_kind = kind; fft_fp[0] = fp_N; fft_fp[1] = fp_N1;
    }
    // The MSM that took such a transform's output last time, if it is worth starting again: NULL otherwise.
    template <class Fits>
    const AfterFft* after_transform(size_t N, int kind, Fits&& fits) const {
        auto it = after_fft.find(fft_key(N, kind));
        if (it == after_fft.end()) return nullptr;
        const AfterFft& a = it->second;
        return wrong_guesses(a.table) < 2 && fits(a.table, a.n) && a.n <= N ? &a : nullptr;
    }

    // `t` leaves the cache or changes content: nothing learned may name it any more
    void forget(Table t) {
        if (last_table == t) last_table = nullptr;
        succ.erase(t);
        wrong.erase(t);
        for (auto it = succ.begin(); it != succ.end();) it = it->second == t ? succ.erase(it) : std::next(it);
        for (auto it = after_fft.begin(); it != after_fft.end();) it = it->second.table == t ? after_fft.erase(it) : std::next(it);
    }
    // speculation switched off: everything learned goes
    void clear() { succ.clear(); wrong.clear(); after_fft.clear(); fft_N = 0; last_table = nullptr; }

private:
    static size_t fft_key(size_t N, int kind) { return N * 4 + (size_t)kind; }
    // something learned was seen to hold again: a table given up after two wrong guesses in a row earns its way back, one
    // confirmation at a time
    void earn_back(Table t) {
        auto it = wrong.find(t);
        if (it != wrong.end() && it->second > 0 && --it->second == 0) wrong.erase(it);
    }

    Table last_table = nullptr;                    // the call before, if it was eligible
    uint64_t last_fp = 0;
    size_t last_n = 0;
    std::map<Table, Table> succ;                   // table -> the table asked for next with the same scalars
    std::map<Table, int> wrong;                    // wrong guesses in a row (0 .. 3) of a job started over the table
    // the transform a caller ran last on a host vector: its size and kind, the fingerprints of its output, and -- learned -- which table
    // was asked for with exactly that output as scalars: `h = witness_map(..)` and then multi_scalar_mul(&pk.h_query, &h)
    // (src/groth16.rs:100-106)
    size_t fft_N = 0;
    int fft_kind = 0;
    uint64_t fft_fp[2] = {0, 0};
    std::map<size_t, AfterFft> after_fft;
};
