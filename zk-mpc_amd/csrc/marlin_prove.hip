// marlin_prove.hip -- Marlin::prove as ONE entry point: the three AHP rounds, MarlinKZG10 commitments, the Fiat-Shamir
// transcript, the evaluations and open_combinations, sequenced on the host in C++ over the library's own kernels.
//
// Replaces (reference):
//   Marlin::prove                                  arkworks/marlin/src/lib.rs:152-319
//   AHPForR1CS::prover_{init,first,second,third}_round   arkworks/marlin/src/ahp/prover.rs:216-716
//   AHPForR1CS::{verifier_*_round, verifier_query_set, construct_linear_combinations}   ahp/verifier.rs:42-170, ahp/mod.rs:112-290
//   MarlinKZG10::{commit, open}, Marlin::open_combinations   poly-commit/src/marlin/marlin_pc/mod.rs:172-340, marlin/mod.rs:213-306
//   FiatShamirRng / to_bytes! encodings            marlin/src/rng.rs, ff/src/bytes.rs, marlin_pc/data_structures.rs:252-263
// The same sequence exists as zk-mpc_amd/marlin.py::prove (kept: it is what the collaborative provers build on, and the two are
// tested against each other and against the oracle's independent prover byte for byte).  The index (Marlin::index: matrix
// arithmetisation, index commitments) is a one-off set-up and stays with the caller, who hands over device-resident tables.
//
// Layout: ORACLES states once what each oracle is; MsmJobs is the argument list of one zk_msm_batch_dev call; Marlin<LANES> is one proof in
// progress: its ProofState (marlin_prove_int.hpp) and its device pointers are what crosses the rounds, its methods are the steps that
// marlin_impl runs in order.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "hostgroup.hpp"
#include "internal.hpp"
#include "marlin_prove_int.hpp"
#include "sharednet.hpp"
#include <algorithm>
#include <chrono>
#include <future>
#include <string>
#include <vector>

using namespace zk;
using namespace zk::marlin;      // marlin_prove_int.hpp: the oracle table and the host halves every Marlin prover shares

namespace {

// One lane -- 0: the share lane (or the plain prover), 1: the MAC lane of a SPDZ prover, own scratch names: its polynomials, the device calls on them
struct Prover {
    zk_ctx* ctx;
    int lane = 0;
    int rc = ZK_OK;
    Poly polys[N_ORACLES];

    char* dev(const std::string& name, size_t elems) {
        void* p = nullptr;
        if (rc == ZK_OK) rc = zk_scratch(ctx, ((lane ? "mp1." : "mp.") + name).c_str(), std::max<size_t>(elems, 1) * 32, &p);
        return (char*)p;
    }
    void ck(int r) { if (rc == ZK_OK) rc = r; }
    void d2d(void* dst, const void* src, size_t elems) { if (elems) ck(zk_memcpy_d2d(ctx, dst, src, elems * 32)); }
    void zero(void* dst, size_t elems) { if (elems) ck(zk_dev_zero(ctx, dst, elems * 32)); }
    void op(int o, const void* a, const void* b, void* out, size_t n) { if (n) ck(zk_fr_vec_op_dev(ctx, o, a, b, out, n)); }
    void scale(const void* a, const HF& k, void* out, size_t n) { zk_fr kk = k.abi(); if (n) ck(zk_fr_vec_scale_dev(ctx, a, &kk, out, n)); }
    void ntt(void* buf, const Dom& d, int inverse) { ck(zk_fr_ntt_dev(ctx, buf, d.log, inverse, 0)); }
    // up to four transforms of one size and kind as one launch per pass (ntt.hip::zk_ntt_launch_batch)
    void ntt_batch(std::initializer_list<void*> bufs, const Dom& d, int inverse) {
        std::vector<void*> v(bufs);
        if (rc == ZK_OK) ck(zk_ntt_launch_batch(ctx, v.data(), (int)v.size(), d.log, inverse, 0));
    }
    char* padded(const Dom& d, const Poly& p, const std::string& name) {  // the zero-padded copy evaluate_over_domain transforms
        char* out = dev(name, d.size);
        if (rc != ZK_OK) return out;
        if (p.n < d.size) zero(out + 32 * p.n, d.size - p.n);
        d2d(out, p.p, std::min(p.n, d.size));
        return out;
    }
    char* fft(const Dom& d, const Poly& p, const std::string& name) {     // evaluate_over_domain: zero-pad, forward transform
        char* out = padded(d, p, name);
        ntt(out, d, 0);
        return out;
    }
    bool is_zero(const void* v, size_t n) { int z = 0; ck(zk_fr_vec_is_zero_dev(ctx, v, n, &z)); return z != 0; }
    // p + r (X^n - 1) for deg p < n: one more coefficient
    Poly blind(const char* poly, size_t n, const char* r_dev, const std::string& name) {
        char* out = dev(name, n + 1);
        d2d(out, poly, n);
        d2d(out + 32 * n, r_dev, 1);
        op(ZK_OP_SUB, out, r_dev, out, 1);
        return Poly{out, n + 1};
    }
};

// sum_i c_i G_i for the three powers_of_gamma_g a hiding bound of 1 uses: on the host (a three-term MSM through the device
// pipeline costs a full sort / accumulate / reduce round trip, ~0.5 ms; this is three scalar multiplications in 64-bit limbs), side
// by side on the context's helper threads (0.2 ms each: three in a row were longer than the device batch of a small proof's round
// they are meant to hide under)
zk_g1_projective small_msm_par(zk_ctx* ctx, const zk_g1_projective* pts, const std::vector<HF>& c) {
    if (c.empty()) return zk_g1_projective{};
    std::vector<zk_g1_projective> t(c.size());
    {
        std::vector<ZkTask<void>> tasks;
        for (size_t i = 1; i < c.size(); i++)
            tasks.push_back(zk_async(ctx, [&t, pts, &c, i] { zk_fr k = c[i].abi(); zk_g1_mul(&pts[i], &k, &t[i]); }));
        zk_fr k0 = c[0].abi();
        zk_g1_mul(&pts[0], &k0, &t[0]);
    }
    zk_g1_projective acc = t[0], u;
    for (size_t i = 1; i < c.size(); i++) { zk_g1_add(&acc, &t[i], &u); acc = u; }
    return acc;
}

// The argument list of ONE zk_msm_batch_dev call: jobs in the order they were added, points back in that order.
struct MsmJobs {
    std::vector<const zk_bases*> tables;
    std::vector<size_t> offs, lens; std::vector<const void*> scalars;
    size_t size() const { return tables.size(); }
    size_t add(const zk_bases* table, size_t off, const void* sc, size_t len) {
        tables.push_back(table); offs.push_back(off); scalars.push_back(sc); lens.push_back(len);
        return tables.size() - 1;
    }
    // a polynomial and, next to it, its copy shifted up to the degree bound (the same scalars from base `shift` on: they share a sort)
    size_t add_with_shift(const zk_bases* table, size_t shift, const void* sc, size_t len) {
        add(table, 0, sc, len);
        return add(table, shift, sc, len) - 1;
    }
    std::vector<zk_g1_projective> run(zk_ctx* ctx, int* rc) {
        std::vector<zk_g1_projective> outs(size());
        std::vector<void*> outp(size());
        for (size_t i = 0; i < size(); i++) outp[i] = &outs[i];
        *rc = zk_msm_batch_dev(ctx, size(), tables.data(), offs.data(), scalars.data(), lens.data(), outp.data());
        return outs;
    }
};

// What the caller of a prover entry point hands over (lanes [0] = share / plain, [1] = MAC share under SPDZ)
struct MarlinArgs {
    const zk_marlin_index* ix;
    const zk_bases *powers_g, *powers_gamma_g;
    const void* const* z;
    zk_rng* rng; int mask_on_device; bool shared;
    const void *const *tx, *const *ty, *const *tz;
    const zk_net_vtable* net;
};

// One Marlin::prove in progress, plain (shared = false, LANES = 1: zk_marlin_prove) or over this party's shares
// (zk_marlin_prove_shared[_spdz]): MpcMarlin::prove, src/marlin.rs:56 / arkworks/marlin/src/lib.rs:152-319 with F = MpcField.  Every
// step of the rounds is linear in the witness except z_A * z_B in round 2 (FieldShare::batch_mul over the 4|H| multiplication
// domain) and the zero test of the outer sum-check (an open); commitments / evaluations / opening witnesses of witness-dependent
// oracles are computed on the shares and opened (`publicize()`, lib.rs:171-228,296); public oracles enter a shared combination on
// the leader only (shift()).  LANES = 2: everything linear runs on the share lane and on the MAC lane, every open is MAC-checked;
// the MAC lane of this party's fresh randomness is the share itself (from_add_shared with key 1).
template <int LANES>
struct Marlin : MarlinArgs {
    zk_ctx* const ctx;
    const Shape s;
    const char* zb[2];                            // the (shares of the) padded assignment
    ZkHostLap laps; ZkSharedNet nt; const bool leader;
    Prover PL[2]; Prover& P = PL[0];              // lane 0 also computes everything public
    // divisibility / zero-sum checks whose verdict nothing waits for: the test is enqueued, the round's commitments go out behind it, the verdict
    // is read once the batch has synchronised the streams (a wait here left the device idle while the host prepared the batch: 0.1 - 0.15 ms per round)
    struct Pending { const uint32_t* verdict; const char* msg; };
    std::vector<Pending> pending;
    ZkEarlyMsm* early[N_PROVER] = {};             // MSMs started ahead of their round's batch (start_early), until commit_round collects them
    zk_g1_projective gamma_pts[3];                // powers_of_gamma_g: what a hiding bound of 1 uses
    // ---- what the steps hand on ----
    ProofState ps;                                // the transcript, the challenges, the commitments, the openings' host halves
    char *xb[2], *wq[2], *mask[2], *tmp[2];       // round 1 -> 2: x and w as coefficients, the mask polynomial, |H| elements of scratch
    Marlin(zk_ctx* c, const MarlinArgs& args)
        : MarlinArgs(args), ctx(c), s(ix, powers_g), zb{(const char*)z[0], LANES == 2 ? (const char*)z[1] : nullptr}, laps{c, "marlin."}, nt{c, net},
          leader(nt.leader()), PL{Prover{c, 0}, Prover{c, 1}} {
        for (int l = 0; l < LANES; l++)
            for (int i = 0; i < 12; i++) PL[l].polys[O_A_ROW + i] = Poly{(char*)ix->index_polys[i].ptr, ix->index_polys[i].n};
    }
    ~Marlin() {
        for (ZkEarlyMsm* em : early) if (em) (void)zk_msm_early_finish(ctx, em, nullptr);     // an error path: let them drain
    }
    int lanes_rc() const { for (int l = 0; l < LANES; l++) if (PL[l].rc != ZK_OK) return PL[l].rc; return (int)ZK_OK; }
    // sum_i c_i powers_of_gamma_g[i] on the context's helper threads (the blinding terms: ~1.2 ms of host scalar multiplications each,
    // under the device batch); the caller joins them before it returns
    ZkTask<zk_g1_projective> small_async(const std::vector<HF>& c) {
        return zk_async(ctx, [ctx = ctx, pts = gamma_pts, c] { return small_msm_par(ctx, pts, c); });
    }
    int check_later(const void* v, size_t count, const char* msg) {
        pending.push_back({nullptr, msg});                                       // (a failed launch ends the proof: nothing settles it)
        return zk_fr_vec_is_zero_launch(ctx, v, count, (int)pending.size() - 1, &pending.back().verdict);
    }
    int settle() {
        const char* failed = nullptr;
        for (auto& c : pending) if (!failed && *c.verdict != 0) failed = c.msg;
        pending.clear();
        if (failed) ZK_FAIL(ctx, ZK_ERR_STATE, failed);
        return ZK_OK;
    }
    // The sum over the parties of a device vector of shares (LANES = 2: MAC-checked), into scratch of its own
    int open_dev(const char* const v[2], size_t count, const std::string& name, char** out) {
        char* o = P.dev(name + "_open", count); char* dx = P.dev(name + "_dx", count);
        ZK_TRY(P.rc);
        if (LANES == 2) ZK_TRY(zk_shared_spdz_open_vec(nt, v[0], v[1], count, o, dx));
        else ZK_TRY(nt.open_vec(v[0], count, o));
        *out = o;
        return ZK_OK;
    }
    // Oracles of a round that exist before the round's last polynomial does (ORACLES: the mask polynomial, t, g_2; none of them
    // hiding, so no draw of the prover's rng depends on where their commitment is computed) have their MSMs started as soon as their
    // coefficients are on the device (msm_batch.hip: zk_msm_early_begin); the context stream goes on with the round's polynomial
    // arithmetic, commit_round collects them.  ZK_MARLIN_EARLY=0 keeps every job in the round's batch (A/B).
    int start_early(Oracle o) {
        static const bool early_on = !(getenv("ZK_MARLIN_EARLY") && atoi(getenv("ZK_MARLIN_EARLY")) == 0);
        // from |H| = 2^18 up only: measured on one box, alternating (profiles/r6_marlin_early_ab.jsonl) -- 2^20 65.0 / 64.7 -> 63.9 / 64.0 ms,
        // 2^18 21.8 -> 21.6; below that a round is a chain of latencies and the early job, which runs alone instead of in the round's
        // group launches (its own one-block sort, accumulate launch, reduce chain and host half), makes the proof LONGER:
        // 2^10 3.5 -> 4.2 ms, 2^12 4.3 -> 5.4, 2^14 6.1 -> 7.0, 2^16 9.5 -> 10.2
        if (!early_on || s.n < ((size_t)1 << 18)) return ZK_OK;
        if (ORACLES[o].early == EarlyMsm::No || (ORACLES[o].early == EarlyMsm::Plain && shared)) return ZK_OK;
        const Poly& p = P.polys[o];
        if (!p.n) return ZK_OK;
        if (oracle_bounded(o) && p.n - 1 > s.bound(o)) return ZK_OK;                      // (commit_round reports it)
        const size_t offs[2] = {0, oracle_bounded(o) ? s.max_degree - s.bound(o) : 0};
        return zk_msm_early_begin(ctx, oracle_bounded(o) ? 2 : 1, powers_g, offs, p.p, p.n, &early[o]);
    }
    // MarlinKZG10::commit for one round (marlin_pc/mod.rs:172-243): blinding polynomials in the reference's rng order, all MSMs
    // of the round (every lane) as one pipelined batch; shared oracles' commitments opened; the round's bytes into the transcript;
    // then the verdicts of the round's pending checks
    int commit_round(int round) {
        const std::vector<Oracle> os = round_oracles(round);
        ZK_TRY(ps.draw_blinds(round, rng));
        MsmJobs jobs;
        struct Acc { zk_g1_projective pt; bool has = false; } acc[2][2][N_PROVER];   // [lane][0 = comm / 1 = shifted]
        std::vector<Acc*> dest;                                                  // where the batch's points go, in job order
        ZkTask<zk_g1_projective> blind[2][N_PROVER];                             // [comm / shifted]: the blinding terms, under the device batch
        for (Oracle o : os) {
            const OracleInfo& oi = ORACLES[o];
            const Blinds& r = ps.rands[o];
            for (int lane = 0; lane < LANES; lane++) {
                if (lane == 1 && !oi.shared) continue;                           // public oracles are the same on every lane: committed once
                if (lane == 0 && early[o]) continue;                             // started early: collected below
                const Poly& p = PL[lane].polys[o];
                dest.push_back(&acc[lane][0][o]);
                if (!oracle_bounded(o)) { jobs.add(powers_g, 0, p.p, p.n); continue; }
                if (p.n - 1 > s.bound(o)) { ctx->last_error = std::string("zk_marlin_prove: ") + oi.label + " exceeds its degree bound"; return ZK_ERR_STATE; }
                jobs.add_with_shift(powers_g, s.max_degree - s.bound(o), p.p, p.n);
                dest.push_back(&acc[lane][1][o]);
            }
            if (oi.hiding) blind[0][o] = small_async(r.plain);
            if (oi.hiding && oracle_bounded(o)) blind[1][o] = small_async(r.shifted);
        }
        ZK_TRY(lanes_rc());
        laps.lap("commit.prep");
        int brc = ZK_OK;
        const std::vector<zk_g1_projective> outs = jobs.run(ctx, &brc);
        for (Oracle o : os) {                                                    // the jobs that were started early
            if (!early[o]) continue;
            zk_g1_projective eo[2]; void* eop[2] = {&eo[0], &eo[1]};
            ZkEarlyMsm* em = early[o]; early[o] = nullptr;                      // (finish deletes the handle)
            const int erc = zk_msm_early_finish(ctx, em, eop);
            if (brc == ZK_OK) brc = erc;
            acc[0][0][o] = {eo[0], true};
            if (oracle_bounded(o)) acc[0][1][o] = {eo[1], true};
        }
        laps.lap("commit.msm");
        zk_g1_projective bl[2][N_PROVER]; bool blinded[2][N_PROVER] = {};
        for (Oracle o : os)                                                      // joined before any return
            for (int w = 0; w < 2; w++) if ((blinded[w][o] = blind[w][o].valid())) bl[w][o] = blind[w][o].get();
        laps.lap("commit.blinds");
        ZK_TRY(brc);
        for (size_t i = 0; i < outs.size(); i++) *dest[i] = {outs[i], true};
        for (Oracle o : os)                                                      // the MAC lane of this party's fresh blinds is the share itself
            for (int w = 0; w < 2; w++)
                for (int lane = 0; lane < LANES && blinded[w][o]; lane++) {
                    Acc& c = acc[lane][w][o];
                    if (!c.has) continue;
                    zk_g1_projective t;
                    zk_g1_add(&c.pt, &bl[w][o], &t);
                    c.pt = t;
                }
        if (shared) {                                                            // first_comms.publicize() (lib.rs:180,205,228)
            ZkSmallItems pts[2], opened;
            std::vector<Acc*> what;
            for (Oracle o : os) {
                if (!ORACLES[o].shared) continue;
                for (int which = 0; which < 2; which++) {
                    if (!acc[0][which][o].has) continue;
                    for (int lane = 0; lane < LANES; lane++) pts[lane].g1.push_back(acc[lane][which][o].pt);
                    what.push_back(&acc[0][which][o]);
                }
            }
            ZK_TRY(zk_shared_open_small(nt, LANES, pts, &opened));
            for (size_t i = 0; i < what.size(); i++) what[i]->pt = opened.g1[i];
        }
        std::vector<zk_g1_projective> all;
        for (Oracle o : os) {
            all.push_back(acc[0][0][o].pt);
            if (oracle_bounded(o)) all.push_back(acc[0][1][o].pt);
        }
        ps.commitments(round, all);
        return settle();
    }

    // The transcript seed: PROTOCOL_NAME | index_vk | public_input (lib.rs:161-164).  Over shares the instance part of the
    // assignment is shared like the rest (from_public: the leader holds it) and opened here.  Out: gamma_pts, ps seeded
    int seed_transcript() {
        zk_g1_affine g[3];
        ZK_TRY(zk_bases_download_g1(ctx, powers_gamma_g, 0, 3, g));
        for (int i = 0; i < 3; i++) zk_g1_from_affine(&g[i], &gamma_pts[i]);
        const size_t ni = s.ni;
        std::vector<zk_fr> x(ni);
        const char* from = zb[0];
        if (shared && ni > 1) ZK_TRY(open_dev(zb, ni, "pub", (char**)&from));   // (ni = 1: no public input beside the constant 1, nothing to open)
        if (!shared || ni > 1) ZK_TRY(zk_memcpy_d2h(ctx, x.data(), from, ni * 32));
        ps.seed(ix, x.data(), ni);
        laps.lap("setup");
        return ZK_OK;
    }

    // Round 1 (prover.rs:216-404), every lane.  In: the assignment, the prover's rng.  Out: w, z_a, z_b, mask_poly committed; xb, wq, mask, tmp; alpha, eta
    int round1() {
        const Dom &H = s.H, &X = s.X;
        const size_t n = s.n, md = s.md, nwq = s.nwq;
        char* rnd = P.dev("rnd", 3 + md + 1);                                    // this party's (share of the) prover randomness: both lanes read it
        ZK_TRY(P.rc);
        const size_t host_n = mask_on_device ? 3 : 3 + md + 1;
        std::vector<zk_fr> h(host_n);
        ZK_TRY(zk_rng_fill_fr(rng, h.data(), host_n));
        ZK_TRY(zk_memcpy_h2d(ctx, rnd, h.data(), host_n * 32));
        if (mask_on_device) {
            uint8_t key[32];
            ZK_TRY(zk_rng_fill_bytes(rng, key, 32));
            ZK_TRY(zk_fr_random_dev(ctx, key, 0, rnd + 96, md + 1));
        }
        for (int l = 0; l < LANES; l++) {                                        // the mask polynomial first: its commitment (the round's longest job) starts now
            Prover& Q = PL[l];
            mask[l] = Q.dev("mask", md + 1);
            char* mq = Q.dev("mask_q", md + 1); char* mr = Q.dev("mask_r", n);
            Q.d2d(mask[l], rnd + 96, md + 1);
            ZK_TRY(Q.rc);
            ZK_TRY(zk_poly_divide_by_vanishing_dev(ctx, mask[l], md + 1, H.log, mq, mr));
            Q.op(ZK_OP_SUB, mask[l], mr, mask[l], 1);                            // the sum over H becomes zero
            Q.polys[O_MASK_POLY] = Poly{mask[l], md + 1};
            ZK_TRY(Q.rc);
        }
        ZK_TRY(start_early(O_MASK_POLY));
        for (int l = 0; l < LANES; l++) {
            Prover& Q = PL[l];
            char* z_a = Q.dev("z_a", n); char* z_b = Q.dev("z_b", n);
            ZK_TRY(Q.rc);
            ZK_TRY(zk_r1cs_matvec_dev(ctx, ix->r1cs, 0, zb[l], z_a, n));
            ZK_TRY(zk_r1cs_matvec_dev(ctx, ix->r1cs, 1, zb[l], z_b, n));
            xb[l] = Q.dev("x_poly", X.size);
            Q.d2d(xb[l], zb[l], X.size);
            Q.ntt(xb[l], X, 1);
            char* x_evals = Q.fft(H, Poly{xb[l], X.size}, "x_evals");
            char* w_evals = Q.dev("w_evals", n);
            tmp[l] = Q.dev("tmp_h", n);
            ZK_TRY(Q.rc);
            ZK_TRY(zk_fr_gather_dev(ctx, zb[l], ix->w_idx, n, w_evals));
            ZK_TRY(zk_fr_gather_dev(ctx, x_evals, ix->x_idx, n, tmp[l]));
            Q.op(ZK_OP_SUB, w_evals, tmp[l], w_evals, n);
            char* za = Q.dev("za_c", n); char* zbb = Q.dev("zb_c", n);
            Q.d2d(za, z_a, n); Q.d2d(zbb, z_b, n);
            Q.ntt_batch({w_evals, za, zbb}, H, 1);                               // the three interpolations of the round: one launch per pass
            const Poly w_h = Q.blind(w_evals, n, rnd, "w_h");
            wq[l] = Q.dev("w_poly", nwq);
            char* wr = Q.dev("w_rem", X.size);
            ZK_TRY(Q.rc);
            ZK_TRY(zk_poly_divide_by_vanishing_dev(ctx, w_h.p, n + 1, X.log, wq[l], wr));
            // (over shares the remainder is a share of zero: the reference's assert!(remainder.is_zero()) cannot be evaluated locally)
            if (!shared) ZK_TRY(check_later(wr, X.size, "zk_marlin_prove: w polynomial is not divisible by v_X"));
            Q.polys[O_W] = Poly{wq[l], nwq};
            Q.polys[O_Z_A] = Q.blind(za, n, rnd + 32, "z_a_poly");
            Q.polys[O_Z_B] = Q.blind(zbb, n, rnd + 64, "z_b_poly");
            ZK_TRY(Q.rc);
        }
        laps.lap("polys");
        ZK_TRY(commit_round(1));
        laps.lap("commit");
        ps.challenges(1, s);
        laps.lap("round1");
        return ZK_OK;
    }

    // Round 2 (prover.rs:438-565).  In: alpha, eta; z_a, z_b, w (wq), x (xb), mask; tmp.  Out: t, g_1, h_1 committed; v_h_alpha; beta
    int round2() {
        // public: r(alpha, X) on H, t = sum_M eta_M M^T r, their evaluations over the multiplication domain (computed once)
        const Dom &H = s.H, &X = s.X, &MUL = s.MUL;
        const size_t n = s.n, md = s.md, nwq = s.nwq;
        const HF one = HF::one(), &alpha = ps.alpha, &v_h_alpha = ps.v_h_alpha, *const eta = ps.eta;
        char* elems = P.dev("h_elems", n);
        char* ra = P.dev("r_alpha", n);
        ZK_TRY(P.rc);
        ZK_TRY(zk_fr_powers_launch(ctx, H.gen.v, one.v, n, elems, ZK_FR_EXT));
        ZK_TRY(zk_fr_powers_launch(ctx, one.v, alpha.v, n, ra, ZK_FR_EXT));      // the constant vector alpha
        P.op(ZK_OP_SUB, ra, elems, ra, n);
        ZK_TRY(P.rc);
        ZK_TRY(zk_fr_batch_inverse_dev(ctx, ra, n));
        P.scale(ra, v_h_alpha, ra, n);                                           // r(alpha, X) on H (ahp/mod.rs:352-360)
        char* t_ev = P.dev("t_ev", n);
        for (int which = 0; which < 3; which++) {                                // calculate_t on the transposed matrices
            ZK_TRY(P.rc);
            ZK_TRY(zk_r1cs_matvec_dev(ctx, ix->r1cs_t, which, ra, which == 0 ? t_ev : tmp[0], n));
            if (which == 0) P.scale(t_ev, eta[0], t_ev, n);
            else { P.scale(tmp[0], eta[which], tmp[0], n); P.op(ZK_OP_ADD, t_ev, tmp[0], t_ev, n); }
        }
        P.ntt_batch({t_ev, ra}, H, 1);
        for (int l = 0; l < LANES; l++) PL[l].polys[O_T] = Poly{t_ev, n};
        ZK_TRY(P.rc);
        ZK_TRY(start_early(O_T));                                                // public: the product of the two witness vectors and h_1 are still to come
        char* e_rp = P.padded(MUL, Poly{ra, n}, "e_r"); char* e_tp = P.padded(MUL, P.polys[O_T], "e_t");
        P.ntt_batch({e_rp, e_tp}, MUL, 0);
        char *e_a[2], *e_b[2], *e_s[2], *e_z[2];
        for (int l = 0; l < LANES; l++) {
            Prover& Q = PL[l];
            char* zp = Q.dev("z_poly", n + 1);                                   // z = w v_X + x
            Q.zero(zp, n + 1);
            Q.d2d(zp + 32 * X.size, wq[l], nwq);
            Q.op(ZK_OP_SUB, zp, wq[l], zp, nwq);
            Q.op(ZK_OP_ADD, zp, xb[l], zp, X.size);
            e_a[l] = Q.padded(MUL, Q.polys[O_Z_A], "e_a"); e_b[l] = Q.padded(MUL, Q.polys[O_Z_B], "e_b");
            e_s[l] = Q.dev("e_s", MUL.size);
            e_z[l] = Q.padded(MUL, Poly{zp, n + 1}, "e_z");
            Q.ntt_batch({e_a[l], e_b[l], e_z[l]}, MUL, 0);
            ZK_TRY(Q.rc);
        }
        // z_a z_b: the one product of two witness vectors (`DensePolynomial::mul` on MpcField = FieldShare::batch_mul)
        if (!shared) P.op(ZK_OP_MUL, e_a[0], e_b[0], e_s[0], MUL.size);
        else ZK_TRY(zk_shared_beaver_mul(nt, LANES, (const void* const*)e_a, (const void* const*)e_b, (void* const*)e_s, MUL.size, tx, ty, tz, "mp_bv"));
        char *hq[2], *hr[2];
        for (int l = 0; l < LANES; l++) {
            Prover& Q = PL[l];
            // r(alpha, X) (eta_c z_a z_b + eta_a z_a + eta_b z_b) - z t on the multiplication domain (public * own value: local): one pass
            ZK_TRY(Q.rc);
            ZK_TRY(zk_fr_outer_q1_launch(ctx, e_s[l], e_a[l], e_b[l], e_z[l], e_rp, e_tp, eta[0].v, eta[1].v, eta[2].v, e_s[l], MUL.size));
            Q.ntt(e_s[l], MUL, 1);                                               // q_1 (prover.rs:517-541)
            Q.op(ZK_OP_ADD, e_s[l], mask[l], e_s[l], md + 1);
            hq[l] = Q.dev("h1_q", MUL.size - n); hr[l] = Q.dev("h1_r", n);
            ZK_TRY(Q.rc);
            ZK_TRY(zk_poly_divide_by_vanishing_dev(ctx, e_s[l], MUL.size, H.log, hq[l], hr[l]));
        }
        // the outer sum-check's zero test (prover.rs:547-550): over shares the constant term is opened
        const char* const not_zero = OUTER_NOT_ZERO;
        char* zo = nullptr;
        if (!shared) ZK_TRY(check_later(hr[0], 1, not_zero));
        else ZK_TRY(open_dev(hr, 1, "zero", &zo));
        const bool zero_sum = !shared || P.is_zero(zo, 1);
        ZK_TRY(P.rc);
        if (!zero_sum) ZK_FAIL(ctx, ZK_ERR_STATE, not_zero);
        for (int l = 0; l < LANES; l++) {
            PL[l].polys[O_G_1] = Poly{hr[l] + 32, n - 1};
            PL[l].polys[O_H_1] = Poly{hq[l], s.h1n};
        }
        laps.lap("polys");
        ZK_TRY(commit_round(2));
        laps.lap("commit");
        ps.challenges(2, s);
        laps.lap("round2");
        return ZK_OK;
    }

    // Round 3 (prover.rs:583-716): public values only.  In: alpha, eta, beta, v_h_alpha.  Out: g_2, h_2 committed; vv; gamma
    int round3() {
        const Dom &K = s.K, &B = s.B;
        const HF &alpha = ps.alpha, &beta = ps.beta, &vv = ps.vv, *const eta = ps.eta;
        char* f_ev = P.dev("f_ev", K.size);
        char* a_ev = P.dev("a_ev", B.size); char* b_ev = P.dev("b_ev", B.size);
        ZK_TRY(P.rc);
        { zk_fr al = alpha.abi(), be = beta.abi(), v = vv.abi(), et[3] = {eta[0].abi(), eta[1].abi(), eta[2].abi()};
          ZK_TRY(zk_marlin_round3_f_evals_dev(ctx, ix->on_k, K.size, &al, &be, et, &v, f_ev));
          ZK_TRY(zk_marlin_round3_ab_evals_dev(ctx, ix->on_b, B.size, &al, &be, et, &v, a_ev, b_ev)); }
        P.ntt(f_ev, K, 1);
        for (int l = 0; l < LANES; l++) PL[l].polys[O_G_2] = Poly{f_ev + 32, K.size - 1};
        ZK_TRY(P.rc);
        ZK_TRY(start_early(O_G_2));                                              // both of its commitments (degree bound |K| - 2), under the division that yields h_2
        char* f_on_b = P.fft(B, Poly{f_ev, K.size}, "f_on_b");                  // a - b f on B itself (degree <= 4|K| - 4 < |B|)
        P.op(ZK_OP_MUL, b_ev, f_on_b, b_ev, B.size);
        P.op(ZK_OP_SUB, a_ev, b_ev, a_ev, B.size);
        P.ntt(a_ev, B, 1);
        char* h2q = P.dev("h2_q", B.size - K.size); char* h2r = P.dev("h2_r", K.size);
        ZK_TRY(P.rc);
        ZK_TRY(zk_poly_divide_by_vanishing_dev(ctx, a_ev, B.size, K.log, h2q, h2r));
        ZK_TRY(check_later(h2r, K.size, INNER_NOT_DIVISIBLE));
        for (int l = 0; l < LANES; l++) PL[l].polys[O_H_2] = Poly{h2q, B.size - K.size};
        laps.lap("polys");
        ZK_TRY(commit_round(3));
        laps.lap("commit");
        ps.challenges(3, s);
        laps.lap("round3");
        return ZK_OK;
    }

    // The evaluations of the query set, absorbed, and the linear combinations over them.  In: oracles, challenges.  Out: ps.qs, ps.xi, ps.plan
    int evaluate() {
        // one batch (two launches, one copy back); z_b and g_1 are shared: every lane's evaluation, opened (`evaluations.publicize()`, lib.rs:296)
        std::vector<zk_poly_ref> refs;
        std::vector<zk_fr> pts;
        for (const QueryValue& w : QUERY_VALUES) { const Poly& p = P.polys[w.o]; refs.push_back(zk_poly_ref{p.p, p.n}); pts.push_back(ps.point(w.at_gamma).abi()); }
        static_assert(QUERY_VALUES[0].o == O_Z_B && QUERY_VALUES[1].o == O_G_1, "the two shared values come first");
        if (LANES == 2)                                                          // behind them: the MAC lane of the two shared ones
            for (Oracle o : {O_Z_B, O_G_1}) { const Poly& p = PL[1].polys[o]; refs.push_back(zk_poly_ref{p.p, p.n}); pts.push_back(ps.beta.abi()); }
        std::vector<zk_fr> vals(refs.size());
        ZK_TRY(zk_poly_evaluate_batch_dev(ctx, refs.data(), pts.data(), refs.size(), vals.data()));
        if (shared) {
            ZkSmallItems frs[2], opened;
            frs[0].fr = {vals[0], vals[1]};
            if (LANES == 2) frs[1].fr = {vals[N_QUERY_VALUES], vals[N_QUERY_VALUES + 1]};
            ZK_TRY(zk_shared_open_small(nt, LANES, frs, &opened));
            vals[0] = opened.fr[0]; vals[1] = opened.fr[1];
        }
        ZK_TRY(P.rc);
        ps.evaluated(vals.data(), s);
        laps.lap("evals+lc");
        return ZK_OK;
    }

    // open_combinations (marlin/mod.rs:213-306, marlin_pc/mod.rs:245-340).  In: ps.plan, the query points.  Out: ps.wit, ps.has_rv, ps.rvs.
    // Over shares: the witness of a share combination is a share of the witness.  A combination with a shared oracle in it runs on
    // every lane, public oracles entering it on the leader only (shift(): in both lanes, mac_share = 1 there), and its witness
    // (and random_v) is opened; a combination of public oracles only (the query point gamma) is computed alike by every party.
    int open_combinations() {
        MsmJobs jobs;
        size_t counts[2][2] = {{0, 0}, {0, 0}};                                  // [query point][lane]
        std::vector<ZkTask<zk_g1_projective>> extra[2];                          // the blinding witnesses: host threads, joined after the batch
        bool q_shared[2] = {false, false};
        for (int q = 0; q < 2; q++) {
            const HF z = ps.point(q);
            const OpenPlan& plan = ps.plan[q];
            const std::vector<std::pair<Oracle, HF>>&terms = plan.terms, &shifted = plan.shifted;
            bool any_shared = false;
            for (auto& t : terms) any_shared = any_shared || (shared && ORACLES[t.first].shared);
            q_shared[q] = any_shared;
            size_t cn = 0;
            for (auto& t : terms) cn = std::max(cn, P.polys[t.first].n);
            for (int l = 0; l < (any_shared ? LANES : 1); l++) {
                Prover& Q = PL[l];
                char* comb = Q.dev("comb" + std::to_string(q), cn);
                // one launch for the whole combination (vec_ops.hip::k_lincomb)
                std::vector<const void*> tp; std::vector<size_t> tn; std::vector<Fr> tk;
                for (auto& t : terms) {
                    if (any_shared && !ORACLES[t.first].shared && !leader) continue;   // a public oracle in a shared combination: the leader's
                    const Poly& p = Q.polys[t.first];
                    tp.push_back(p.p); tn.push_back(p.n);
                    tk.push_back(t.second.v);
                }
                ZK_TRY(Q.rc);
                ZK_TRY(zk_fr_lincomb_launch(ctx, (int)tp.size(), tp.data(), tn.data(), tk.data(), comb, cn));
                char* quo = Q.dev("quo" + std::to_string(q), cn);
                ZK_TRY(Q.rc);
                { zk_fr zz = z.abi(); ZK_TRY(zk_poly_divide_by_linear_dev(ctx, comb, cn, &zz, quo, nullptr)); }
                const size_t first_job = jobs.add(powers_g, 0, quo, cn - 1);
                int si = 0;
                for (auto& sh : shifted) {
                    if (any_shared && !ORACLES[sh.first].shared && !leader) continue;
                    const Poly& p = Q.polys[sh.first];
                    char* wq2 = Q.dev("swit" + std::to_string(q) + "_" + std::to_string(si++), p.n);
                    ZK_TRY(Q.rc);
                    { zk_fr zz = z.abi(); ZK_TRY(zk_poly_divide_by_linear_dev(ctx, p.p, p.n, &zz, wq2, nullptr)); }
                    Q.scale(wq2, sh.second, wq2, p.n - 1);
                    jobs.add(powers_g, s.max_degree - s.bound(sh.first), wq2, p.n - 1);
                }
                counts[q][l] = jobs.size() - first_job;
            }
            const OpenBlinds ob = ps.blinds_at(q);
            if (ob.hiding) extra[q].push_back(small_async(ob.plain_w));
            if (!ob.shifted_w.empty()) extra[q].push_back(small_async(ob.shifted_w));
        }
        ZK_TRY(lanes_rc());
        int orc = ZK_OK;
        const std::vector<zk_g1_projective> outs = jobs.run(ctx, &orc);
        std::vector<zk_g1_projective> extra_pts[2];
        for (int q = 0; q < 2; q++) for (auto& f : extra[q]) extra_pts[q].push_back(f.get());
        ZK_TRY(orc);
        size_t k = 0;
        std::vector<zk_g1_projective> wits;
        for (int q = 0; q < 2; q++) {
            zk_g1_projective wl[2];
            const int nl = q_shared[q] ? LANES : 1;
            for (int l = 0; l < nl; l++) {
                zk_g1_projective w = outs[k];
                for (size_t i = 1; i < counts[q][l]; i++) { zk_g1_projective t; zk_g1_add(&w, &outs[k + i], &t); w = t; }
                for (auto& e : extra_pts[q]) { zk_g1_projective t; zk_g1_add(&w, &e, &t); w = t; }    // own randomness: the same on the MAC lane
                k += counts[q][l];
                wl[l] = w;
            }
            if (q_shared[q]) {                                                   // the witness (and random_v) of a shared combination: opened
                ZkSmallItems mine[2], opened;
                for (int l = 0; l < LANES; l++) { mine[l].g1.push_back(wl[l]); if (ps.has_rv[q]) mine[l].fr.push_back(ps.rvs[q].abi()); }
                ZK_TRY(zk_shared_open_small(nt, LANES, mine, &opened));
                wl[0] = opened.g1[0];
                if (ps.has_rv[q]) ps.rvs[q] = HF::from_abi(opened.fr[0]);
            }
            wits.push_back(wl[0]);
        }
        ps.witnesses(wits.data());
        laps.lap("open");
        return ZK_OK;
    }
};

template <int LANES>
int marlin_impl(zk_ctx* ctx, const MarlinArgs& a, uint8_t* proof_out, size_t cap, size_t* proof_len, uint64_t* bytes_sent) {
    const zk_marlin_index* ix = a.ix;
    if (!ctx || !ix || !a.powers_g || !a.powers_gamma_g || !a.z[0] || (LANES == 2 && !a.z[1]) || !a.rng || !proof_out || !proof_len) return ZK_ERR_ARG;
    ZK_TRY(check_index_and_srs(ctx, ix, a.powers_g, a.powers_gamma_g));
    if (cap < zk_marlin_proof_max_size()) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: output buffer smaller than zk_marlin_proof_max_size()");
    Marlin<LANES> m(ctx, a);
    ZK_TRY(check_sizes(ctx, m.s.max_degree, m.s.n, m.s.K.size, m.s.B.size));
    ZK_TRY(m.seed_transcript());
    ZK_TRY(m.round1());
    ZK_TRY(m.round2());
    ZK_TRY(m.round3());
    ZK_TRY(m.evaluate());
    ZK_TRY(m.open_combinations());
    if (!m.ps.write(proof_out, cap, proof_len)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_marlin_prove: output buffer too small");
    if (bytes_sent) *bytes_sent = m.nt.bytes;
    return ZK_OK;
}

}  // namespace

extern "C" size_t zk_marlin_proof_max_size(void) { return 8 + 3 * 8 + 9 * 49 + 2 * 48 + 8 + 7 * 32 + 8 + 3 + 8 + 2 * (49 + 32) + 1; }

extern "C" int zk_marlin_prove(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g,
                               const void* z_dev, zk_rng* zk_rng_, int mask_on_device, uint8_t* proof_out, size_t cap, size_t* proof_len) {
    ZK_API_BEGIN(ctx)
    const void *z[2] = {z_dev, nullptr}, *none[2] = {nullptr, nullptr};
    return marlin_impl<1>(ctx, MarlinArgs{ix, powers_g, powers_gamma_g, z, zk_rng_, mask_on_device, false, none, none, none, nullptr}, proof_out, cap,
                          proof_len, nullptr);
    ZK_API_END
}

// MpcMarlin::prove over additive shares (src/marlin.rs:56): z_share_dev = this party's share of the padded assignment, zk_rng =
// this party's own generator (its share of the prover's randomness); tx / ty / tz = Beaver triple shares for the one product of
// round 2 (4|H| elements... the multiplication domain) or NULL for DummyFieldTripleSource.  Every party returns the same bytes.
extern "C" int zk_marlin_prove_shared(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g,
                                      const void* z_share_dev, zk_rng* zk_rng_, int mask_on_device, const void* tx, const void* ty,
                                      const void* tz, const zk_net_vtable* net, uint8_t* proof_out, size_t cap, size_t* proof_len,
                                      uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    const void* z[2] = {z_share_dev, nullptr};
    const void *txs[2] = {tx, nullptr}, *tys[2] = {ty, nullptr}, *tzs[2] = {tz, nullptr};
    return marlin_impl<1>(ctx, MarlinArgs{ix, powers_g, powers_gamma_g, z, zk_rng_, mask_on_device, true, txs, tys, tzs, net}, proof_out, cap, proof_len,
                          bytes_sent);
    ZK_API_END
}

// ... over SPDZ shares (the `malicious` feature; BASELINE config 5's prover): lanes [0] = share, [1] = MAC share.
extern "C" int zk_marlin_prove_shared_spdz(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g,
                                           const void* const z_lanes_dev[2], zk_rng* zk_rng_, int mask_on_device,
                                           const void* const tx_lanes[2], const void* const ty_lanes[2], const void* const tz_lanes[2],
                                           const zk_net_vtable* net, uint8_t* proof_out, size_t cap, size_t* proof_len, uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    const void* none[2] = {nullptr, nullptr};
    return marlin_impl<2>(ctx, MarlinArgs{ix, powers_g, powers_gamma_g, z_lanes_dev ? z_lanes_dev : none, zk_rng_, mask_on_device, true, tx_lanes ? tx_lanes : none,
                                          ty_lanes ? ty_lanes : none, tz_lanes ? tz_lanes : none, net}, proof_out, cap, proof_len, bytes_sent);
    ZK_API_END
}
