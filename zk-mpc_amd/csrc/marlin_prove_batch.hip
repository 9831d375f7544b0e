// marlin_prove_batch.hip -- count Marlin proofs of ONE index in one call (Marlin::prove, arkworks/marlin/src/lib.rs:152-319, for
// count assignments).  Proof k is byte for byte what zk_marlin_prove writes for (z_k, rngs[k]), and rngs[k] is left as that call leaves it.
//
// A small proof leaves the device idle: every round ends in a chain of sort -> accumulate -> fold -> grid per commitment and a host
// wait for the transcript.  A shorter chain does not remove the waits; they can only be shared.  Here the proofs of a chunk go
// through seed -> round 1 -> round 2 -> round 3 -> evaluate -> open in lock-step:
//   * every oracle and every intermediate of the chunk lives in one call-owned allocation, proof after proof at a fixed stride
//     (Layout), so the multi-vector MSM jobs (msm.hip: zk_msm_prepare_multi), the strided transforms (ntt.hip) and the batched
//     kernels (marlin_batch.hip, poly.hip, r1cs.hip) apply directly: the launches of a step do not grow with the chunk;
//   * a round's commitments are one multi-vector job per (oracle, offset), each on a stream of its own, enqueued before any is
//     collected; the blinding terms sum c_i powers_of_gamma_g[i] of all proofs (about 7 scalar multiplications per proof and step)
//     are one zk_g1_lincomb_launch per step on a stream of its own once they are too many for the host's helper threads, which
//     is where the single prover computes them (HOST_BLIND_MULS);
//   * each proof keeps its own transcript, challenges and blinding scalars on the host (marlin_prove_int.hpp: ProofState, the single
//     prover's); the per-proof host loops run over ranges of proofs on the context's pool (zk_over_ranges);
//   * no MSM starts early (Marlin::start_early hides ONE proof's latency; the batch hides it by width).
// The per-proof constants of a step (alpha, eta, beta, ..., the opening's coefficients) are a small device table written once per
// step through a ZkStage.  The only per-proof launches are the device mask sampler (once per call and cheap).  A failing zero test
// says that SOME proof of the chunk fails; which one, and with which text, is then found by running the single prover over the
// chunk's proofs in order (the failures -- an unsatisfied system, w not divisible by v_X, the inner sum-check -- depend on the
// assignment and the index alone, not on the randomness).
//
// The same Chunk proves over this party's shares (zk_marlin_prove_shared[_spdz]_batch: MpcMarlin::prove, src/marlin.rs:56, for count
// shared assignments; lanes = 1: additive shares, 2: SPDZ, the MAC lane beside the share lane).  What Marlin<LANES> does per proof
// (marlin_prove.hip) happens here per chunk:
//   * every witness-dependent region holds lanes * C vectors at one stride, lane after lane (vector l * C + k: lane l of proof k), so a
//     linear step is ONE launch over lanes * C vectors and a shared oracle's commitment ONE multi-vector job; the kernels that read a
//     per-proof constant or a public per-proof operand take vector v's from proof v mod C (marlin_batch.hip).  Public work -- r(alpha, X),
//     t, all of round 3, the index polynomials' evaluations -- is computed once per proof;
//   * each exchange of the single prover happens once per chunk: the instance parts as one vector, z_a z_b as one Beaver product over
//     C |MUL| elements per lane, the C constant terms of the outer sum-check as one vector, and one small open per step (the round's
//     commitments, the evaluations, the witness at beta) whose items marlin_shared_plan.hpp lays out;
//   * nothing can be re-run over shares: the outer sum-check's verdict is read per proof from the opened constant terms, which every party
//     sees alike, and the first failing proof ends the call at every party behind the same exchange;
//   * the proofs are collected in memory of the call and copied out behind the last chunk: an error leaves the output untouched.
#include "../../include/zkmpc_hip.h"
#include "devutil.cuh"
#include "groth16_int.hpp"
#include "marlin_prove_int.hpp"
#include "marlin_shared_plan.hpp"
#include "sharednet.hpp"
#include <algorithm>
#include <cstdlib>
#include <string>
#include <vector>

using namespace zk;
using namespace zk::marlin;

namespace {

constexpr size_t HOST_TASKS = 16;
// The blinding terms of a step go to the host's helper threads up to this many scalar multiplications (0.2 ms each on a core, sixteen
// side by side: at most 2 ms, under the step's MSM jobs) and to the device beyond: k_g1_lincomb is one lane per term, about 4 ms
// whatever the number of terms (measured at |H| = 2^10: three launches added 11.8 ms to a batch of two proofs)
constexpr size_t HOST_BLIND_MULS = 160;
constexpr int MAX_ROUND_JOBS = 4;                 // multi-vector jobs in flight in one step (ZK_SLOT_G16_BATCH has five slots)
static_assert(MAX_ROUND_JOBS <= ZK_SLOT_G16_COUNT, "a step's jobs each take a scratch slot of their own");

// count vectors of one length in the call's allocation: proof k's at p + k * stride elements
struct Vec {
    char* p = nullptr; size_t stride = 0;
    char* at(size_t k) const { return p + k * stride * 32; }
};

// Where everything of a chunk of C proofs lives: place() hands out the regions of one allocation in a fixed order (base = NULL:
// the bytes it takes).  Over shares a witness-dependent region holds lanes * C vectors, lane after lane; what is public holds C.
struct Layout {
    Vec rnd, mask, mask_q, mask_r, sums, z_a, z_b, xb, x_ev, w_ev, tmp, w_h, wq, wr, za_p, zb_p;       // round 1
    Vec ra, mv[3], t_ev, e_r, e_t, e_a, e_b, e_s, e_z, zp, h1_q, h1_r, zt;                             // round 2
    Vec den, f_ev, a_ev, b_ev, f_on_b, h2_q, h2_r;                                                     // round 3
    Vec comb[2], quo[2], sw[2], spans, pub, lc_out, ntt_tmp;                                           // evaluate, open
    Vec zin, pub_open, pub_dx, zt_open, zt_dx;                                                         // over shares: the lanes' assignments side by side; the vector opens
    char* elems = nullptr;                                                                             // the elements of H: one vector for every proof
    char* beaver = nullptr;                                                                            // over shares: the product's scratch, (2 lanes + 3) C |MUL| elements
    size_t lc_segments = 0;
    size_t place(char* base, size_t C, const Shape& s, int lanes = 1, bool shared = false) {
        size_t used = 0;
        auto take = [&](size_t elems_) { char* p = base ? base + used : nullptr; used += (elems_ * 32 + 255) & ~(size_t)255; return p; };
        auto pvec = [&](Vec& v, size_t per) { v.stride = std::max<size_t>(per, 1); v.p = take(C * v.stride); };                     // public: one vector per proof
        auto vec = [&](Vec& v, size_t per) { v.stride = std::max<size_t>(per, 1); v.p = take((size_t)lanes * C * v.stride); };      // one per lane and proof
        const size_t n = s.n, Xs = s.X.size, M = s.MUL.size, Ks = s.K.size, Bs = s.B.size;
        size_t sums_n = zk_poly_divv_sums_elems(s.md + 1, s.H.log);
        sums_n = std::max(sums_n, zk_poly_divv_sums_elems(n + 1, s.X.log));
        sums_n = std::max(sums_n, zk_poly_divv_sums_elems(M, s.H.log));
        sums_n = std::max(sums_n, zk_poly_divv_sums_elems(Bs, s.K.log));
        vec(rnd, 3 + s.md + 1); vec(mask, s.md + 1); vec(mask_q, s.md + 1 - n); vec(mask_r, n); vec(sums, sums_n);
        vec(z_a, n); vec(z_b, n); vec(xb, Xs); vec(x_ev, n); vec(w_ev, n); vec(tmp, n); vec(w_h, n + 1); vec(wq, s.nwq); vec(wr, Xs);
        vec(za_p, n + 1); vec(zb_p, n + 1);
        pvec(ra, n); for (Vec& v : mv) pvec(v, n); pvec(t_ev, n);
        pvec(e_r, M); pvec(e_t, M); vec(e_a, M); vec(e_b, M); vec(e_s, M); vec(e_z, M); vec(zp, n + 1); vec(h1_q, M - n); vec(h1_r, n); vec(zt, 1);
        pvec(den, 3 * Ks); pvec(f_ev, Ks); pvec(a_ev, Bs); pvec(b_ev, Bs); pvec(f_on_b, Bs); pvec(h2_q, Bs - Ks); pvec(h2_r, Ks);
        vec(comb[0], s.cn[0]); vec(quo[0], s.cn[0]); pvec(comb[1], s.cn[1]); pvec(quo[1], s.cn[1]);      // at beta: the witness's oracles; at gamma: public ones
        vec(sw[0], n); pvec(sw[1], Ks);
        vec(spans, 2 * zk_poly_divlin_spans(std::max(s.cn[0], s.cn[1])));
        vec(pub, s.ni);
        lc_segments = 3 * C;
        pvec(lc_out, 10);                          // per proof: three affine points (96 bytes each) and their three flags
        vec(ntt_tmp, std::max(std::max(M, Bs), n));
        elems = take(n);
        if (shared) {
            if (lanes > 1) vec(zin, s.nv);
            pvec(pub_open, s.ni); pvec(pub_dx, s.ni); pvec(zt_open, 1); pvec(zt_dx, 1);
            beaver = take((size_t)(2 * lanes + 3) * C * M);
        }
        return used;
    }
};

// A multi-vector job of a step over `vectors` vectors (C, or lanes * C for a shared oracle) and where its points go
struct StepJob { const char* scalars; size_t stride, len, off, vectors; std::vector<zk_g1_projective> out; };

// What the caller's arguments are for one chunk (lanes [0] = share / plain, [1] = MAC share under SPDZ)
struct ChunkArgs {
    const char* z[2]; size_t zs;                  // the chunk's assignments
    zk_rng* const* rngs;
    int mask_on_device;
    int lanes; bool shared;
    ZkSharedNet* nt;                              // over shares: the call's transport
    const char *tx[2], *ty[2], *tz[2];            // the chunk's Beaver triples (all NULL: the dummy source)
    uint8_t* proofs_out; size_t slot; size_t* proof_lens;      // where the chunk's proofs go
};

struct Chunk {
    zk_ctx* const ctx;
    const zk_marlin_index* const ix;
    const zk_bases *const powers_g, *const powers_gamma_g;
    const Shape& s;
    const Layout& L;
    ZkStage& stage;
    char* const down;                             // page-locked: what a step reads back
    const size_t C;                               // proofs in this chunk
    const ChunkArgs A;
    const char* const z; const size_t zs;         // their assignments (the share lane's)
    zk_rng* const* const rngs;
    const int mask_on_device;
    const int lanes; const bool shared, leader;
    const size_t V;                               // vectors of a witness-dependent region: lanes * C, lane after lane
    const size_t wrap;                            // what the kernels with a per-proof operand take as `proofs`: 0 in the plain batch, where vector k is proof k
    const zk_g1_projective* const gamma_pts;      // powers_of_gamma_g[0 .. 2] on the host
    std::vector<ProofState> P;
    Vec polys[N_PROVER];                          // a shared oracle's (ORACLES[o].shared) over shares: V vectors
    Vec zv;                                       // the assignments, lane after lane
    ZkHostLap xl;                                 // over shares: the host's time between exchanges (local) and inside each kind of them
    const uint32_t* verdicts[3] = {nullptr, nullptr, nullptr};
    static const char* const check_text[3];

    Chunk(zk_ctx* c, const zk_marlin_index* ix_, const zk_bases* pg, const zk_bases* pgg, const Shape& s_, const Layout& L_, ZkStage& st, char* down_, size_t C_,
          const ChunkArgs& a, const zk_g1_projective* gp)
        : ctx(c), ix(ix_), powers_g(pg), powers_gamma_g(pgg), s(s_), L(L_), stage(st), down(down_), C(C_), A(a), z(a.z[0]), zs(a.zs), rngs(a.rngs),
          mask_on_device(a.mask_on_device), lanes(a.lanes), shared(a.shared), leader(!a.shared || a.nt->leader()), V((size_t)a.lanes * C_),
          wrap(a.shared ? C_ : 0), gamma_pts(gp), P(C_), xl{c, "marlin_shared."} {}
    // how many vectors an oracle's region holds, and the point of lane l of proof k among a job's
    size_t vectors_of(Oracle o) const { return shared && o < N_PROVER && ORACLES[o].shared ? V : C; }

    template <class Fn>
    int each(const Fn& f) {                       // f(k) for every proof of the chunk, over ranges on the pool; the first failing proof's code
        zk_over_ranges(ctx, C, HOST_TASKS, [&](size_t lo, size_t hi) { for (size_t k = lo; k < hi; k++) if (P[k].rc == ZK_OK) P[k].rc = f(k); });
        for (size_t k = 0; k < C; k++)
            if (P[k].rc != ZK_OK) { if (!P[k].err.empty()) ctx->last_error = P[k].err; return P[k].rc; }
        return ZK_OK;
    }
    // (cnt vectors: V for what depends on the witness, C for what is public)
    int ntt(const Vec& v, const Dom& d, int inverse, size_t cnt) { return zk_ntt_launch_strided(ctx, v.p, cnt, v.stride, d.log, inverse, 0, L.ntt_tmp.p); }
    // the zero-padded copies evaluate_over_domain transforms
    int padded(const Vec& out, const Dom& d, const Vec& p, size_t pn, size_t cnt) {
        if (pn < d.size) ZK_TRY(zk_b_zero(ctx, out.p + 32 * pn, out.stride, d.size - pn, cnt));
        return zk_b_copy(ctx, out.p, out.stride, p.p, p.stride, std::min(pn, d.size), cnt);
    }
    int divv(const Vec& c, size_t cn, const Dom& d, const Vec& q, const Vec& rem, size_t cnt) {
        return zk_poly_divide_by_vanishing_strided(ctx, c.p, c.stride, cn, d.log, cnt, q.p, q.stride, rem.p, rem.stride, L.sums.p);
    }
    // The sum over the parties of `count` elements of shares, lane l's at v + l * lane_stride elements (lanes = 2: MAC-checked)
    int open_vec(const char* v, size_t lane_stride, size_t count, char* out, char* dx) {
        xl.lap("local");
        const int rc = lanes == 2 ? zk_shared_spdz_open_vec(*A.nt, v, v + lane_stride * 32, count, out, dx) : A.nt->open_vec(v, count, out);
        xl.lap("vec_open");
        return rc;
    }
    // one small open of the chunk: mine[l] = lane l's items, by proof within each kind
    int open_small(const ZkSmallItems mine[2], ZkSmallItems* opened) {
        xl.lap("local");
        const int rc = zk_shared_open_small(*A.nt, lanes, mine, opened);
        xl.lap("small_open");
        return rc;
    }
    // one row of `per` constants per proof, on the device
    template <class Fn>
    int table(size_t per, const Fn& fill, const FrK** out) {
        std::vector<FrK> t(C * per);
        for (size_t k = 0; k < C; k++) fill(k, &t[k * per]);
        const void* d;
        ZK_TRY(stage.put(t.data(), t.size() * sizeof(FrK), &d));
        *out = (const FrK*)d;
        return ZK_OK;
    }
    int check_later(int slot, const void* v, size_t count) { return zk_fr_vec_is_zero_launch(ctx, v, count, slot, &verdicts[slot]); }

    // ---- a step's commitments: the multi-vector jobs side by side, the blinding terms of all proofs as one launch ----
    // blind(k, seg): the coefficients over powers_of_gamma_g of proof k's segment seg < nseg (empty: none); their sums land in bl
    template <class Blind>
    int commit(std::vector<StepJob>& jobs, size_t nseg, const Blind& blind, std::vector<zk_g1_projective>& bl, std::vector<char>& has_bl) {
        if (jobs.size() > (size_t)MAX_ROUND_JOBS) return ZK_ERR_STATE;
        ZkHostLap laps{ctx, "marlin_batch.commit."};
        hipStream_t st[MAX_ROUND_JOBS] = {ctx->aux[0], ctx->acc_stream, ctx->aux[1], ctx->stream};
        ZK_TRY(zk_behind_context_stream(ctx, st, 3));                       // the scalars were produced on the context stream
        ZkMsmJob J[MAX_ROUND_JOBS];
        struct Streams {                           // declared after the jobs: every exit drains the streams before the jobs and their events go
            zk_ctx* ctx;
            ~Streams() {
                (void)hipStreamSynchronize(ctx->aux[0]);
                (void)hipStreamSynchronize(ctx->aux[1]);
                (void)hipStreamSynchronize(ctx->aux[2]);
                (void)hipStreamSynchronize(ctx->acc_stream);
                (void)hipStreamSynchronize(ctx->stream);
            }
        } drain{ctx};
        // the blinding terms sum c_i powers_of_gamma_g[i], segments of up to three terms: few of them on the host's helper threads under
        // the device's work, as the single prover computes them; many as one launch on a stream of their own (canonical scalars),
        // enqueued BEFORE the jobs: that stream waits for the context stream, which the shortest job's chain is about to join
        bl.assign(C * nseg, zk_g1_projective{});
        has_bl.assign(C * nseg, 0);
        std::vector<std::vector<HF>> cs;
        std::vector<size_t> where;
        size_t muls = 0;
        for (size_t k = 0; k < C; k++)
            for (size_t sg = 0; sg < nseg; sg++) {
                std::vector<HF> c = blind(k, sg);
                if (c.empty()) continue;
                if (c.size() > 3) return ZK_ERR_STATE;
                muls += c.size();
                cs.push_back(std::move(c));
                where.push_back(k * nseg + sg);
                has_bl[k * nseg + sg] = 1;
            }
        if (where.size() > L.lc_segments) return ZK_ERR_STATE;
        const bool on_host = muls <= HOST_BLIND_MULS;
        uint32_t* got = (uint32_t*)down;
        hipStream_t side = ctx->aux[2];
        ZkTask<void> host_blinds;                                            // (declared after everything its task references)
        if (!where.empty() && on_host) {
            host_blinds = zk_async(ctx, [&] {
                zk_over_ranges(ctx, where.size(), HOST_TASKS, [&](size_t lo, size_t hi) {
                    for (size_t i = lo; i < hi; i++) {
                        zk_g1_projective acc{}, t, u;
                        for (size_t j = 0; j < cs[i].size(); j++) {
                            const zk_fr kk = cs[i][j].abi();
                            zk_g1_mul(&gamma_pts[j], &kk, &t);
                            if (j == 0) { acc = t; continue; }
                            zk_g1_add(&acc, &t, &u);
                            acc = u;
                        }
                        bl[where[i]] = acc;
                    }
                });
            });
        } else if (!where.empty()) {
            ZkLincombPack pack;
            for (size_t i = 0; i < where.size(); i++) {
                uint32_t idx[3] = {0, 1, 2}, k8[24];
                for (size_t j = 0; j < cs[i].size(); j++) cs[i][j].canon_words(k8 + 8 * j);
                if (!pack.add(idx, k8, cs[i].size())) return ZK_ERR_STATE;
            }
            pack.finish();
            const void *d_idx, *d_k, *d_off;
            ZK_TRY(stage.put(pack.point_index.data(), pack.point_index.size() * 4, &d_idx));
            ZK_TRY(stage.put(pack.scalars.data(), pack.scalars.size() * 4, &d_k));
            ZK_TRY(stage.put(pack.seg_off.data(), pack.seg_off.size() * 4, &d_off));
            ZK_TRY(zk_behind_context_stream(ctx, &side, 1));                  // the three uploads
            uint32_t* o_aff = (uint32_t*)L.lc_out.p;
            uint32_t* o_inf = o_aff + 24 * where.size();
            ZK_TRY(zk_g1_lincomb_launch(ctx, powers_gamma_g->dev, 3, (const uint32_t*)d_idx, (const uint32_t*)d_k, (const uint32_t*)d_off, where.size(),
                                        pack.lanes(), o_aff, o_inf, side));
            ZK_HIP(ctx, hipMemcpyAsync(got, o_aff, where.size() * 100, hipMemcpyDeviceToHost, side));
        }
        laps.lap("blinds");
        // longest first: the longest chain starts first, and the context stream (which also carries the blinding terms) takes the shortest
        std::vector<size_t> order(jobs.size());
        for (size_t j = 0; j < jobs.size(); j++) order[j] = j;
        std::stable_sort(order.begin(), order.end(), [&](size_t a, size_t b) { return jobs[a].len > jobs[b].len; });
        for (size_t p = 0; p < order.size(); p++) {
            StepJob& j = jobs[order[p]];
            j.out.assign(j.vectors, zk_g1_projective{});
            if (!j.len) continue;                                            // an empty polynomial commits to the identity
            ZK_TRY(zk_msm_prepare_multi(ctx, &J[p], powers_g, j.off, j.scalars, j.len, j.stride, j.vectors, ZK_SLOT_G16_BATCH + (int)p));
            ZK_TRY(zk_msm_enqueue_sort(ctx, &J[p], st[p], nullptr));
            ZK_TRY(zk_msm_enqueue_accum(ctx, &J[p], st[p]));
            ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[p], st[p]));
        }
        laps.lap("enqueue");
        for (size_t p = 0; p < order.size(); p++)
            if (jobs[order[p]].len) ZK_TRY(zk_msm_finish_multi(ctx, &J[p], jobs[order[p]].out.data()));
        laps.lap("msm_wait");
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));                     // everything of the step on the context stream (the zero test's verdict among it)
        if (host_blinds.valid()) host_blinds.get();
        else if (!where.empty()) {
            ZK_HIP(ctx, hipStreamSynchronize(side));
            for (size_t i = 0; i < where.size(); i++) {
                if (got[24 * where.size() + i]) continue;                    // the identity
                zk_g1_affine a;
                host_aff_to_abi<G1Field>((uint64_t*)&a, aff_load<G1Field>(got + 24 * i));
                zk_g1_from_affine(&a, &bl[where[i]]);
            }
        }
        laps.lap("blinds_wait");
        stage.reset();
        return ZK_OK;
    }
    // Did a zero test of this step fail for some proof of the chunk?  Then the single prover names the proof and the reason.
    int settle(int slot, size_t first_proof) {
        if (!verdicts[slot] || *verdicts[slot] == 0) return ZK_OK;
        if (shared) return settle_shared(slot, first_proof);
        std::vector<uint8_t> buf(zk_marlin_proof_max_size());
        for (size_t k = 0; k < C; k++) {
            size_t len = 0;
            const int rc = zk_marlin_prove(ctx, ix, powers_g, powers_gamma_g, z + k * zs * 32, rngs[k], mask_on_device, buf.data(), buf.size(), &len);
            if (rc == ZK_OK) continue;
            ctx->last_error = "proof " + std::to_string(first_proof + k) + ": " + ctx->last_error;
            return rc;
        }
        ZK_FAIL(ctx, ZK_ERR_STATE, std::string("zk_marlin_prove_batch: ") + check_text[slot] + " failed for the chunk, yet every proof of it passes alone");
    }
    // Over shares nothing is run again (the single prover cannot be re-run silently: it would exchange).  The one test that still reaches
    // here is public -- the inner sum-check, a - b f against v_K -- so every party names the same proof: the first whose remainder is not zero
    int settle_shared(int slot, size_t first_proof) {
        if (slot != 2) ZK_FAIL(ctx, ZK_ERR_STATE, std::string("zk_marlin_prove_shared_batch: ") + check_text[slot] + " was tested on shares");
        const size_t Ks = s.K.size;
        std::vector<uint64_t> rem(C * Ks * 4);
        ZK_TRY(zk_memcpy_d2h(ctx, rem.data(), L.h2_r.p, C * Ks * 32));      // (h2_r's stride is |K|)
        for (size_t k = 0; k < C; k++)
            for (size_t i = 0; i < Ks * 4; i++)
                if (rem[k * Ks * 4 + i]) ZK_FAIL(ctx, ZK_ERR_STATE, "proof " + std::to_string(first_proof + k) + ": " + INNER_NOT_DIVISIBLE);
        ZK_FAIL(ctx, ZK_ERR_STATE, std::string("zk_marlin_prove_shared_batch: ") + check_text[slot] + " failed for the chunk, yet no proof's remainder is non-zero");
    }
    // The first proof of the chunk whose opened value (C elements on the device, the same at every party) is not zero fails the call
    int fail_first_nonzero(const char* opened, size_t first_proof, const char* text) {
        std::vector<uint64_t> v(C * 4);
        ZK_TRY(zk_memcpy_d2h(ctx, v.data(), opened, C * 32));
        for (size_t k = 0; k < C; k++)
            if (v[4 * k] | v[4 * k + 1] | v[4 * k + 2] | v[4 * k + 3]) ZK_FAIL(ctx, ZK_ERR_STATE, "proof " + std::to_string(first_proof + k) + ": " + text);
        return ZK_OK;
    }
    // MarlinKZG10::commit for one round (marlin_pc/mod.rs:172-243) of every proof: blinding polynomials in the reference's rng order,
    // the round's jobs, the round's bytes into each transcript.  Over shares a shared oracle's job covers every lane, the blinding terms
    // (this party's fresh randomness: its MAC lane is the share itself) go to both lanes' points, and the witness-dependent commitments
    // of all proofs are opened in ONE exchange (first_comms.publicize(), lib.rs:180,205,228) before any transcript absorbs them.
    int commit_round(int round, size_t first_proof, int check_slot) {
        const std::vector<Oracle> os = round_oracles(round);
        ZK_TRY(each([&](size_t k) { return P[k].draw_blinds(round, rngs[k]); }));
        std::vector<StepJob> jobs;
        struct Dest { Oracle o; int which; };
        std::vector<Dest> dest, segs;
        for (Oracle o : os) {
            const Vec& p = polys[o];
            jobs.push_back({p.p, p.stride, s.oracle_n(o), 0, vectors_of(o), {}});
            dest.push_back({o, 0});
            if (oracle_bounded(o)) {
                jobs.push_back({p.p, p.stride, s.oracle_n(o), s.max_degree - s.bound(o), vectors_of(o), {}});
                dest.push_back({o, 1});
            }
            if (ORACLES[o].hiding) segs.push_back({o, 0});
            if (ORACLES[o].hiding && oracle_bounded(o)) segs.push_back({o, 1});
        }
        std::vector<zk_g1_projective> bl;
        std::vector<char> has_bl;
        ZK_TRY(commit(jobs, segs.size(), [&](size_t k, size_t sg) { const Blinds& r = P[k].rands[segs[sg].o]; return segs[sg].which ? r.shifted : r.plain; }, bl,
                      has_bl));
        ZK_TRY(settle(check_slot, first_proof));
        // over shares: the open's items, by proof within the kind (marlin_shared_plan.hpp), and the sums that come back
        namespace plan = zk::marlin_plan;
        const plan::Open which_open = round == 1 ? plan::OPEN_ROUND1 : plan::OPEN_ROUND2;
        std::vector<size_t> open_jobs;                                       // the jobs whose points are opened, in wire order
        for (size_t j = 0; shared && j < jobs.size(); j++) if (ORACLES[dest[j].o].shared) open_jobs.push_back(j);
        const size_t per = open_jobs.size();
        ZkSmallItems mine[2], opened;
        if (per) {
            if (per != plan::per_proof(which_open, plan::KIND_G1)) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_shared_batch: a round's open differs from its plan");
            for (int l = 0; l < lanes; l++) mine[l].g1.resize(C * per);
            ZK_TRY(each([&](size_t k) {
                for (size_t i = 0; i < per; i++) {
                    const size_t j = open_jobs[i];
                    for (int l = 0; l < lanes; l++) {
                        zk_g1_projective pt = jobs[j].out[(size_t)l * C + k];
                        for (size_t sg = 0; sg < segs.size(); sg++) {
                            if (segs[sg].o != dest[j].o || segs[sg].which != dest[j].which || !has_bl[k * segs.size() + sg]) continue;
                            zk_g1_projective t;
                            zk_g1_add(&pt, &bl[k * segs.size() + sg], &t);
                            pt = t;
                        }
                        mine[l].g1[plan::slot(which_open, plan::KIND_G1, k, i)] = pt;
                    }
                }
                return (int)ZK_OK;
            }));
            ZK_TRY(open_small(mine, &opened));
        }
        return each([&](size_t k) {
            zk_g1_projective acc[2][N_PROVER];
            for (size_t j = 0; j < jobs.size(); j++) acc[dest[j].which][dest[j].o] = jobs[j].out[k];
            for (size_t sg = 0; sg < segs.size(); sg++) {
                if (!has_bl[k * segs.size() + sg]) continue;
                zk_g1_projective& c = acc[segs[sg].which][segs[sg].o];
                zk_g1_projective t;
                zk_g1_add(&c, &bl[k * segs.size() + sg], &t);
                c = t;
            }
            for (size_t i = 0; i < per; i++) acc[dest[open_jobs[i]].which][dest[open_jobs[i]].o] = opened.g1[plan::slot(which_open, plan::KIND_G1, k, i)];
            std::vector<zk_g1_projective> all;
            for (Oracle o : os) {
                all.push_back(acc[0][o]);
                if (oracle_bounded(o)) all.push_back(acc[1][o]);
            }
            P[k].commitments(round, all);
            return (int)ZK_OK;
        });
    }
    int challenges(int round) { return each([&](size_t k) { P[k].challenges(round, s); return (int)ZK_OK; }); }

    // The transcript seeds: PROTOCOL_NAME | index_vk | public_input (lib.rs:161-164).  Over shares the instance part of an assignment is
    // shared like the rest (from_public: the leader holds it): the chunk's instance parts are gathered into one vector and opened once
    // (one element beside the constant 1 at least: otherwise there is nothing to open, as in the single prover)
    int seed_transcripts() {
        zv = Vec{(char*)z, zs};
        if (lanes > 1) {                                                     // the lanes' assignments side by side: one launch per lane here, one per step from here on
            for (int l = 0; l < lanes; l++) ZK_TRY(zk_b_copy(ctx, L.zin.at((size_t)l * C), L.zin.stride, A.z[l], zs, s.nv, C));
            zv = L.zin;
        }
        std::vector<zk_fr> x(C * s.ni);
        if (!shared || s.ni > 1) {
            ZK_TRY(zk_b_copy(ctx, L.pub.p, L.pub.stride, zv.p, zv.stride, s.ni, shared ? V : C));
            const char* from = L.pub.p;
            if (shared) {
                ZK_TRY(open_vec(L.pub.p, C * L.pub.stride, C * s.ni, L.pub_open.p, L.pub_dx.p));
                from = L.pub_open.p;
            }
            ZK_TRY(zk_memcpy_d2h(ctx, x.data(), from, C * s.ni * 32));
        }
        return each([&](size_t k) { P[k].seed(ix, &x[k * s.ni], s.ni); return (int)ZK_OK; });
    }

    // Round 1 (prover.rs:216-404)
    int round1(size_t first_proof) {
        const size_t n = s.n, md = s.md, host_n = mask_on_device ? 3 : 3 + md + 1;
        {
            std::vector<zk_fr> h(C * host_n);
            std::vector<uint8_t> keys(C * 32);
            ZK_TRY(each([&](size_t k) {
                ZK_TRY(zk_rng_fill_fr(rngs[k], h.data() + k * host_n, host_n));
                return mask_on_device ? zk_rng_fill_bytes(rngs[k], keys.data() + 32 * k, 32) : (int)ZK_OK;
            }));
            if (L.rnd.stride == host_n) ZK_TRY(zk_xfer_h2d(ctx, L.rnd.p, h.data(), C * host_n * 32));
            else {
                // (three scalars per proof: through the step's upload area, then spread to the proofs' strides)
                const void* d;
                ZK_TRY(stage.put(h.data(), C * host_n * 32, &d));
                ZK_TRY(zk_b_copy(ctx, L.rnd.p, L.rnd.stride, d, host_n, host_n, C));
                for (size_t k = 0; k < C; k++) ZK_TRY(zk_fr_random_dev(ctx, keys.data() + 32 * k, 0, L.rnd.at(k) + 96, md + 1));
            }
        }
        // this party's (share of the) prover randomness is its own: its MAC lane is the share itself, a copy beside it, and every step
        // from here on covers the V vectors of its region
        if (lanes > 1) ZK_TRY(zk_b_copy(ctx, L.rnd.at(C), L.rnd.stride, L.rnd.p, L.rnd.stride, 3 + md + 1, C));
        ZK_TRY(zk_b_copy(ctx, L.mask.p, L.mask.stride, L.rnd.p + 96, L.rnd.stride, md + 1, V));
        ZK_TRY(divv(L.mask, md + 1, s.H, L.mask_q, L.mask_r, V));
        ZK_TRY(zk_b_op(ctx, ZK_OP_SUB, L.mask.p, L.mask.stride, L.mask_r.p, L.mask_r.stride, L.mask.p, L.mask.stride, 1, V));      // the sum over H becomes zero
        polys[O_MASK_POLY] = L.mask;
        ZK_TRY(zk_r1cs_matvec_strided(ctx, ix->r1cs, 0, zv.p, zv.stride, V, L.z_a.p, L.z_a.stride, n));
        ZK_TRY(zk_r1cs_matvec_strided(ctx, ix->r1cs, 1, zv.p, zv.stride, V, L.z_b.p, L.z_b.stride, n));
        ZK_TRY(zk_b_copy(ctx, L.xb.p, L.xb.stride, zv.p, zv.stride, s.X.size, V));
        ZK_TRY(ntt(L.xb, s.X, 1, V));
        ZK_TRY(padded(L.x_ev, s.H, L.xb, s.X.size, V));
        ZK_TRY(ntt(L.x_ev, s.H, 0, V));
        ZK_TRY(zk_b_gather(ctx, zv.p, zv.stride, ix->w_idx, n, L.w_ev.p, L.w_ev.stride, V));
        ZK_TRY(zk_b_gather(ctx, L.x_ev.p, L.x_ev.stride, ix->x_idx, n, L.tmp.p, L.tmp.stride, V));
        ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_SUB, L.w_ev.p, L.tmp.p, L.w_ev.p, V * n));
        ZK_TRY(ntt(L.w_ev, s.H, 1, V));                                      // the three interpolations of the round
        ZK_TRY(ntt(L.z_a, s.H, 1, V));
        ZK_TRY(ntt(L.z_b, s.H, 1, V));
        ZK_TRY(zk_b_blind(ctx, L.w_ev.p, L.w_ev.stride, n, L.rnd.p, L.rnd.stride, L.w_h.p, L.w_h.stride, V));
        ZK_TRY(divv(L.w_h, n + 1, s.X, L.wq, L.wr, V));
        // (over shares the remainder is a share of zero: the reference's assert!(remainder.is_zero()) cannot be evaluated locally)
        if (!shared) ZK_TRY(check_later(0, L.wr.p, C * s.X.size));
        ZK_TRY(zk_b_blind(ctx, L.z_a.p, L.z_a.stride, n, L.rnd.p + 32, L.rnd.stride, L.za_p.p, L.za_p.stride, V));
        ZK_TRY(zk_b_blind(ctx, L.z_b.p, L.z_b.stride, n, L.rnd.p + 64, L.rnd.stride, L.zb_p.p, L.zb_p.stride, V));
        polys[O_W] = L.wq; polys[O_Z_A] = L.za_p; polys[O_Z_B] = L.zb_p;
        ZK_TRY(commit_round(1, first_proof, 0));
        return challenges(1);
    }

    // Round 2 (prover.rs:438-565)
    int round2(size_t first_proof) {
        const size_t n = s.n, M = s.MUL.size;
        const HF one = HF::one();
        const FrK *t_alpha, *t_vh, *t_eta;
        ZK_TRY(table(1, [&](size_t k, FrK* r) { r[0] = to_frk(fp_int_to_ext<FrParams>(P[k].alpha.v)); }, &t_alpha));
        ZK_TRY(table(1, [&](size_t k, FrK* r) { r[0] = to_frk(P[k].v_h_alpha.v); }, &t_vh));
        ZK_TRY(table(3, [&](size_t k, FrK* r) { for (int m = 0; m < 3; m++) r[m] = to_frk(P[k].eta[m].v); }, &t_eta));
        ZK_TRY(zk_fr_powers_launch(ctx, s.H.gen.v, one.v, n, L.elems, ZK_FR_EXT));
        ZK_TRY(zk_b_const_minus(ctx, t_alpha, 1, L.elems, n, L.ra.p, L.ra.stride, C));
        ZK_TRY(zk_fr_batch_inverse_dev(ctx, L.ra.p, C * n));
        ZK_TRY(zk_b_scale(ctx, L.ra.p, L.ra.stride, t_vh, 1, L.ra.p, L.ra.stride, n, C));      // r(alpha, X) on H (ahp/mod.rs:352-360)
        {                                                                                       // calculate_t on the transposed matrices
            const void* ps[3]; size_t strides[3], ns[3];
            for (int which = 0; which < 3; which++) {
                ZK_TRY(zk_r1cs_matvec_strided(ctx, ix->r1cs_t, which, L.ra.p, L.ra.stride, C, L.mv[which].p, L.mv[which].stride, n));
                ps[which] = L.mv[which].p; strides[which] = L.mv[which].stride; ns[which] = n;
            }
            ZK_TRY(zk_b_lincomb(ctx, 3, ps, strides, ns, t_eta, 3, L.t_ev.p, L.t_ev.stride, n, C));
        }
        ZK_TRY(ntt(L.t_ev, s.H, 1, C));
        ZK_TRY(ntt(L.ra, s.H, 1, C));
        polys[O_T] = L.t_ev;
        ZK_TRY(padded(L.e_r, s.MUL, L.ra, n, C));
        ZK_TRY(padded(L.e_t, s.MUL, L.t_ev, n, C));
        // z = w v_X + x
        ZK_TRY(zk_b_zero(ctx, L.zp.p, L.zp.stride, n + 1, V));
        ZK_TRY(zk_b_copy(ctx, L.zp.p + 32 * s.X.size, L.zp.stride, L.wq.p, L.wq.stride, s.nwq, V));
        ZK_TRY(zk_b_op(ctx, ZK_OP_SUB, L.zp.p, L.zp.stride, L.wq.p, L.wq.stride, L.zp.p, L.zp.stride, s.nwq, V));
        ZK_TRY(zk_b_op(ctx, ZK_OP_ADD, L.zp.p, L.zp.stride, L.xb.p, L.xb.stride, L.zp.p, L.zp.stride, s.X.size, V));
        ZK_TRY(padded(L.e_a, s.MUL, L.za_p, n + 1, V));
        ZK_TRY(padded(L.e_b, s.MUL, L.zb_p, n + 1, V));
        ZK_TRY(padded(L.e_z, s.MUL, L.zp, n + 1, V));
        for (const Vec* v : {&L.e_r, &L.e_t}) ZK_TRY(ntt(*v, s.MUL, 0, C));
        for (const Vec* v : {&L.e_a, &L.e_b, &L.e_z}) ZK_TRY(ntt(*v, s.MUL, 0, V));
        // z_a z_b: the one product of two witness vectors.  Over shares FieldShare::batch_mul of the chunk's C |MUL| products at once (a
        // region's stride is |MUL|, so a lane's C vectors are contiguous): the two vector opens of ONE proof
        if (!shared) ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_MUL, L.e_a.p, L.e_b.p, L.e_s.p, C * M));
        else {
            const void *xa[2] = {L.e_a.p, lanes > 1 ? L.e_a.at(C) : nullptr}, *yb[2] = {L.e_b.p, lanes > 1 ? L.e_b.at(C) : nullptr};
            void* os[2] = {L.e_s.p, lanes > 1 ? L.e_s.at(C) : nullptr};
            const void *tx[2] = {A.tx[0], A.tx[1]}, *ty[2] = {A.ty[0], A.ty[1]}, *tz[2] = {A.tz[0], A.tz[1]};
            xl.lap("local");
            const int brc = zk_shared_beaver_mul_in(*A.nt, lanes, xa, yb, os, C * M, tx, ty, tz, L.beaver);
            xl.lap("beaver");
            ZK_TRY(brc);
        }
        // (public * own value: local; r(alpha, X) and t are one vector per proof)
        ZK_TRY(zk_b_outer_q1(ctx, L.e_s.p, L.e_a.p, L.e_b.p, L.e_z.p, L.e_r.p, L.e_t.p, M, t_eta, 3, L.e_s.p, M, V, wrap));
        ZK_TRY(ntt(L.e_s, s.MUL, 1, V));                                                       // q_1 (prover.rs:517-541)
        ZK_TRY(zk_b_op(ctx, ZK_OP_ADD, L.e_s.p, L.e_s.stride, L.mask.p, L.mask.stride, L.e_s.p, L.e_s.stride, s.md + 1, V));
        ZK_TRY(divv(L.e_s, M, s.H, L.h1_q, L.h1_r, V));
        // the outer sum-check's zero test (prover.rs:547-550): the constant terms of the count remainders, laid back to back -- over
        // shares opened as one vector, and the verdict read per proof from the opened values right behind that exchange
        ZK_TRY(zk_b_copy(ctx, L.zt.p, L.zt.stride, L.h1_r.p, L.h1_r.stride, 1, V));
        if (!shared) ZK_TRY(check_later(1, L.zt.p, C));
        else {
            ZK_TRY(open_vec(L.zt.p, C * L.zt.stride, C, L.zt_open.p, L.zt_dx.p));
            ZK_TRY(fail_first_nonzero(L.zt_open.p, first_proof, OUTER_NOT_ZERO));
        }
        polys[O_G_1] = Vec{L.h1_r.p + 32, L.h1_r.stride};
        polys[O_H_1] = L.h1_q;
        ZK_TRY(commit_round(2, first_proof, 1));
        return challenges(2);
    }

    // Round 3 (prover.rs:583-716)
    int round3(size_t first_proof) {
        const size_t Ks = s.K.size, Bs = s.B.size;
        const FrK* tab;
        ZK_TRY(table(ZK_B_R3_ROW, [&](size_t k, FrK* r) {
            const Fr eta[3] = {P[k].eta[0].v, P[k].eta[1].v, P[k].eta[2].v};
            zk_b_round3_row(P[k].alpha.v, P[k].beta.v, eta, P[k].vv.v, r);
        }, &tab));
        ZK_TRY(zk_b_round3_denoms(ctx, ix->on_k, Ks, tab, L.den.p, C));
        ZK_TRY(zk_fr_batch_inverse_dev(ctx, L.den.p, C * 3 * Ks));          // zero denominators stay zero, as in ark_ff::batch_inversion
        ZK_TRY(zk_b_round3_f(ctx, ix->on_k, Ks, tab, L.den.p, L.f_ev.p, L.f_ev.stride, C));
        ZK_TRY(zk_b_round3_ab(ctx, ix->on_b, Bs, tab, L.a_ev.p, L.b_ev.p, Bs, C));
        ZK_TRY(ntt(L.f_ev, s.K, 1, C));
        polys[O_G_2] = Vec{L.f_ev.p + 32, L.f_ev.stride};
        ZK_TRY(padded(L.f_on_b, s.B, L.f_ev, Ks, C));                      // a - b f on B itself (degree <= 4|K| - 4 < |B|)
        ZK_TRY(ntt(L.f_on_b, s.B, 0, C));
        ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_MUL, L.b_ev.p, L.f_on_b.p, L.b_ev.p, C * Bs));
        ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_SUB, L.a_ev.p, L.b_ev.p, L.a_ev.p, C * Bs));
        ZK_TRY(ntt(L.a_ev, s.B, 1, C));
        ZK_TRY(divv(L.a_ev, Bs, s.K, L.h2_q, L.h2_r, C));
        ZK_TRY(check_later(2, L.h2_r.p, C * Ks));
        polys[O_H_2] = L.h2_q;
        ZK_TRY(commit_round(3, first_proof, 2));
        return challenges(3);
    }

    Vec poly_of(Oracle o) const {
        if (o < N_PROVER) return polys[o];
        return Vec{(char*)ix->index_polys[o - O_A_ROW].ptr, 0};               // an index oracle: one vector for every proof
    }

    // The evaluations of every proof's query set in one batch (two launches, one copy back), absorbed; the linear combinations over them.
    // Over shares z_b(beta) and g_1(beta) are shares: behind the share lane's values the MAC lane's of every proof, and all of them
    // opened in ONE exchange (`evaluations.publicize()`, lib.rs:296)
    int evaluate() {
        const QueryValue* const want = QUERY_VALUES;
        const size_t W = N_QUERY_VALUES;
        namespace plan = zk::marlin_plan;
        const size_t mac_n = lanes > 1 ? plan::EV_ITEMS : 0, total = C * (W + mac_n);
        std::vector<zk_poly_ref> refs(total);
        std::vector<zk_fr> pts(total), vals(total);
        for (size_t k = 0; k < C; k++) {
            for (size_t i = 0; i < W; i++) {
                const Vec v = poly_of(want[i].o);
                refs[k * W + i] = zk_poly_ref{v.at(k), s.oracle_n(want[i].o)};
                pts[k * W + i] = P[k].point(want[i].at_gamma).abi();
            }
            for (size_t i = 0; i < mac_n; i++) {                             // want[0], want[1]: z_b and g_1 at beta, in the open's order
                refs[C * W + k * mac_n + i] = zk_poly_ref{poly_of(want[i].o).at(C + k), s.oracle_n(want[i].o)};
                pts[C * W + k * mac_n + i] = P[k].beta.abi();
            }
        }
        ZK_TRY(zk_poly_evaluate_batch_dev(ctx, refs.data(), pts.data(), total, vals.data()));
        if (shared) {
            static_assert(QUERY_VALUES[plan::EV_Z_B_BETA].o == O_Z_B && QUERY_VALUES[plan::EV_G_1_BETA].o == O_G_1 && plan::EV_ITEMS == 2,
                          "the evaluations' open lists z_b, g_1 as the query values do");
            ZkSmallItems mine[2], opened;
            for (int l = 0; l < lanes; l++) mine[l].fr.resize(C * plan::EV_ITEMS);
            for (size_t k = 0; k < C; k++)
                for (size_t i = 0; i < (size_t)plan::EV_ITEMS; i++) {
                    mine[0].fr[plan::slot(plan::OPEN_EVALS, plan::KIND_FR, k, i)] = vals[k * W + i];
                    if (lanes > 1) mine[1].fr[plan::slot(plan::OPEN_EVALS, plan::KIND_FR, k, i)] = vals[C * W + k * mac_n + i];
                }
            ZK_TRY(open_small(mine, &opened));
            for (size_t k = 0; k < C; k++)
                for (size_t i = 0; i < (size_t)plan::EV_ITEMS; i++) vals[k * W + i] = opened.fr[plan::slot(plan::OPEN_EVALS, plan::KIND_FR, k, i)];
        }
        return each([&](size_t k) { P[k].evaluated(&vals[k * W], s); return (int)ZK_OK; });
    }

    // open_combinations (marlin/mod.rs:213-306, marlin_pc/mod.rs:245-340): the same oracles enter a combination for every proof, with
    // coefficients of its own; per query point one combination, its witness quotient and the shifted witnesses of the bounded oracles.
    // Over shares the combination at beta holds shared oracles: it runs on the V vectors, a public oracle (t) enters it on the leader
    // only -- which terms and coefficients go into the per-proof table -- as one vector per proof in both lanes (shift(): mac_share = 1
    // there), and the witnesses (and random_v) of all proofs are opened in ONE exchange; the one at gamma is public and computed alike
    // by every party, once per proof.
    int open_combinations() {
        namespace plan = zk::marlin_plan;
        std::vector<StepJob> jobs;
        size_t njobs[2] = {0, 0};
        bool q_shared[2] = {false, false};
        for (int q = 0; q < 2; q++) {
            const OpenPlan& p0 = P[0].plan[q];
            const size_t T = p0.terms.size();
            for (size_t k = 1; k < C; k++) {                                  // (the plan's shape depends on the query set alone)
                const OpenPlan& pk = P[k].plan[q];
                bool same = pk.terms.size() == T && pk.shifted.size() == p0.shifted.size();
                for (size_t t = 0; same && t < T; t++) same = pk.terms[t].first == p0.terms[t].first;
                for (size_t t = 0; same && t < p0.shifted.size(); t++) same = pk.shifted[t].first == p0.shifted[t].first;
                if (!same) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_batch: the proofs' opening plans differ");
            }
            if (p0.shifted.size() > 1) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_batch: more than one shifted witness at a query point");
            for (auto& t : p0.terms) q_shared[q] = q_shared[q] || (shared && ORACLES[t.first].shared);
            if (shared && q_shared[q] != (q == 0)) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_shared_batch: shared oracles are opened at beta and only there");
            const size_t cnt = q_shared[q] ? V : C, proofs = q_shared[q] ? wrap : 0;
            std::vector<const void*> ps; std::vector<size_t> strides, ns, use;      // use: the terms that enter at this party
            unsigned per_proof = 0;
            size_t cn = 0;
            for (size_t t = 0; t < T; t++) {
                const Oracle o = p0.terms[t].first;
                cn = std::max(cn, s.oracle_n(o));
                if (q_shared[q] && !ORACLES[o].shared && !leader) continue;     // a public oracle in a shared combination: the leader's
                const Vec v = poly_of(o);
                if (q_shared[q] && !ORACLES[o].shared) per_proof |= 1u << use.size();
                ps.push_back(v.p); strides.push_back(v.stride); ns.push_back(s.oracle_n(o)); use.push_back(t);
            }
            const size_t U = use.size();
            if (cn > s.cn[q] || cn < 2 || !U) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_batch: a combination outgrows its buffer");
            const FrK* coef;
            ZK_TRY(table(U, [&](size_t k, FrK* r) { for (size_t t = 0; t < U; t++) r[t] = to_frk(P[k].plan[q].terms[use[t]].second.v); }, &coef));
            ZK_TRY(zk_b_lincomb(ctx, (int)U, ps.data(), strides.data(), ns.data(), coef, U, L.comb[q].p, L.comb[q].stride, cn, cnt, proofs, per_proof));
            std::vector<Fr> zpt(cnt);
            for (size_t v = 0; v < cnt; v++) zpt[v] = P[v % C].point(q).v;
            ZK_TRY(zk_poly_divide_by_linear_strided(ctx, L.comb[q].p, L.comb[q].stride, cn, zpt.data(), cnt, L.quo[q].p, L.quo[q].stride, L.spans.p, &stage));
            jobs.push_back({L.quo[q].p, L.quo[q].stride, cn - 1, 0, cnt, {}});
            njobs[q] = 1;
            for (auto& sh : p0.shifted) {
                if (q_shared[q] != (shared && ORACLES[sh.first].shared))
                    ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_shared_batch: a shifted witness of another kind than its combination");
                const Vec v = poly_of(sh.first);
                const size_t pn = s.oracle_n(sh.first);
                if (pn < 2) continue;
                ZK_TRY(zk_poly_divide_by_linear_strided(ctx, v.p, v.stride, pn, zpt.data(), cnt, L.sw[q].p, L.sw[q].stride, L.spans.p, &stage));
                const FrK* c1;
                ZK_TRY(table(1, [&](size_t k, FrK* r) { r[0] = to_frk(P[k].plan[q].shifted[0].second.v); }, &c1));
                ZK_TRY(zk_b_scale(ctx, L.sw[q].p, L.sw[q].stride, c1, 1, L.sw[q].p, L.sw[q].stride, pn - 1, cnt, proofs));
                jobs.push_back({L.sw[q].p, L.sw[q].stride, pn - 1, s.max_degree - s.bound(sh.first), cnt, {}});
                njobs[q]++;
            }
        }
        // the blinding witnesses: per proof and query point the plain and the shifted one
        std::vector<OpenBlinds> ob(C * 2);
        ZK_TRY(each([&](size_t k) {
            for (int q = 0; q < 2; q++) ob[2 * k + q] = P[k].blinds_at(q);
            return (int)ZK_OK;
        }));
        // (at gamma nothing is hiding: g_2, h_2 and the index are committed without blinds)
        for (size_t k = 0; k < C; k++)
            if (ob[2 * k + 1].hiding || !ob[2 * k + 1].shifted_w.empty()) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_batch: a blinding witness at gamma");
        std::vector<zk_g1_projective> bl;
        std::vector<char> has_bl;
        ZK_TRY(commit(jobs, 2, [&](size_t k, size_t sg) { return sg == 0 ? ob[2 * k].plain_w : ob[2 * k].shifted_w; }, bl, has_bl));
        // lane l's witness of proof k at query point q (own randomness: the same on the MAC lane)
        auto witness = [&](size_t k, int q, int l) {
            const size_t j = q ? njobs[0] : 0, at = (size_t)l * C + k;
            zk_g1_projective w = jobs[j].out[at];
            for (size_t i = 1; i < njobs[q]; i++) { zk_g1_projective t; zk_g1_add(&w, &jobs[j + i].out[at], &t); w = t; }
            for (size_t sg = 0; sg < 2 && q == 0; sg++) {
                if (!has_bl[2 * k + sg]) continue;
                zk_g1_projective t;
                zk_g1_add(&w, &bl[2 * k + sg], &t);
                w = t;
            }
            return w;
        };
        ZkSmallItems mine[2], opened;
        if (q_shared[0]) {                                                   // the witness (and random_v) of a shared combination: opened
            static_assert(plan::WI_ITEMS == 1, "one witness and at most one random_v per proof");
            for (int l = 0; l < lanes; l++) mine[l].g1.resize(C);
            ZK_TRY(each([&](size_t k) { for (int l = 0; l < lanes; l++) mine[l].g1[plan::slot(plan::OPEN_WITNESS, plan::KIND_G1, k, plan::WI_WITNESS_BETA)] = witness(k, 0, l); return (int)ZK_OK; }));
            // random_v: C scalars at the plan's slots -- or none at all, if no proof's combination is hiding (the blinding polynomials of
            // the opened oracles cancel: negligible).  A chunk in which only some are would not fit the open's layout.
            for (size_t k = 1; k < C; k++)
                if (P[k].has_rv[0] != P[0].has_rv[0]) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_marlin_prove_shared_batch: random_v at beta for some proofs of a chunk only");
            for (int l = 0; l < lanes && P[0].has_rv[0]; l++) {
                mine[l].fr.resize(C);
                for (size_t k = 0; k < C; k++) mine[l].fr[plan::slot(plan::OPEN_WITNESS, plan::KIND_FR, k, plan::WI_RANDOM_V)] = P[k].rvs[0].abi();
            }
            ZK_TRY(open_small(mine, &opened));
        }
        return each([&](size_t k) {
            zk_g1_projective wits[2];
            for (int q = 0; q < 2; q++) {
                if (!q_shared[q]) { wits[q] = witness(k, q, 0); continue; }
                wits[q] = opened.g1[plan::slot(plan::OPEN_WITNESS, plan::KIND_G1, k, plan::WI_WITNESS_BETA)];
                if (P[k].has_rv[q]) P[k].rvs[q] = HF::from_abi(opened.fr[plan::slot(plan::OPEN_WITNESS, plan::KIND_FR, k, plan::WI_RANDOM_V)]);
            }
            P[k].witnesses(wits);
            return (int)ZK_OK;
        });
    }

    int run(size_t first_proof) {
        ZkHostLap laps{ctx, "marlin_batch."};
        ZK_TRY(seed_transcripts());
        laps.lap("seed");
        ZK_TRY(round1(first_proof));
        laps.lap("round1");
        ZK_TRY(round2(first_proof));
        laps.lap("round2");
        ZK_TRY(round3(first_proof));
        laps.lap("round3");
        ZK_TRY(evaluate());
        laps.lap("evaluate");
        ZK_TRY(open_combinations());
        laps.lap("open");
        return each([&](size_t k) {
            if (!P[k].write(A.proofs_out + k * A.slot, A.slot, &A.proof_lens[k])) { P[k].err = "zk_marlin_prove_batch: output slot too small"; return (int)ZK_ERR_ARG; }
            return (int)ZK_OK;
        });
    }
};
const char* const Chunk::check_text[3] = {"the divisibility of w by v_X", "the outer sum-check", "the inner sum-check"};

// device bytes of one chunk's MSM scratch: per job in flight its sort (~16 bytes per digit) and its bucket sums (groth16_batch.hip's rule)
size_t msm_bytes(const zk_bases* tab, size_t len, size_t chunk) {
    const size_t W = tab->pre ? (255 + tab->c_pre - 1) / tab->c_pre : 32;
    const size_t buckets = tab->pre ? ((size_t)1 << (tab->c_pre - 1)) : W * std::max<size_t>(len, 16);
    return (size_t)MAX_ROUND_JOBS * chunk * (len * W * 16 + buckets * 48 * 4 * 2);
}

// What the three entry points hand over (lanes [0] = share / plain, [1] = MAC share under SPDZ)
struct BatchArgs {
    const char* name;                             // the entry point, for error texts
    const zk_marlin_index* ix;
    const zk_bases *powers_g, *powers_gamma_g;
    size_t count;
    const void* z[2]; size_t z_stride;
    zk_rng* const* rngs; int mask_on_device;
    int lanes; bool shared;
    const void *tx[2], *ty[2], *tz[2];
    const zk_net_vtable* net;
    uint8_t* proofs_out; size_t slot; size_t* proof_lens; uint64_t* bytes_sent;
};

// The argument checks every entry point makes before it forwards a single proof or plans a batch
int check_args(zk_ctx* ctx, const BatchArgs& a) {
    const std::string name = a.name;
    if (!ctx || !a.ix || !a.powers_g || !a.powers_gamma_g || !a.rngs || !a.proofs_out || !a.proof_lens) return ZK_ERR_ARG;
    for (int l = 0; l < a.lanes; l++) if (!a.z[l]) ZK_FAIL(ctx, ZK_ERR_ARG, name + ": an assignment lane is missing");
    if (a.count == 0) ZK_FAIL(ctx, ZK_ERR_ARG, name + ": count must be at least 1");
    for (size_t k = 0; k < a.count; k++) if (!a.rngs[k]) ZK_FAIL(ctx, ZK_ERR_ARG, name + ": a generator is missing");
    if (a.slot < zk_marlin_proof_max_size()) ZK_FAIL(ctx, ZK_ERR_ARG, name + ": slot smaller than zk_marlin_proof_max_size()");
    if (a.z_stride < a.ix->num_variables) ZK_FAIL(ctx, ZK_ERR_ARG, name + ": z_stride is shorter than the padded assignment");
    if (a.shared && zk_shared_triple_given(a.lanes, a.tx, a.ty, a.tz) < 0) ZK_FAIL(ctx, ZK_ERR_ARG, name + ": give a whole Beaver triple (every lane) or none");
    return ZK_OK;
}

// count >= 2 proofs in chunks.  Plain: the chunk is this device's own.  Over shares every party must cut the same chunks (an exchange
// carries a chunk's items), so the local bound -- 0: not one proof fits, or this party failed before the exchange -- is published in one
// exchange of 8 bytes and all take the minimum (marlin_shared_plan.hpp); the proofs are collected in memory of the call and copied out
// behind the last chunk.  Parties that share ONE device each size their bound against the same free memory: the call's own buffers are
// allocated before the exchange, so a party that loses that race publishes 0, but the MSM jobs' sort scratch (the context's arena, grown at
// the first job) is not -- several parties on one device should cap the chunk with ZK_MARLIN_BATCH_CHUNK.
int batch_impl(zk_ctx* ctx, const BatchArgs& a) {
    const zk_marlin_index* ix = a.ix;
    const zk_bases *powers_g = a.powers_g, *powers_gamma_g = a.powers_gamma_g;
    const size_t count = a.count;
    const int lanes = a.lanes;
    ZkHostLap laps{ctx, "marlin_batch."};
    ZK_TRY(check_index_and_srs(ctx, ix, powers_g, powers_gamma_g));
    const Shape s(ix, powers_g);
    ZK_TRY(check_sizes(ctx, s.max_degree, s.n, s.K.size, s.B.size));
    // the chunk: what one multi-vector job takes (a shared oracle's covers every lane), what fits the device, what the environment asks for
    size_t chunk = count, longest = 0;
    auto job_of = [&](size_t len) { if (len) chunk = std::min(chunk, zk_msm_multi_chunk(powers_g, len) / (size_t)lanes); longest = std::max(longest, len); };
    for (int o = 0; o < N_PROVER; o++) job_of(s.oracle_n((Oracle)o));
    for (int q = 0; q < 2; q++) job_of(s.cn[q] - 1);
    if (s.n > 2) job_of(s.n - 2);
    if (s.K.size > 2) job_of(s.K.size - 2);
    Layout L;
    std::string nomem;
    ZkCallMem mem{ctx}, up{ctx};
    ZkStage stage;
    stage.ctx = ctx;
    char* down = nullptr;
    zk_g1_projective gamma_pts[3];
    // This party's bound and, for it, everything the call allocates -- BEFORE the plan's exchange: behind that exchange a party must
    // not fail alone (its peers would wait for it in the next one), so what can fail locally fails here and is published as a bound of 0.
    // The agreed chunk is at most this one, and its Layout lies inside the same allocation.
    auto local_plan = [&]() -> int {
        if (chunk == 0) { nomem = std::string(a.name) + ": the lanes of one proof exceed what a multi-vector job takes"; return ZK_OK; }
        size_t free_b = 0, total_b = 0;
        ZK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
        auto need = [&](size_t c) { return (double)L.place(nullptr, c, s, lanes, a.shared) + (double)msm_bytes(powers_g, longest, (size_t)lanes * c); };
        while (chunk > 1 && need(chunk) > (double)(free_b / 10 * 9)) chunk = (chunk + 1) / 2;
        if (need(chunk) > (double)(free_b / 10 * 9)) {
            chunk = 0;
            nomem = "marlin batch: the working set of one proof (" + std::to_string((unsigned long long)(need(1) / 1048576.0)) +
                    " MiB) does not fit the free device memory (" + std::to_string(free_b >> 20) + " MiB)";
            return ZK_OK;
        }
        if (const char* e = getenv("ZK_MARLIN_BATCH_CHUNK")) {              // read at every call: the seam between chunks at small shapes
            const long v = atol(e);
            if (v > 0) chunk = std::min(chunk, (size_t)v);
        }
        zk_presort_free(ctx);                                                // (a Groth16 proof's jobs enqueued ahead use the streams this call waits on)
        ZK_TRY(zk_prover_streams(ctx, 3));
        zk_g1_affine g[3];
        ZK_TRY(zk_bases_download_g1(ctx, powers_gamma_g, 0, 3, g));
        for (int i = 0; i < 3; i++) zk_g1_from_affine(&g[i], &gamma_pts[i]);
        ZK_HIP(ctx, hipMalloc(&mem.p, L.place(nullptr, chunk, s, lanes, a.shared)));
        // what a step uploads: the job arrays of four divisions (one job per vector), the constants' tables, the blinding terms' lanes
        stage.cap = chunk * ((size_t)lanes * 4 * zk_poly_divlin_job_bytes() + 64 * sizeof(FrK) + 16 * 36 + 1024) + 65536;
        ZK_HIP(ctx, hipMalloc(&up.p, stage.cap));
        stage.dev = (char*)up.p;
        ZK_TRY(zk_pinned(ctx, {ZK_PIN_MARLIN_BATCH, 0}, stage.cap, (void**)&stage.host));
        return zk_pinned(ctx, {ZK_PIN_MARLIN_BATCH, 1}, chunk * 3 * 100 + 256, (void**)&down);
    };
    const int local_rc = local_plan();
    if (local_rc != ZK_OK) chunk = 0;
    ZkSharedNet nt{ctx, a.net};
    if (a.shared) {                                                          // one plan for all parties, before any device work
        const uint64_t mine = chunk;
        std::vector<uint8_t> all;
        const std::string local_text = ctx->last_error;
        const int grc = nt.gather((const uint8_t*)&mine, 8, all);
        if (local_rc != ZK_OK) { ctx->last_error = local_text; return local_rc; }      // (published as 0: the peers return ZK_ERR_NOMEM)
        ZK_TRY(grc);
        std::vector<uint64_t> bounds((size_t)nt.parties());
        memcpy(bounds.data(), all.data(), bounds.size() * 8);
        chunk = (size_t)zk::marlin_plan::agreed_bound(bounds.data(), bounds.size());
        if (chunk == 0 && nomem.empty()) nomem = std::string(a.name) + ": a peer's device does not hold the working set of one proof";
    }
    ZK_TRY(local_rc);
    if (chunk == 0) ZK_FAIL(ctx, ZK_ERR_NOMEM, nomem);
    L.place((char*)mem.p, chunk, s, lanes, a.shared);
    laps.lap("plan+alloc");
    // over shares nothing is written before the last chunk has passed its MAC checks and zero tests
    std::vector<uint8_t> held(a.shared ? count * a.slot : 0);
    std::vector<size_t> held_lens(a.shared ? count : 0);
    uint8_t* const out = a.shared ? held.data() : a.proofs_out;
    size_t* const lens = a.shared ? held_lens.data() : a.proof_lens;
    const size_t M = s.MUL.size;
    for (size_t i = 0; i < zk::marlin_plan::chunks_of(count, chunk); i++) {
        const zk::marlin_plan::Span sp = zk::marlin_plan::chunk_at(count, chunk, i);
        const size_t k0 = sp.first;
        stage.reset();
        ChunkArgs ca{};
        for (int l = 0; l < lanes; l++) {
            ca.z[l] = (const char*)a.z[l] + k0 * a.z_stride * 32;
            ca.tx[l] = a.tx[l] ? (const char*)a.tx[l] + k0 * M * 32 : nullptr;      // proof k's triple at k |MUL|
            ca.ty[l] = a.ty[l] ? (const char*)a.ty[l] + k0 * M * 32 : nullptr;
            ca.tz[l] = a.tz[l] ? (const char*)a.tz[l] + k0 * M * 32 : nullptr;
        }
        ca.zs = a.z_stride; ca.rngs = a.rngs + k0; ca.mask_on_device = a.mask_on_device; ca.lanes = lanes; ca.shared = a.shared; ca.nt = &nt;
        ca.proofs_out = out + k0 * a.slot; ca.slot = a.slot; ca.proof_lens = lens + k0;
        Chunk c(ctx, ix, powers_g, powers_gamma_g, s, L, stage, down, sp.size, ca, gamma_pts);
        const int rc = c.run(k0);
        (void)hipStreamSynchronize(ctx->stream);                             // every exit leaves nothing behind on the stream it enqueued on
        ZK_TRY(rc);
    }
    if (a.shared) {
        for (size_t k = 0; k < count; k++) memcpy(a.proofs_out + k * a.slot, held.data() + k * a.slot, held_lens[k]);
        memcpy(a.proof_lens, held_lens.data(), count * sizeof(size_t));
    }
    if (a.bytes_sent) *a.bytes_sent = nt.bytes;
    return ZK_OK;
}

}  // namespace

extern "C" int zk_marlin_prove_batch(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g, size_t count,
                                     const void* z_dev, size_t z_stride, zk_rng* const* rngs, int mask_on_device, uint8_t* proofs_out, size_t slot,
                                     size_t* proof_lens) {
    ZK_API_BEGIN(ctx)
    if (!z_dev) return ZK_ERR_ARG;
    const BatchArgs a{"zk_marlin_prove_batch", ix, powers_g, powers_gamma_g, count, {z_dev, nullptr}, z_stride, rngs, mask_on_device, 1, false,
                      {nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}, nullptr, proofs_out, slot, proof_lens, nullptr};
    ZK_TRY(check_args(ctx, a));
    if (count == 1) return zk_marlin_prove(ctx, ix, powers_g, powers_gamma_g, z_dev, rngs[0], mask_on_device, proofs_out, slot, proof_lens);
    return batch_impl(ctx, a);
    ZK_API_END
}

// MpcMarlin::prove (src/marlin.rs:56) for count shared assignments of one index, over additive shares: every argument as
// zk_marlin_prove_shared's, per proof (z_k at z + 32 k z_stride, rngs[k], proof k's triple at k |MUL| elements of tx / ty / tz)
extern "C" int zk_marlin_prove_shared_batch(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g,
                                            size_t count, const void* z_share_dev, size_t z_stride, zk_rng* const* rngs, int mask_on_device,
                                            const void* tx, const void* ty, const void* tz, const zk_net_vtable* net, uint8_t* proofs_out, size_t slot,
                                            size_t* proof_lens, uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    if (!z_share_dev) return ZK_ERR_ARG;
    const BatchArgs a{"zk_marlin_prove_shared_batch", ix, powers_g, powers_gamma_g, count, {z_share_dev, nullptr}, z_stride, rngs, mask_on_device, 1, true,
                      {tx, nullptr}, {ty, nullptr}, {tz, nullptr}, net, proofs_out, slot, proof_lens, bytes_sent};
    ZK_TRY(check_args(ctx, a));
    if (count == 1)
        return zk_marlin_prove_shared(ctx, ix, powers_g, powers_gamma_g, z_share_dev, rngs[0], mask_on_device, tx, ty, tz, net, proofs_out, slot, proof_lens,
                                      bytes_sent);
    return batch_impl(ctx, a);
    ZK_API_END
}

// ... over SPDZ shares: lanes [0] = share, [1] = MAC share
extern "C" int zk_marlin_prove_shared_spdz_batch(zk_ctx* ctx, const zk_marlin_index* ix, const zk_bases* powers_g, const zk_bases* powers_gamma_g,
                                                 size_t count, const void* const z_lanes_dev[2], size_t z_stride, zk_rng* const* rngs, int mask_on_device,
                                                 const void* const tx_lanes[2], const void* const ty_lanes[2], const void* const tz_lanes[2],
                                                 const zk_net_vtable* net, uint8_t* proofs_out, size_t slot, size_t* proof_lens, uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    if (!z_lanes_dev) return ZK_ERR_ARG;
    const void* none[2] = {nullptr, nullptr};
    const void* const* txs = tx_lanes ? tx_lanes : none;
    const void* const* tys = ty_lanes ? ty_lanes : none;
    const void* const* tzs = tz_lanes ? tz_lanes : none;
    const BatchArgs a{"zk_marlin_prove_shared_spdz_batch", ix, powers_g, powers_gamma_g, count, {z_lanes_dev[0], z_lanes_dev[1]}, z_stride, rngs,
                      mask_on_device, 2, true, {txs[0], txs[1]}, {tys[0], tys[1]}, {tzs[0], tzs[1]}, net, proofs_out, slot, proof_lens, bytes_sent};
    ZK_TRY(check_args(ctx, a));
    if (count == 1)
        return zk_marlin_prove_shared_spdz(ctx, ix, powers_g, powers_gamma_g, z_lanes_dev, rngs[0], mask_on_device, tx_lanes, ty_lanes, tz_lanes, net,
                                           proofs_out, slot, proof_lens, bytes_sent);
    return batch_impl(ctx, a);
    ZK_API_END
}
