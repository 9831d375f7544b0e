// groth16_pipeline.hip -- the five MSMs of create_proof (src/groth16.rs:106,110,137,148,160) as a pipeline over three streams, with
// the next proof's front and the collaborative prover's presorts enqueued ahead of their proofs (ZkG16Flight).
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include <chrono>

using namespace zk;
using Stage = ZkG16Flight::Stage;

static void drain_streams(zk_ctx* ctx) {                  // the three streams of the pipeline (zk_prover_streams has run)
    (void)hipStreamSynchronize(ctx->aux[0]);
    (void)hipStreamSynchronize(ctx->acc_stream);
    (void)hipStreamSynchronize(ctx->stream);
}

void zk_presort_free(zk_ctx* ctx) {
    if (!ctx || !ctx->flight) return;
    const std::unique_ptr<ZkG16Flight> f(std::exchange(ctx->flight, nullptr));
    if (f->beyond_sort_z()) drain_streams(ctx);                     // its kernels run on the accumulate and context streams as well
    else (void)hipStreamSynchronize(ctx->aux[0]);           // its kernels write the job's scratch slot
}

int zk_next_z_drop(zk_ctx* ctx, bool drain) {
    if (drain) {                    // its front reads the slot it was uploaded to; the upload may still run
        zk_presort_free(ctx);
        if (ctx->copy_stream) ZK_HIP(ctx, hipStreamSynchronize(ctx->copy_stream));
    }
    ctx->next.clear();
    return ZK_OK;
}

int zk_groth16_key_matches(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r) {
    const size_t n = r->ni + r->nw;
    if (!pk->a || !pk->b_g1 || !pk->b_g2 || !pk->l || !pk->h || r->ni < 1 || pk->a->n != n || pk->b_g1->n != n || pk->b_g2->n != n ||
        pk->l->n != r->nw)
        ZK_FAIL(ctx, ZK_ERR_ARG, "groth16: proving key does not match the constraint system");
    return ZK_OK;
}

int zk_prover_streams(zk_ctx* ctx, size_t k) {
    while (ctx->aux.size() < k) {
        hipStream_t st;
        ZK_HIP(ctx, zk_stream_create(&st, true));
        ctx->aux.push_back(st);
    }
    // (the accumulate stream is an ordinary stream: a CU mask that withholds compute units for the other streams costs what it
    // frees -- round 3, ZK_ACC_CU_RESERVE)
    if (!ctx->acc_stream) ZK_HIP(ctx, zk_stream_create(&ctx->acc_stream, false));
    return ZK_OK;
}

int zk_behind_context_stream(zk_ctx* ctx, const hipStream_t* waiters, int count) {
    ZK_HIP(ctx, zk_streams_follow(ctx->stream, waiters, count));
    return ZK_OK;
}

namespace {

// What every entry point here does first: a pending flight that is not this call's goes, the key is checked, the helper streams are
// there, and the first `waiters` of {sort stream, accumulate stream} wait for the context stream, where z was produced.
int enter(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, bool keep_flight, int waiters) {
    if (!keep_flight) zk_presort_free(ctx);
    ZK_TRY(zk_groth16_key_matches(ctx, pk, r));
    ZK_TRY(zk_prover_streams(ctx, 1));
    const hipStream_t w[2] = {ctx->aux[0], ctx->acc_stream};
    return zk_behind_context_stream(ctx, w, waiters);
}

// The five MSMs of create_proof as a pipeline over THREE streams (the runtime maps streams onto ~3
// usable hardware queues; a fourth stream lands on an occupied queue and serialises behind it):
//   main       : witness map, then the sort of the H job (its scalars come out of the witness map)
//   sort/reduce: sort of the z-dependent jobs first (B-in-G2 / A / B-in-G1 share one sort: same scalars
//                z[1..]), then, as the accumulate kernels complete, each job's reduce phase in job order
//   accum      : the five accumulate kernels back to back, B-in-G2 first (longest reduce), H last;
//                the first one is gated on the witness map, which would otherwise be starved 15x beside it
// The plan: the stream of the z jobs' sort and of each job's accumulate kernel and reduce chain (accumulate order = job order)
struct StreamPlan { hipStream_t sort_z, accum[5], reduce[5]; };
enum PlanRow { PLAN_LARGE, PLAN_SMALL, PLAN_GROUPED, PLAN_FRONT };
StreamPlan stream_plan(zk_ctx* ctx, PlanRow row) {
    const hipStream_t main = ctx->stream, sort = ctx->aux[0], acc = ctx->acc_stream;      // (the sort stream carries reduce chains as well)
    switch (row) {
    case PLAN_LARGE:
        // B-in-G2's reduce chain (the long one) stays on the sort stream; the four G1 reduces go to the main stream, idle by
        // then, so that each runs right behind its own accumulate kernel instead of queueing behind the G2 chain (that
        // queueing left 4 x 0.7 ms of reduces after the last accumulate).
        // The last two reduce chains alternate between the two streams (the sort stream is idle again once the G2 chain is
        // through): on one stream the last job's chain queued behind its predecessor's, which was still waiting for slots
        // beside the last accumulate kernel, and ~0.6 ms of it ran after the GPU had otherwise gone idle.
        return {sort, {acc, acc, acc, acc, acc}, {sort, main, sort, main, sort}};
    case PLAN_SMALL:
        // A job of up to 2^16 terms occupies a tenth of the chip for the length of its longest bucket (~0.3 ms): five of them one
        // behind the other on the accumulate stream are most of a small proof.  There every job's accumulate kernel goes on the stream
        // of its own reduce chain instead (G2 alone on the accumulate stream, the G1 jobs alternating between the sort stream and the
        // context stream): the kernels overlap, the chain follows its kernel without an event.  (Ordering against the next proof's
        // front does not lean on the accumulate stream: that front waits for every job's reduce_done / accum_done event.)
        return {sort, {acc, sort, main, sort, main}, {acc, sort, main, sort, main}};
    case PLAN_GROUPED:
        // ... and where the four G1 jobs qualify (tables of window multiples with the same bucket count: every key of >= 256 points)
        // they are ONE accumulate launch and one launch per level of the reduce chain, on the sort stream (round 5: two jobs per stream,
        // one behind the other, were 2 x (0.26 + 0.2) ms of a 1.2 ms proof at 2^10)
        return {sort, {acc, sort, sort, sort, sort}, {acc, sort, sort, sort, sort}};
    default:
        // The front of the NEXT proof: its z-sort goes on the accumulate stream (in order behind the five accumulate kernels, the
        // readers of this proof's sort products); a whole chain (a grouped proof's front) on the streams this proof's own chains are
        // on, so stream order keeps every reader of a scratch buffer in front of its next writer.
        return {acc, {acc, sort, sort, sort, sort}, {acc, sort, sort, sort, sort}};
    }
}

// The stages: each advances at[] and passes over a job that is already there.  First the z jobs: one sort of z[1..], job 0's
// (first_only: no more than that), which a presort or a front may have enqueued already; the others borrow it.
int sort_z(zk_ctx* ctx, ZkG16Flight& F, const ZkG16Jobs& T, hipStream_t st, bool first_only = false) {
    if (F.at[first_only ? 0 : 1] >= Stage::SORTED) return ZK_OK;
    ZK_TRY(T.sort_z(ctx, F.J, st, ZK_SLOT_G16, 0, F.at[0] >= Stage::SORTED, first_only ? 1 : 4));
    F.at[0] = Stage::SORTED;
    if (!first_only) { F.at[1] = F.at[2] = Stage::SORTED; if (T.l_shared) F.at[3] = Stage::SORTED; }
    return ZK_OK;
}

// The witness map into F.h (the caller brings h: none) and H's prepare and sort, on the context stream.  The first accumulate
// kernel is gated on the witness map, which would otherwise be starved beside it (un-gating it: within the noise of consecutive
// runs, round 3): wm_done, which the accumulate stream waits for.
// `behind`: F is the front of the proof after `behind`.  Its witness map and H-sort queue behind that proof's H-sort and reduce
// chains on the context stream; the H-sort rewrites slot 5 and also waits for the last accumulate kernel, the reader of the H
// job's sort products, and for H's own chain (k_fold reads ctr / heavy there), which may be on the other stream.  The gate is left
// to the call that takes the front over: it finds at[4] == SORTED.  (prepare only fills the job in on the host: it enqueues nothing.)
int witness_map_and_h(zk_ctx* ctx, ZkG16Flight& F, const ZkG16Jobs& T, ZkPhaseTimer* tm, const ZkG16Flight* behind) {
    if (F.at[4] == Stage::NONE) {
        if (F.h) {
            if (tm) tm->begin("witness_map");
            const int rc = T.witness_map(ctx, F.z, F.h);
            if (tm) tm->end();
            ZK_TRY(rc);
        }
        ZK_TRY(T.prepare(ctx, 4, &F.J[4], ZK_SLOT_G16));
        ZK_HIP(ctx, F.wm_done.record(ctx->stream));
        if (behind) {
            ZK_HIP(ctx, behind->J[4].accumulated_at.order(ctx->stream));
            ZK_HIP(ctx, behind->J[4].reduced_at.order(ctx->stream));
        }
        ZK_TRY(zk_msm_enqueue_sort(ctx, &F.J[4], ctx->stream, nullptr));
        F.at[4] = Stage::SORTED;
    }
    if (!behind) ZK_HIP(ctx, hipStreamWaitEvent(ctx->acc_stream, F.wm_done.get(), 0));
    return ZK_OK;
}

// L's sort after the witness map where L does not share the z jobs' (it is not needed before the fourth accumulate kernel)
int sort_l_late(zk_ctx* ctx, ZkG16Flight& F, hipStream_t st) {
    if (F.at[3] >= Stage::SORTED) return ZK_OK;
    if (F.wm_done) ZK_HIP(ctx, hipStreamWaitEvent(st, F.wm_done.get(), 0));
    ZK_TRY(zk_msm_enqueue_sort(ctx, &F.J[3], st, nullptr));
    F.at[3] = Stage::SORTED;
    return ZK_OK;
}

// The first `njobs` jobs that are at `from` go one stage on -- SORTED: the accumulate kernels, ACCUMULATED: the reduce chains --
// each on its stream of the plan, the G1 jobs of a group as one launch (one per level of the chain).
int advance(zk_ctx* ctx, ZkG16Flight& F, const StreamPlan& P, Stage from, int njobs = 5) {
    const bool acc = from == Stage::SORTED;
    const hipStream_t* st = acc ? P.accum : P.reduce;
    for (int k = 0; k < njobs; k++) {
        if (F.at[k] != from || (F.grouped && k != 0)) continue;
        ZK_TRY(acc ? zk_msm_enqueue_accum(ctx, &F.J[k], st[k]) : zk_msm_enqueue_reduce(ctx, &F.J[k], st[k]));
        F.at[k] = Stage(from + 1);
    }
    if (F.grouped && F.at[1] == from) {
        ZK_TRY(acc ? zk_msm_enqueue_accum_group(ctx, F.g1, 4, st[1]) : zk_msm_enqueue_reduce_group(ctx, F.g1, 4, st[1]));
        F.at[1] = F.at[2] = F.at[3] = F.at[4] = Stage(from + 1);
    }
    return ZK_OK;
}
int accumulate(zk_ctx* ctx, ZkG16Flight& F, const StreamPlan& P) { return advance(ctx, F, P, Stage::SORTED); }
int reduce(zk_ctx* ctx, ZkG16Flight& F, const StreamPlan& P, int njobs = 5) { return advance(ctx, F, P, Stage::ACCUMULATED, njobs); }

// finish in completion order: the host-side Horner of an early job overlaps the GPU work of the later ones
int collect(zk_ctx* ctx, ZkG16Flight& F, zk_g1_projective out_g1[4], zk_g2_projective* out_g2, const std::function<void()>& after_abc) {
    void* outs[5] = {out_g2, &out_g1[2], &out_g1[3], &out_g1[1], &out_g1[0]};
    if (F.grouped) {
        // the four G1 jobs of a group become ready together: their host halves side by side, B in G2's on this thread
        ZkTask<int> g1fin = zk_async(ctx, [&] { (void)hipSetDevice(ctx->device); return zk_msm_finish_many(ctx, F.g1, outs + 1, 4); });
        const int rc0 = zk_msm_finish(ctx, &F.J[0], outs[0]), rc1 = g1fin.get();
        if (rc0 == ZK_OK && rc1 == ZK_OK && after_abc) after_abc();
        return rc0 != ZK_OK ? rc0 : rc1;
    }
    for (int k = 0; k < 5; k++) {
        ZK_TRY(zk_msm_finish(ctx, &F.J[k], outs[k]));
        if (k == 2 && after_abc) after_abc();      // A, B1, B2 are in: the caller's host work overlaps the rest
    }
    return ZK_OK;
}

// The caller announced the next assignment (zk_groth16_hint_next_dev): enqueue that proof's front N now, behind the kernels of this
// proof C.  Its z-sort also waits for the reduce chains, whose fold kernels read the segment tables.  No buffer is doubled: stream
// order and these events keep every reader in front of the next writer.
int enqueue_front(zk_ctx* ctx, const ZkG16Flight& C, ZkG16Flight& N, const ZkG16Jobs& T) {
    const StreamPlan P = stream_plan(ctx, PLAN_FRONT);
    if (N.z == ctx->next.dev && ctx->next.ready) {      // announced from the host: its upload runs on the copy stream
        ZK_HIP(ctx, hipStreamWaitEvent(P.sort_z, ctx->next.ready.get(), 0));
        ZK_HIP(ctx, hipStreamWaitEvent(ctx->stream, ctx->next.ready.get(), 0));
    }
    // a reduce chain reads its job's segment tables (k_fold: ctr / heavy live in the sort scratch of the job's slot).  The
    // next proof's z-sort rewrites slot 1, whose products the four z jobs share: it waits for THEIR chains (not for the H
    // job's, the last one: the z-sort is meant to run under that tail); the next H-sort rewrites slot 5 and waits for the
    // H job's chain.
    for (int k = 0; k < 4; k++) ZK_HIP(ctx, C.J[k].reduced_at.order(P.sort_z));
    ZK_TRY(sort_z(ctx, N, T, P.sort_z, true));
    ZK_TRY(witness_map_and_h(ctx, N, T, nullptr, &C));
    // A SMALL proof (its four G1 jobs one group): the next proof's whole device chain goes out as well -- accumulate launches and
    // reduce chains of all five jobs.  The device then runs from one proof's chain into the next while the host
    // finishes the first (Horner chains, the tail's scalar multiplications, the caller's next call: ~0.2 ms during which the
    // chip used to wait).  The results land in the other pair of pinned buffers: this proof's are still to be read.
    if (!C.grouped || !ctx->chain_fronts) return ZK_OK;
    const uint32_t par = (uint32_t)(ctx->front_parity ^= 1);
    N.J[0].pin = {ZK_PIN_FRONT, par};
    N.J[1].pin = {ZK_PIN_FRONT_GROUP, par};                    // (the group's results travel in its first job's buffer)
    ZK_TRY(sort_z(ctx, N, T, P.sort_z));                       // (l_shared here: the z-sort above serves all four)
    if (!(N.grouped = zk_msm_group_ok(N.g1, 4))) return ZK_OK; // (not for one key: whether its G1 jobs group is the key's property)
    ZK_TRY(accumulate(ctx, N, P));
    return reduce(ctx, N, P);
}

}  // namespace

int zk_groth16_run_msms(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* z, const void* h_in, void* h_scratch,
                        zk_g1_projective out_g1[4], zk_g2_projective* out_g2, const std::function<void()>& after_abc) {
    const auto t_enter = std::chrono::steady_clock::now();
    // Part of this proof may already be under way (ZkG16Flight): take it over.  A front's witness map wrote h_scratch; a begun set
    // can only be taken over whole, by the call that brings h; a sort of z[1..] alone serves any call.  Anything else is drained
    // and dropped: its jobs own the scratch slots this call is about to use.
    ZkG16Flight* const pend = ctx->flight;
    const bool mine = pend && pend->pk == pk && pend->z == z && pend->J[0].n == r->ni + r->nw - 1 &&
                      (pend->h ? !h_in && pend->r == r && pend->h == h_scratch : !pend->beyond_sort_z() || (h_in && pend->r == r));
    // z was produced on the context stream.  (With a front that stream already carries this proof's witness map and H-sort:
    // waiting for it here would hold the sort stream -- and the G2 reduce chain on it -- until the H-sort is through.)
    ZK_TRY(enter(ctx, pk, r, mine, mine && pend->h ? 0 : 1));
    const ZkG16Jobs T(pk, r, z, h_in ? h_in : h_scratch, true, h_in != nullptr);      // (a caller's h is the quotient: over h_query)
    ZkG16Flight own(pk, r, z, nullptr);
    const std::unique_ptr<ZkG16Flight> taken(mine ? std::exchange(ctx->flight, nullptr) : nullptr);
    ZkG16Flight& F = mine ? *taken : own;
    F.h = h_in ? nullptr : h_scratch;
    const bool small = F.at[1] < Stage::ACCUMULATED && T.D <= ((size_t)1 << 16);      // (a begun set, a chained front: enqueued further already)
    StreamPlan P = stream_plan(ctx, small ? PLAN_SMALL : PLAN_LARGE);
    ZkPhaseTimer tm(ctx);
    int rc = sort_z(ctx, F, T, P.sort_z);
    if (rc == ZK_OK) rc = witness_map_and_h(ctx, F, T, &tm, nullptr);
    if (rc == ZK_OK) rc = sort_l_late(ctx, F, P.sort_z);
    if (rc == ZK_OK && small && (F.grouped = zk_msm_group_ok(F.g1, 4))) P = stream_plan(ctx, PLAN_GROUPED);
    if (rc == ZK_OK) rc = accumulate(ctx, F, P);
    if (rc == ZK_OK) rc = reduce(ctx, F, P);
    const void* const zn = std::exchange(ctx->next.z, nullptr);
    if (rc == ZK_OK && zn && !h_in && T.l_shared) {
        std::unique_ptr<ZkG16Flight> N(new ZkG16Flight(pk, r, zn, h_scratch));
        rc = enqueue_front(ctx, F, *N, ZkG16Jobs(pk, r, zn, h_scratch));
        if (rc == ZK_OK) ctx->flight = N.release();
        else drain_streams(ctx);                           // part of it is in flight: let it drain before its jobs go
    }
    if (ctx->profiling) {                          // host time from the call to the last enqueue (a small proof's device chain starts late by it)
        auto& t = ctx->timers["host.enqueue"];
        t.ms += std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t_enter).count();
        t.count += 1;
    }
    if (rc == ZK_OK) rc = collect(ctx, F, out_g1, out_g2, after_abc);
    if (!ctx->flight) drain_streams(ctx);                  // (with a front in flight the streams carry the next proof's kernels)
    tm.resolve();
    return rc;
}

// The next zk_groth16_prove_dev on this context will be for `z_next_dev` (same key, same constraint system): the proof
// in between enqueues that proof's front (z-sort, witness map, H-sort) behind its own kernels.  Pass NULL to withdraw.
extern "C" int zk_groth16_hint_next_dev(zk_ctx* ctx, const void* z_next_dev) {
    ZK_API_BEGIN(ctx)
    if (!ctx) return ZK_ERR_ARG;
    ctx->next.z = z_next_dev;
    return ZK_OK;
    ZK_API_END
}

// Whether the front of an announced SMALL proof also carries that proof's accumulate launches and reduce chains (default: yes --
// one context proving a queue goes from 0.54 to 0.43 ms per proof at 2^10).  Several contexts sharing one GPU do better without:
// every context then keeps the hardware queues filled with its own next chain and they serialise (four contexts, eight queues:
// 0.27 ms per proof without, 0.47 with; profiles/r5_small_throughput.jsonl).
extern "C" int zk_groth16_chain_fronts(zk_ctx* ctx, int on) {
    ZK_API_BEGIN(ctx)
    if (!ctx) return ZK_ERR_ARG;
    ctx->chain_fronts = on != 0;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_groth16_msms_presort_dev(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* z) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !z) return ZK_ERR_ARG;
    ZK_TRY(enter(ctx, pk, r, false, 1));
    std::unique_ptr<ZkG16Flight> F(new ZkG16Flight(pk, r, z, nullptr));
    ZK_TRY(sort_z(ctx, *F, ZkG16Jobs(pk, r, z, nullptr, true, true), ctx->aux[0], true));
    ctx->flight = F.release();
    return ZK_OK;
    ZK_API_END
}

// The four MSMs over z -- B in G2, A, B in G1, L -- enqueued to the end (sort, accumulate, reduce); returns at once.
// zk_groth16_msms_dev(ctx, pk, r, z, h, ...) with the same pk / r / z then only adds the H job and collects the five results.
// For the collaborative prover (mpc.py::create_proof_shared): the Beaver open of the witness map's product and the second
// half of the witness map run under accumulate kernels that do not need h.  The context stream stays free for the caller's
// own kernels.
extern "C" int zk_groth16_msms_begin_dev(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* z) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !z) return ZK_ERR_ARG;
    ZK_TRY(enter(ctx, pk, r, false, 2));
    std::unique_ptr<ZkG16Flight> F(new ZkG16Flight(pk, r, z, nullptr));
    const ZkG16Jobs T(pk, r, z, nullptr, true, true);      // (zk_groth16_msms_dev brings the quotient)
    const StreamPlan P = stream_plan(ctx, PLAN_LARGE);
    int rc = sort_z(ctx, *F, T, P.sort_z);
    if (rc == ZK_OK) rc = sort_l_late(ctx, *F, P.sort_z);
    if (rc == ZK_OK) rc = accumulate(ctx, *F, P);          // (jobs 0..3: H is not sorted)
    // only the G2 job's reduce chain here (sort stream); the G1 chains are enqueued by zk_groth16_msms_dev, which spreads them over
    // the context stream (the caller's own kernels are through by then) and the sort stream as the one-call form does
    if (rc == ZK_OK) rc = reduce(ctx, *F, P, 1);
    if (rc == ZK_OK) ctx->flight = F.release();
    else drain_streams(ctx);                                     // whatever was enqueued drains before the jobs (and their events) go
    return rc;
    ZK_API_END
}

extern "C" int zk_groth16_msms_dev(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* z, const void* h,
                                   zk_g1_projective out_g1[4], zk_g2_projective* out_g2) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !z || !h || !out_g1 || !out_g2) return ZK_ERR_ARG;
    return zk_groth16_run_msms(ctx, pk, r, z, h, nullptr, out_g1, out_g2);
    ZK_API_END
}

