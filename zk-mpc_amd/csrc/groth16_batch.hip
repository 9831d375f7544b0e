// groth16_batch.hip -- count proofs of ONE key and ONE constraint system in one call (create_proof, src/groth16.rs:68-183, for
// count assignments).  Every proof is the bytes zk_groth16_prove_dev returns for the same (z, r, s).
//
// A small proof leaves the device idle: its MSMs are chains of launch and dependency latencies.  Here the five MSMs of all the
// proofs are five multi-vector jobs (msm.hip: zk_msm_prepare_multi): one sort, one accumulate launch and one reduce chain each, over
// count bucket spaces of one table -- the launches of one proof, whatever count is.  The z jobs (A, B in G1, L over l_pad, B in G2)
// share one sort of the count z vectors where their window widths agree, as zk_groth16_run_msms shares it for one proof.
// The witness maps of all proofs are one batched witness map (r1cs.hip: zk_groth16_witness_map_batch: mat-vec, strided transforms
// and vector operations over count D elements), on the context stream beside the z sort.  So the call's launches do not grow with
// count until a job reaches the multi-job limits (zk_msm_multi_chunk): then the MSMs run in chunks of proofs.
// Host tails (ZkProofTail would start six pool tasks per proof): the terms that need no MSM result (delta r, delta s, delta_2 s)
// as at most 8 tasks while the device works -- beside the at most 8 threads of a multi job's Horner chains -- and the rest as at
// most 16 tasks over contiguous ranges of proofs once the sums are in.
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include <algorithm>

using namespace zk;

namespace {

constexpr size_t TAIL_TASKS = 16, PRE_TASKS = 8;

// cnt proofs: z = their assignments (m elements each), h = their cnt quotients of D elements once front() has run on the context
// stream (the first chunk enqueues the batched witness map there, beside its z sort); pre_ready() returns once the pre terms of tails[0..cnt) are complete
int prove_chunk(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t cnt, const char* z, const char* h, const std::function<int()>& front,
                const std::function<void()>& pre_ready, ZkTail* tails, uint8_t* proofs) {
    const ZkG16Jobs T(pk, r, z, h);
    hipStream_t s_sort = ctx->aux[0], s_acc = ctx->acc_stream;
    ZK_TRY(zk_behind_context_stream(ctx, &s_sort, 1));               // z was produced on the context stream
    ZkMsmJob J[5];                                                   // 0: B in G2, 1: A, 2: B in G1, 3: L, 4: H
    struct Streams {                       // declared after the jobs: every exit drains the streams before the jobs and their events go
        zk_ctx* ctx;
        ~Streams() {
            (void)hipStreamSynchronize(ctx->aux[0]);
            (void)hipStreamSynchronize(ctx->acc_stream);
            (void)hipStreamSynchronize(ctx->stream);
        }
    } drain{ctx};
    ZK_TRY(T.sort_z(ctx, J, s_sort, ZK_SLOT_G16_BATCH, cnt));
    if (!T.l_shared) ZK_TRY(zk_msm_enqueue_sort(ctx, &J[3], s_sort, nullptr));
    ZK_TRY(front());                                                 // the witness map on the context stream, beside the z sort
    ZK_TRY(T.prepare(ctx, 4, &J[4], ZK_SLOT_G16_BATCH, cnt));
    ZK_TRY(zk_msm_enqueue_sort(ctx, &J[4], ctx->stream, nullptr));
    // B in G2 (the long reduce chain) on the accumulate stream, the z jobs of G1 on the sort stream, H on the context stream
    ZK_TRY(zk_msm_enqueue_accum(ctx, &J[0], s_acc));
    ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[0], s_acc));
    for (int j = 1; j <= 3; j++) {
        ZK_TRY(zk_msm_enqueue_accum(ctx, &J[j], s_sort));
        ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[j], s_sort));
    }
    ZK_TRY(zk_msm_enqueue_accum(ctx, &J[4], ctx->stream));
    ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[4], ctx->stream));
    std::vector<zk_g1_projective> a(cnt), b1(cnt), l(cnt), hs(cnt);
    std::vector<zk_g2_projective> b2(cnt);
    ZK_TRY(zk_msm_finish_multi(ctx, &J[0], b2.data()));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[1], a.data()));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[2], b1.data()));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[3], l.data()));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[4], hs.data()));
    pre_ready();
    zk_over_ranges(ctx, cnt, TAIL_TASKS, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++) {
            zk_tail_chain_a(pk, &tails[k], a[k]);
            zk_tail_chain_b(pk, &tails[k], b1[k]);
            zk_tail_chain_2(pk, &tails[k], b2[k]);
            zk_tail_finish(tails[k], hs[k], l[k], proofs + k * 192, T.l_const);
        }
    });
    return ZK_OK;
}

// The key against the system, the proofs per MSM chunk, and the device memory: the assignments (count m elements: the caller's,
// or the host form's upload) and the witness map's 6 count D elements (a | b | c and the transforms' scratch), plus one chunk's
// MSM scratch, against 90 % of the free memory.
int batch_plan(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, size_t* chunk_out) {
    ZK_TRY(zk_groth16_key_matches(ctx, pk, r));
    const size_t m = r->ni + r->nw, D = (size_t)1 << r->log_d;
    size_t bytes;
    zk_g16_batch_chunk(pk, r, count, false, chunk_out, &bytes);
    return zk_g16_batch_fits(ctx, count, (double)(m + 6 * D) * 32.0, bytes);
}

int run_batch(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, size_t chunk, const void* z_dev, const zk_fr* r_,
              const zk_fr* s_, uint8_t* proofs_out) {
    const size_t m = r->ni + r->nw, D = (size_t)1 << r->log_d;
    // an announced next assignment (zk_groth16_hint_next_dev, zk_groth16_prove_queued) is drained and dropped: its front reads
    // scratch this call does not own, and the next single proof is not the one it was announced for
    ZK_TRY(zk_next_z_drop(ctx, true));
    if (count == 1) return zk_groth16_prove_dev(ctx, pk, r, z_dev, r_, s_, proofs_out);
    ZK_TRY(zk_prover_streams(ctx, 1));
    ZkCallMem wm{ctx};
    ZK_HIP(ctx, hipMalloc(&wm.p, count * 6 * D * 32));
    std::vector<ZkTail> tails(count);
    // the terms of the tails that need no MSM result, beside the device work (prove_chunk waits for them before its tails)
    ZkTask<void> pre_task = zk_async(ctx, [&] {
        zk_over_ranges(ctx, count, PRE_TASKS, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                zk_tail_begin(&r_[k], &s_[k], &tails[k]);
                zk_tail_pre_a(pk, &tails[k]);
                zk_tail_pre_b(pk, &tails[k]);
                zk_tail_pre_2(pk, &tails[k]);
            }
        });
    });
    const std::function<void()> pre_ready = [&] { if (pre_task.valid()) pre_task.get(); };
    const std::function<int()> wmap = [&] { return ZkG16Jobs(pk, r, nullptr, nullptr).witness_map_batch(ctx, count, z_dev, wm.p); };
    const std::function<int()> none = [] { return ZK_OK; };
    int rc = ZK_OK;
    for (size_t k0 = 0; k0 < count && rc == ZK_OK; k0 += chunk)
        rc = prove_chunk(ctx, pk, r, std::min(chunk, count - k0), (const char*)z_dev + k0 * m * 32, (const char*)wm.p + k0 * D * 32,
                         k0 == 0 ? wmap : none, pre_ready, tails.data() + k0, proofs_out + k0 * 192);
    return rc;
}

}  // namespace

void zk_g16_batch_chunk(const zk_pk* pk, const zk_r1cs* r, size_t count, bool quotient_given, size_t* chunk_out, size_t* chunk_bytes) {
    const ZkG16Jobs T(pk, r, nullptr, nullptr, true, quotient_given);
    size_t chunk = count;
    for (const ZkG16Jobs::Job& j : T.j) chunk = std::min(chunk, zk_msm_multi_chunk(j.tab, j.n));
    // per job its sort (sorted entries, keys, values and the segment tables: ~16 bytes per digit) and its bucket sums (with room
    // for split buckets)
    size_t bytes = 0;
    for (const ZkG16Jobs::Job& j : T.j) {
        const size_t W = j.tab->pre ? (255 + j.tab->c_pre - 1) / j.tab->c_pre : 32;
        const size_t XW = j.tab->group == 1 ? 48 : 96;
        const size_t buckets = j.tab->pre ? ((size_t)1 << (j.tab->c_pre - 1)) : W * std::max<size_t>(j.n, 16);
        bytes += chunk * (j.n * W * 16 + buckets * XW * 4 * 2);
    }
    *chunk_out = chunk;
    *chunk_bytes = bytes;
}

int zk_g16_batch_fits(zk_ctx* ctx, size_t count, double per_proof, size_t chunk_bytes) {
    size_t free_b = 0, total_b = 0;
    ZK_HIP(ctx, hipMemGetInfo(&free_b, &total_b));
    const double need = (double)count * per_proof + (double)chunk_bytes;
    if (need > (double)(free_b / 10 * 9))
        ZK_FAIL(ctx, ZK_ERR_NOMEM, "groth16 batch: the working set of " + std::to_string(count) + " proofs (" +
                                       std::to_string((unsigned long long)(need / 1048576.0)) + " MiB) does not fit the free device memory (" +
                                       std::to_string(free_b >> 20) + " MiB)");
    return ZK_OK;
}

extern "C" int zk_groth16_prove_batch_dev(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, const void* z_dev, const zk_fr* r_,
                                          const zk_fr* s_, uint8_t* proofs_out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !count || !z_dev || !r_ || !s_ || !proofs_out) return ZK_ERR_ARG;
    size_t chunk;
    ZK_TRY(batch_plan(ctx, pk, r, count, &chunk));
    return run_batch(ctx, pk, r, count, chunk, z_dev, r_, s_, proofs_out);
    ZK_API_END
}

extern "C" int zk_groth16_prove_batch(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, const zk_fr* z_host, const zk_fr* r_,
                                      const zk_fr* s_, uint8_t* proofs_out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !count || !z_host || !r_ || !s_ || !proofs_out) return ZK_ERR_ARG;
    size_t chunk;
    ZK_TRY(batch_plan(ctx, pk, r, count, &chunk));                 // before the upload: the assignments are part of the working set
    const size_t m = r->ni + r->nw;
    ZkCallMem z{ctx};
    ZK_HIP(ctx, hipMalloc(&z.p, count * m * 32));
    ZK_TRY(zk_xfer_h2d(ctx, z.p, z_host, count * m * 32, zk_host_is_pinned(z_host)));
    return run_batch(ctx, pk, r, count, chunk, z.p, r_, s_, proofs_out);
    ZK_API_END
}
