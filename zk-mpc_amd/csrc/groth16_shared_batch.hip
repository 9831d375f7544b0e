// groth16_shared_batch.hip -- count collaborative proofs of ONE key and ONE constraint system in one call: proof k is the bytes
// zk_groth16_prove_shared[_spdz] returns for (z_k, r_k, s_k, triple_k), and the call makes the exchanges of ONE such proof.
//
// What a collaborative proof costs that a faster device does not shrink is its round trips: two vector opens (the Beaver product of
// the witness map) and two small opens (the fused open, the reveal of C), each followed by a MAC exchange under SPDZ.  Here the
// count products are one Beaver product over count D elements and the small opens carry the items of all proofs, ordered by proof
// within each kind: the exchanges do not grow with count, their payload does.  The device work is the plain batch's
// (groth16_batch.hip): the witness map's halves over count vectors with launches that do not grow with count, the five MSMs as
// multi-vector jobs -- the z jobs of the share lane enqueued before the Beaver exchange, so that they run under it -- in chunks of
// proofs where count exceeds what one multi job takes.  The exchanges are not cut into chunks.  The host algebra of each proof is
// groth16_shared_int.hpp's, over ranges of proofs on the helper threads.
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "groth16_shared_int.hpp"
#include "sharednet.hpp"
#include <algorithm>

using namespace zk;

namespace {

namespace sh = zk_shared;
constexpr size_t TAIL_TASKS = 16, PRE_TASKS = 8;

// every exit drains the pipeline's streams before the jobs (declared before it) and their events go
struct Streams {
    zk_ctx* ctx;
    ~Streams() {
        (void)hipStreamSynchronize(ctx->aux[0]);
        (void)hipStreamSynchronize(ctx->acc_stream);
        (void)hipStreamSynchronize(ctx->stream);
    }
};

// The sums of one lane: proof k's at [k]
struct LaneSums {
    std::vector<zk_g1_projective> a, b1, l, h;
    std::vector<zk_g2_projective> b2;
    explicit LaneSums(size_t count) : a(count), b1(count), l(count), h(count), b2(count) {}
};

// The four z jobs of cnt proofs (J[0..3]: B in G2, A, B in G1, L) to the end: B in G2 (the long reduce chain) on the accumulate stream,
// the G1 jobs on the sort stream.  The context stream stays free: the witness map's halves and the exchanges' kernels go there.
int begin_z_jobs(zk_ctx* ctx, const ZkG16Jobs& T, size_t cnt, ZkMsmJob* J) {
    hipStream_t s_sort = ctx->aux[0], s_acc = ctx->acc_stream;
    ZK_TRY(zk_behind_context_stream(ctx, &s_sort, 1));               // z was produced on the context stream
    ZK_TRY(T.sort_z(ctx, J, s_sort, ZK_SLOT_G16_BATCH, cnt));
    if (!T.l_shared) ZK_TRY(zk_msm_enqueue_sort(ctx, &J[3], s_sort, nullptr));
    ZK_TRY(zk_msm_enqueue_accum(ctx, &J[0], s_acc));
    ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[0], s_acc));
    for (int j = 1; j <= 3; j++) {
        ZK_TRY(zk_msm_enqueue_accum(ctx, &J[j], s_sort));
        ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[j], s_sort));
    }
    return ZK_OK;
}

// ... and the H job over their quotients (on the context stream, behind the post half), then the five sums into out[k0..k0 + cnt)
int finish_jobs(zk_ctx* ctx, const ZkG16Jobs& T, size_t cnt, ZkMsmJob* J, LaneSums* out, size_t k0) {
    ZK_TRY(T.prepare(ctx, 4, &J[4], ZK_SLOT_G16_BATCH, cnt));
    ZK_TRY(zk_msm_enqueue_sort(ctx, &J[4], ctx->stream, nullptr));
    ZK_TRY(zk_msm_enqueue_accum(ctx, &J[4], ctx->stream));
    ZK_TRY(zk_msm_enqueue_reduce(ctx, &J[4], ctx->stream));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[0], out->b2.data() + k0));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[1], out->a.data() + k0));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[2], out->b1.data() + k0));
    ZK_TRY(zk_msm_finish_multi(ctx, &J[3], out->l.data() + k0));
    return zk_msm_finish_multi(ctx, &J[4], out->h.data() + k0);
}

// The key against the system, the proofs per MSM chunk, and the device memory -- the plain batch's rule (groth16_batch.hip:
// batch_plan) with the lanes and the Beaver product: per proof the assignments (lanes m elements: the caller's), the witness map's
// a | b | c per lane and its 3 D elements of transform scratch, and the product's 2 lanes + 3 vectors; plus one chunk's MSM scratch
double per_proof_bytes(const zk_r1cs* r, int lanes) {
    const size_t m = r->ni + r->nw, D = (size_t)1 << r->log_d;
    return ((double)lanes * (double)m + (double)(3 * lanes + 3 + 2 * lanes + 3) * (double)D) * 32.0;
}
int shared_batch_plan(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, int lanes, size_t* chunk) {
    ZK_TRY(zk_groth16_key_matches(ctx, pk, r));
    size_t bytes;
    zk_g16_batch_chunk(pk, r, count, true, chunk, &bytes);
    return zk_g16_batch_fits(ctx, count, per_proof_bytes(r, lanes), bytes);
}

// z / rs / ss / tx..tz by lane: count assignments of m elements, count scalars, count D triple elements (or none)
template <int LANES>
int prove_shared_batch_impl(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, size_t chunk, const void* const z[2],
                            const zk_fr* const rs[2], const zk_fr* const ss[2], const void* const tx[2], const void* const ty[2],
                            const void* const tz[2], const zk_net_vtable* net, uint8_t* proofs_out, uint64_t* bytes_sent) {
    const bool leader = ctx->party_id == 0;
    const size_t m = r->ni + r->nw, D = (size_t)1 << r->log_d, total = count * D;
    // an announced next assignment is drained and dropped, as the plain batch does (run_batch)
    ZK_TRY(zk_next_z_drop(ctx, true));
    ZK_TRY(zk_prover_streams(ctx, 1));
    ZkSharedNet nt{ctx, net};
    // the call's buffers: a | b | c of each lane, the transforms' scratch, the Beaver product's scratch
    ZkCallMem mem{ctx};
    ZK_HIP(ctx, hipMalloc(&mem.p, (size_t)(3 * LANES + 3 + 2 * LANES + 3) * total * 32));
    char *a[2] = {nullptr, nullptr}, *c[2] = {nullptr, nullptr};
    for (int l = 0; l < LANES; l++) { a[l] = (char*)mem.p + (size_t)l * 3 * total * 32; c[l] = a[l] + 2 * total * 32; }
    char* tmp = (char*)mem.p + (size_t)LANES * 3 * total * 32;
    char* bv = tmp + 3 * total * 32;
    const sh::Key K(pk, leader);
    std::vector<sh::Proof> P(count);
    // public point x shared scalar for every proof and lane, beside the device work
    ZkTask<void> pre_task = zk_async(ctx, [&] {
        zk_over_ranges(ctx, count, PRE_TASKS, [&](size_t lo, size_t hi) {
            for (size_t k = lo; k < hi; k++) {
                const zk_fr *rk[2] = {rs[0] + k, LANES == 2 ? rs[1] + k : nullptr}, *sk[2] = {ss[0] + k, LANES == 2 ? ss[1] + k : nullptr};
                sh::begin(LANES, rk, sk, &P[k]);
                for (int l = 0; l < LANES; l++) { sh::pre_r_g1(K, &P[k], l); sh::pre_s_g1(K, &P[k], l); sh::pre_s_g2(K, &P[k], l); }
            }
        });
    });
    std::vector<LaneSums> sums;
    for (int l = 0; l < LANES; l++) sums.emplace_back(count);
    {
        // the share lane's first chunk: its z jobs go out before the exchange and run under it
        const size_t cnt0 = std::min(chunk, count);
        const ZkG16Jobs T0(pk, r, z[0], a[0], true, true);
        ZkMsmJob J0[5];
        Streams drain{ctx};
        ZK_TRY(begin_z_jobs(ctx, T0, cnt0, J0));
        for (int l = 0; l < LANES; l++) ZK_TRY(zk_groth16_witness_map_batch_pre(ctx, r, count, z[l], a[l], tmp));      // local: linear in the shares
        // FieldShare::batch_mul of all count D products at once (share/field.rs:97-129): two vector opens per CALL
        {
            const void* xa[2] = {a[0], a[1]};
            const void* yb[2] = {a[0] + total * 32, LANES == 2 ? a[1] + total * 32 : nullptr};
            void* oa[2] = {a[0], a[1]};
            ZK_TRY(zk_shared_beaver_mul_in(nt, LANES, xa, yb, oa, total, tx, ty, tz, bv));
        }
        for (int l = 0; l < LANES; l++) ZK_TRY(zk_groth16_witness_map_batch_post(ctx, r, count, a[l], c[l], tmp));     // h shares in a[l]
        ZK_TRY(finish_jobs(ctx, T0, cnt0, J0, &sums[0], 0));
    }
    // the other chunks of the share lane and the MAC lane's MSMs (spdz.rs:482-488: twice), five jobs each
    for (int l = 0; l < LANES; l++)
        for (size_t k0 = l == 0 ? chunk : 0; k0 < count; k0 += chunk) {
            const size_t cnt = std::min(chunk, count - k0);
            const ZkG16Jobs T(pk, r, (const char*)z[l] + k0 * m * 32, a[l] + k0 * D * 32, true, true);
            ZkMsmJob J[5];
            Streams drain{ctx};
            ZK_TRY(begin_z_jobs(ctx, T, cnt, J));
            ZK_TRY(finish_jobs(ctx, T, cnt, J, &sums[l], k0));
        }
    pre_task.get();
    // calculate_coeff and the items of the fused open, ordered by proof within each kind
    ZkSmallItems fused[2], opened;
    for (int l = 0; l < LANES; l++) { fused[l].fr.resize(2 * count); fused[l].g1.resize(3 * count); fused[l].g2.resize(count); }
    zk_over_ranges(ctx, count, TAIL_TASKS, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++)
            for (int l = 0; l < LANES; l++) {
                const zk_g1_projective m1[4] = {sums[l].h[k], sums[l].l[k], sums[l].a[k], sums[l].b1[k]};
                sh::coeff(K, &P[k], l, m1, sums[l].b2[k]);
                sh::fused_items(K, P[k], l, &fused[l].fr[2 * k], &fused[l].g1[3 * k], &fused[l].g2[k]);
            }
    });
    ZK_TRY(zk_shared_open_small(nt, LANES, fused, &opened));
    // the three GroupShare::scale tails and the C share of every proof
    ZkSmallItems c_share[2], c_opened;
    for (int l = 0; l < LANES; l++) c_share[l].g1.resize(count);
    zk_over_ranges(ctx, count, TAIL_TASKS, [&](size_t lo, size_t hi) {
        for (size_t k = lo; k < hi; k++) {
            const zk_fr &oy_s = opened.fr[2 * k], &oy_r = opened.fr[2 * k + 1];
            const sh::SX1 p0 = sh::scale_finish(leader, sh::point1(opened.g1[3 * k]), oy_s);           // r s delta
            const sh::SX1 p1 = sh::scale_finish(leader, sh::point1(opened.g1[3 * k + 1]), oy_s);       // s A
            const sh::SX1 p2 = sh::scale_finish(leader, sh::point1(opened.g1[3 * k + 2]), oy_r);       // r B1
            const sh::SX1 t = sh::scaled_sum(p0, p1, p2);
            for (int l = 0; l < LANES; l++) c_share[l].g1[k] = sh::c_share(P[k], l, t);
        }
    });
    ZK_TRY(zk_shared_open_small(nt, LANES, c_share, &c_opened));      // Proof::reveal of every C
    // (nothing was written so far: a failed MAC check leaves proofs_out as it was)
    for (size_t k = 0; k < count; k++) sh::write_proof(opened.g1[3 * k + 1], opened.g2[k], c_opened.g1[k], proofs_out + k * 192);
    if (bytes_sent) *bytes_sent = nt.bytes;
    return ZK_OK;
}

}  // namespace

extern "C" int zk_groth16_prove_shared_batch(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, const void* z_share,
                                             const zk_fr* r_share, const zk_fr* s_share, const void* tx, const void* ty, const void* tz,
                                             const zk_net_vtable* net, uint8_t* proofs_out, uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !count || !z_share || !r_share || !s_share || !proofs_out) return ZK_ERR_ARG;
    const void* z[2] = {z_share, nullptr};
    const zk_fr *rs[2] = {r_share, nullptr}, *ss[2] = {s_share, nullptr};
    const void *txs[2] = {tx, nullptr}, *tys[2] = {ty, nullptr}, *tzs[2] = {tz, nullptr};
    if (zk_shared_triple_given(1, txs, tys, tzs) < 0) ZK_FAIL(ctx, ZK_ERR_ARG, "prove_shared_batch: give a whole Beaver triple or none");
    size_t chunk;
    ZK_TRY(shared_batch_plan(ctx, pk, r, count, 1, &chunk));
    if (count == 1) {
        ZK_TRY(zk_next_z_drop(ctx, true));
        return zk_groth16_prove_shared(ctx, pk, r, z_share, r_share, s_share, tx, ty, tz, net, proofs_out, bytes_sent);
    }
    return prove_shared_batch_impl<1>(ctx, pk, r, count, chunk, z, rs, ss, txs, tys, tzs, net, proofs_out, bytes_sent);
    ZK_API_END
}

extern "C" int zk_groth16_prove_shared_spdz_batch(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, size_t count, const void* const z_lanes[2],
                                                  const zk_fr* const r_lanes[2], const zk_fr* const s_lanes[2], const void* const tx_lanes[2],
                                                  const void* const ty_lanes[2], const void* const tz_lanes[2], const zk_net_vtable* net,
                                                  uint8_t* proofs_out, uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !count || !z_lanes || !z_lanes[0] || !z_lanes[1] || !r_lanes || !r_lanes[0] || !r_lanes[1] || !s_lanes ||
        !s_lanes[0] || !s_lanes[1] || !proofs_out)
        return ZK_ERR_ARG;
    const void* none[2] = {nullptr, nullptr};
    const void* const* txs = tx_lanes ? tx_lanes : none;
    const void* const* tys = ty_lanes ? ty_lanes : none;
    const void* const* tzs = tz_lanes ? tz_lanes : none;
    if (zk_shared_triple_given(2, txs, tys, tzs) < 0) ZK_FAIL(ctx, ZK_ERR_ARG, "prove_shared_batch: give a whole Beaver triple (every lane) or none");
    size_t chunk;
    ZK_TRY(shared_batch_plan(ctx, pk, r, count, 2, &chunk));
    if (count == 1) {
        ZK_TRY(zk_next_z_drop(ctx, true));
        const zk_fr rl[2] = {*r_lanes[0], *r_lanes[1]}, sl[2] = {*s_lanes[0], *s_lanes[1]};
        return zk_groth16_prove_shared_spdz(ctx, pk, r, z_lanes, rl, sl, tx_lanes, ty_lanes, tz_lanes, net, proofs_out, bytes_sent);
    }
    return prove_shared_batch_impl<2>(ctx, pk, r, count, chunk, z_lanes, r_lanes, s_lanes, txs, tys, tzs, net, proofs_out, bytes_sent);
    ZK_API_END
}
