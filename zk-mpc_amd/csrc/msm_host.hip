// msm_host.hip -- AffineCurve::multi_scalar_mul on HOST slices (zk_msm_g1 / _g2 / _strided, and the MPC entry points' table run),
// and the MSMs it starts ahead of the calls that will ask for them.  The arithmetic is msm.hip's, through the job stages of
// internal.hpp; the tables come from the cache (bases_cache.hip); what is learned about a caller's order of calls is msm_spec.hpp.
#include "../../include/zkmpc_hip.h"
#include "hostgroup.hpp"
#include "internal.hpp"
#include "msm_spec.hpp"
#include <algorithm>
#include <memory>
#include <stdlib.h>
#include <vector>

using namespace zk;

namespace {
__global__ void __launch_bounds__(256) k_scalars_differ(const uint4* a, const uint4* b, size_t n16, uint32_t* flag) {
    bool diff = false;
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
        const uint4 x = a[i], y = b[i];
        diff = diff || x.x != y.x || x.y != y.y || x.z != y.z || x.w != y.w;
    }
    if (diff) *flag = 1;
}
}  // namespace

// ---- MSMs started AHEAD for the tables a caller asks for next with the same scalars -----------------------------------------------
// The unchanged create_proof runs its MSMs one call behind the other, and three of them over ONE scalar vector: calculate_coeff with
// &pk.a_query, then &pk.b_g1_query, then &pk.b_g2_query over `assignment` (src/groth16.rs:137-160).  Every call is synchronous -- the
// trait returns the point -- so the upload, the sort, the reduce chain and the host's Horner half of one call never overlap the next
// call's kernels, as they do in the resident prover.  What CAN be known: which table followed which with the same scalars last time.
// So a context learns "after table T (scalars S) came table T' with the same S" (candidates by a fingerprint of 64 sampled scalars
// taken from host memory), and when T is asked for again it also starts the MSMs over T' and T'' -- on a private copy of the scalars,
// on the context's side stream, own scratch slots (ZK_SLOT_AHEAD) -- before it collects T's result.  The next call, if it names T' and
// its scalars are WORD FOR WORD the ones the speculative job ran on (compared on the device), takes that result; anything else
// drops the speculation (and after two wrong guesses for a table the pattern is forgotten).  Table hits are verified as always.
// Nothing speculative is ever returned unverified; ZK_MSM_SPEC=0 switches the whole thing off (A/B).
//
// One object per context: the policy (what was learned), the jobs in flight with the scalar copy they run on, the counters.
struct ZkMsmSpec {
    struct Job { const zk_bases* table; ZkMsmJob job; };
    zk_ctx* const ctx;
    ZkMsmSpecPolicy policy;
    std::vector<std::unique_ptr<Job>> jobs;              // in the order they will be asked for
    size_t n = 0;                                        // ... all over one copy of n scalars ("spec_scalars") with this fingerprint
    uint64_t fp = 0;
    uint32_t* flag_dev = nullptr;                        // the verdict of k_scalars_differ
    uint32_t* flag_host = nullptr;
    uint64_t started = 0, taken = 0, dropped = 0;        // jobs
    bool off = false;                                    // zk_msm_speculate(ctx, 0)
    bool fp_pending = false;                             // a job started by fft_begin whose fingerprint fft_end still owes
    const void* late_dev = nullptr;                      // a LARGE job fft_begin left to fft_end (defer / start_deferred)
    const zk_bases* late_table = nullptr;
    size_t late_n = 0;

    explicit ZkMsmSpec(zk_ctx* c) : ctx(c) {}
    ~ZkMsmSpec() {
        drop();
        if (flag_dev) (void)hipFree(flag_dev);
        if (flag_host) (void)hipHostFree(flag_host);
    }
    static bool fits(const zk_bases* t, size_t n) { return n <= t->n; }

    // what is in flight is abandoned: its kernels read the scratch slots and the scalar copy, so they are waited for
    void drop() {
        if (jobs.empty()) return;
        if (!ctx->aux.empty()) (void)hipStreamSynchronize(ctx->aux[0]);
        if (ctx->acc_stream) (void)hipStreamSynchronize(ctx->acc_stream);
        dropped += jobs.size();
        jobs.clear();
        fp_pending = false;
    }

    // `t` is leaving the cache or changing content: no job over it, nothing learned about it
    void forget(const zk_bases* t) {
        for (auto& j : jobs) if (j->table == t) { drop(); break; }
        policy.forget(t);
        if (late_table == t) late_dev = nullptr;
    }

    // MSMs over `tables` with a private copy of the scalars (n elements on the device, final on the context stream): every phase of
    // every job on the context's ONE side stream, one job behind the other (core.hip::zk_side_stream says why there is only one)
    int start(const zk_bases* const* tables, int cnt, const void* scalars, size_t n_, uint64_t fp_) {
        void* copy;
        ZK_TRY(zk_scratch(ctx, "spec_scalars", n_ * 32, &copy));
        hipStream_t side;
        ZK_TRY(zk_side_stream(ctx, &side));
        ZK_HIP(ctx, hipMemcpyAsync(copy, scalars, n_ * 32, hipMemcpyDeviceToDevice, ctx->stream));
        ZK_HIP(ctx, zk_streams_follow(ctx->stream, &side, 1));
        int rc = ZK_OK;
        for (int k = 0; k < cnt && rc == ZK_OK; k++) {
            std::unique_ptr<Job> j(new Job());
            j->table = tables[k];
            j->job.pin = {ZK_PIN_AHEAD, (uint32_t)k};
            rc = zk_msm_prepare(ctx, &j->job, tables[k], 0, copy, n_, ZK_SLOT_AHEAD + k);
            if (rc == ZK_OK) rc = zk_msm_enqueue_sort(ctx, &j->job, side, nullptr);
            if (rc == ZK_OK) rc = zk_msm_enqueue_accum(ctx, &j->job, side);
            if (rc == ZK_OK) rc = zk_msm_enqueue_reduce(ctx, &j->job, side);
            jobs.push_back(std::move(j));                    // (even a half-enqueued one: drop waits for whatever it launched)
            if (rc == ZK_OK) started++;
        }
        n = n_;
        fp = fp_;
        if (rc != ZK_OK) drop();
        return rc;
    }
    // the tables that followed `t` last time
    int start_after(const zk_bases* t, const void* scalars, size_t n_, uint64_t fp_) {
        const zk_bases* next[2];
        const int cnt = policy.next(t, n_, fits, next);
        return cnt ? start(next, cnt, scalars, n_, fp_) : ZK_OK;
    }

    // the job over a transform's output (in `dev`) that is too large to run beside the download of that output: once it is through
    void defer(const void* dev, const zk_bases* t, size_t n_) { late_dev = dev; late_table = t; late_n = n_; }
    void start_deferred(size_t N, const uint64_t fp_[2]) {
        if (late_dev && jobs.empty() && (late_n == N || late_n + 1 == N)) (void)start(&late_table, 1, late_dev, late_n, fp_[late_n == N ? 0 : 1]);
        late_dev = nullptr;
    }

    // Is the front job this call's?  The same table, length and fingerprint make it a candidate; it is the call's if the scalars the
    // call brought (on the device, final on the context stream) equal the jobs' copy word for word.  Anything else is a wrong guess,
    // and everything in flight goes.
    int claim_or_drop(const zk_bases* t, size_t n_, uint64_t fp_, bool eligible, const void* scalars, bool* mine) {
        *mine = false;
        if (jobs.empty()) return ZK_OK;
        const zk_bases* front = jobs.front()->table;
        int rc = ZK_OK;
        if (eligible && front == t && n == n_ && fp == fp_) rc = same_scalars(scalars, mine);
        if (rc == ZK_OK && *mine) return ZK_OK;
        *mine = false;
        policy.wrong_guess(front, t, eligible);
        drop();
        return rc;
    }
    // the result that was started during the previous call
    int take(void* out) {
        const int rc = zk_msm_finish(ctx, &jobs.front()->job, out);
        policy.right_guess(jobs.front()->table);
        jobs.erase(jobs.begin());
        taken++;
        return rc;
    }

private:
    int same_scalars(const void* scalars, bool* same) {
        void* copy;
        ZK_TRY(zk_scratch(ctx, "spec_scalars", n * 32, &copy));
        if (!flag_dev) {
            ZK_HIP(ctx, hipMalloc((void**)&flag_dev, 16));
            ZK_HIP(ctx, hipHostMalloc((void**)&flag_host, 16, hipHostMallocDefault));
        }
        ZK_HIP(ctx, hipMemsetAsync(flag_dev, 0, 4, ctx->stream));
        hipLaunchKernelGGL(k_scalars_differ, zk_grid(n * 2, 256), 256, 0, ctx->stream, (const uint4*)scalars, (const uint4*)copy, n * 2, flag_dev);
        ZK_HIP(ctx, hipGetLastError());
        ZK_HIP(ctx, hipMemcpyAsync(flag_host, flag_dev, 4, hipMemcpyDeviceToHost, ctx->stream));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *same = *flag_host == 0;
        return ZK_OK;
    }
};

namespace {
ZkMsmSpec* spec_of(zk_ctx* ctx) {
    if (!ctx->msm_spec) ctx->msm_spec = new ZkMsmSpec(ctx);
    return ctx->msm_spec;
}
// may this context start MSMs ahead now?
bool spec_allowed(const zk_ctx* ctx) {
    static const bool env_on = !(getenv("ZK_MSM_SPEC") && atoi(getenv("ZK_MSM_SPEC")) == 0);
    return env_on && !ctx->profiling && !(ctx->msm_spec && ctx->msm_spec->off);
}
// Does a job over n scalars and `t` run BESIDE the work it is started next to, or BEHIND it?  Up to 2^22 digits (2^17 scalars over a
// plain table) beside, above that behind.
// Next to a table call: a SMALL call is a chain of latencies on a mostly idle chip: the jobs start at once, behind nothing but the
// copy of the scalars, and run beside the call's own kernels (2^10 .. 2^16: -12 .. -20 % per proof).  A LARGE call fills the chip:
// started at once they only delay the call's result (2^20: the A call 4 -> 13.5 ms, the three calls 16.6 -> 21.6), so they queue
// behind the call's whole device chain (a reduce chain beside a running accumulate kernel is starved) and run under the call's host
// half and the caller's way back into the library.
// Next to a transform: a small job starts under the download of the transform's result.  A large one would share a hardware queue
// with that download (2^20: the last transform 1.7 -> 3.2 ms, measured): it starts when the result is through
// (zk_msm_spec_fft_end) and runs under the caller's way back into the library and the upload of the scalars.
bool spec_runs_beside(const zk_bases* t, size_t n) {
    return t->pre ? n * ((255 + t->c_pre - 1) / t->c_pre) <= ((size_t)1 << 22) : n <= ((size_t)1 << 17);
}

// 64 sampled elements and the length: how a repeated scalar vector is recognised (a candidate: see ZkMsmSpec::claim_or_drop)
uint64_t scalars_fingerprint(const zk_fr* s, size_t n) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)n;
    const size_t S = n < 64 ? n : 64;
    for (size_t k = 0; k < S; k++) {
        const size_t i = S > 1 ? k * (n - 1) / (S - 1) : 0;
        for (int w = 0; w < 4; w++) { h ^= s[i].l[w]; h *= 0xFF51AFD7ED558CCDull; h ^= h >> 32; }
    }
    return h ? h : 1;
}

ZkHostTable host_table(int group, const void* host, const ZkAffineLayout* layout) {
    ZkHostTable t;
    t.group = group;
    t.host = host;
    const size_t FE = group == 1 ? 48 : 96;
    if (layout) { t.stride = layout->stride; t.off_x = layout->off_x; t.off_y = layout->off_y; t.off_inf = layout->off_inf; }
    else { t.stride = 2 * FE; t.off_x = 0; t.off_y = FE; t.off_inf = SIZE_MAX; }
    return t;
}

int msm_host(zk_ctx* ctx, int group, const void* bases_host, size_t nb, const ZkAffineLayout* layout, const zk_fr* scalars, size_t ns, void* out) {
    if (!ctx || !out) return ZK_ERR_ARG;
    const size_t n = std::min(nb, ns);  // variable_base.rs:15-17
    if (n && (!bases_host || !scalars)) return ZK_ERR_ARG;
    if (n == 0) {
        if (group == 1) host_write_projective<G1Field>(aff_inf<G1Field>(), (uint64_t*)out);
        else host_write_projective<G2Field>(aff_inf<G2Field>(), (uint64_t*)out);
        return ZK_OK;
    }
    const size_t nu = nb <= 2 * n ? nb : n;                  // the whole slice (it is the cache's key) unless most of it is unused
    void* sdev = nullptr;
    ZK_TRY(zk_scratch(ctx, "msm_scalars_host", n * 32, &sdev));
    ZK_TRY(zk_xfer_h2d(ctx, sdev, scalars, n * 32));
    const void* sc[1] = {sdev};
    void* outs[1] = {out};
    return zk_msm_table_run(ctx, host_table(group, bases_host, layout), nu, 1, sc, n, outs, scalars_fingerprint(scalars, n));
}

bool layout_from_abi(const zk_affine_layout* l, ZkAffineLayout* o) {
    if (!l) return false;
    o->stride = l->stride; o->off_x = l->off_x; o->off_y = l->off_y; o->off_inf = l->off_infinity;
    return true;
}
}  // namespace

// AffineCurve::multi_scalar_mul on host slices.  The bases come through the context's table cache (bases_cache.hip): a table the
// context has seen before -- the queries of a proving key, the powers of an SRS -- is resident already (window multiples are built
// beside later calls), and only the scalars cross PCIe for the arithmetic; the caller's slice crosses once more, UNDER the MSM, to
// be compared in full with what the cached table was made from (a hit is a candidate until that comparison is through).
// n_lanes MSMs over the same table (the two lanes of a SPDZ multi_scale_pub_group: share/spdz.rs:482-488): scalars_dev[l] -> outs[l].
int zk_msm_table_run(zk_ctx* ctx, const ZkHostTable& t, size_t nu, int n_lanes, const void* const* scalars_dev, size_t n, void* const* outs, uint64_t sfp) {
    ZkBasesLease lease(ctx);
    ZK_TRY(zk_bases_cache_get(ctx, t, nu, &lease));
    const bool spec_ok = ZkMsmSpecPolicy::eligible(spec_allowed(ctx), n_lanes, lease.temporary, sfp);
    ZkMsmSpec* sp = spec_ok || ctx->msm_spec ? spec_of(ctx) : nullptr;
    bool take = false;                                       // is this the call the jobs in flight were started for?
    int rc = sp ? sp->claim_or_drop(lease.b, n, sfp, spec_ok, scalars_dev[0], &take) : ZK_OK;
    if (sp) sp->policy.observe(lease.b, n, sfp, spec_ok && rc == ZK_OK);
    for (int attempt = 0; attempt < 2 && rc == ZK_OK; attempt++) {
        bool same = true;
        int vrc = ZK_OK;
        {
            ZkTask<void> verifier;                           // (joins when this block is left, whatever the MSM did)
            if (lease.verify)
                verifier = zk_async(ctx, [&] { (void)hipSetDevice(ctx->device); vrc = zk_bases_cache_verify(ctx, &lease, t, nu, &same); });
            if (take) {
                rc = sp->take(outs[0]);
                take = false;
            } else if (n_lanes == 1) {
                // the MSMs this caller asked for next the last time it came with this table: before this call's own job or after it
                const bool ahead = spec_ok && attempt == 0 && sp->jobs.empty();
                const bool beside = ahead && spec_runs_beside(lease.b, n);
                if (beside) (void)sp->start_after(lease.b, scalars_dev[0], n, sfp);
                ZkMsmJob job;
                rc = zk_msm_prepare(ctx, &job, lease.b, 0, scalars_dev[0], n, ZK_SLOT_RUN);
                if (rc == ZK_OK) rc = zk_msm_enqueue_sort(ctx, &job, ctx->stream, nullptr);
                if (rc == ZK_OK) rc = zk_msm_enqueue_accum(ctx, &job, ctx->stream);
                if (rc == ZK_OK) rc = zk_msm_enqueue_reduce(ctx, &job, ctx->stream);
                if (rc == ZK_OK && ahead && !beside) (void)sp->start_after(lease.b, scalars_dev[0], n, sfp);
                if (rc == ZK_OK) rc = zk_msm_finish(ctx, &job, outs[0]);
                else (void)hipStreamSynchronize(ctx->stream);
            } else {
                const zk_bases* bs[2] = {lease.b, lease.b};
                const size_t lens[2] = {n, n};
                rc = zk_msm_batch_dev(ctx, (size_t)n_lanes, bs, nullptr, scalars_dev, lens, outs);
            }
        }
        if (rc == ZK_OK) rc = vrc;
        if (rc != ZK_OK || same) break;
        rc = zk_bases_cache_replace(ctx, &lease);            // the table at the caller's address is not the cached one any more: again, on the right one
    }
    if (rc != ZK_OK && sp) sp->drop();
    return rc;
}
uint64_t zk_scalars_fingerprint(const void* fr, size_t n) { return scalars_fingerprint((const zk_fr*)fr, n); }

void zk_msm_spec_drop(zk_ctx* ctx) {
    if (ctx->msm_spec) ctx->msm_spec->drop();
}
// A transform of 2^log_n elements on a caller's host vector has been enqueued (its result is in `dev`, final on the context stream,
// not yet on its way back): if the MSM that followed such a transform last time took the output as its scalars, that MSM starts
// now -- under the download of the result and the upload of the scalars the call will bring (which are compared with `dev`'s copy
// before the result is released, like every job started ahead).
void zk_msm_spec_fft_begin(zk_ctx* ctx, const void* dev, size_t N, int kind) {
    ZkMsmSpec* sp = ctx->msm_spec;
    if (sp) sp->late_dev = nullptr;                          // (a transform that failed between begin and end leaves nothing behind)
    if (!sp || !spec_allowed(ctx) || !sp->jobs.empty()) return;
    // (of the seven transforms of a witness map only the last -- the one coset inverse -- writes the H query's scalars: the kind is
    // part of what is learned)
    const ZkMsmSpecPolicy::AfterFft* a = sp->policy.after_transform(N, kind, ZkMsmSpec::fits);
    if (!a) return;
    if (!spec_runs_beside(a->table, a->n)) { sp->defer(dev, a->table, a->n); return; }
    if (sp->start(&a->table, 1, dev, a->n, 0) == ZK_OK && !sp->jobs.empty()) sp->fp_pending = true;
}
// ... and the result has arrived in the caller's vector: fp_of(n) = the fingerprint an MSM entry point would compute over its first n
// elements (plain: scalars_fingerprint; MpcField: mpc_host.hip's)
void zk_msm_spec_fft_end(zk_ctx* ctx, size_t N, int kind, const std::function<uint64_t(size_t)>& fp_of) {
    if (!spec_allowed(ctx) || N < 2) return;
    ZkMsmSpec* sp = spec_of(ctx);
    const uint64_t fp[2] = {fp_of(N), fp_of(N - 1)};
    sp->policy.transform_done(N, kind, fp[0], fp[1]);
    if (sp->fp_pending && !sp->jobs.empty()) sp->fp = fp[sp->n == N ? 0 : 1];
    sp->fp_pending = false;
    sp->start_deferred(N, fp);
}
void zk_msm_spec_forget(zk_ctx* ctx, const zk_bases* b) {
    if (ctx->msm_spec) ctx->msm_spec->forget(b);
}
void zk_msm_spec_free(zk_ctx* ctx) {
    delete ctx->msm_spec;
    ctx->msm_spec = nullptr;
}
extern "C" int zk_msm_speculate(zk_ctx* ctx, int on) {
    ZK_API_BEGIN(ctx)
    if (!ctx) return ZK_ERR_ARG;
    ZkMsmSpec* sp = spec_of(ctx);
    sp->off = on == 0;
    if (sp->off) { sp->drop(); sp->policy.clear(); }
    return ZK_OK;
    ZK_API_END
}
extern "C" int zk_msm_speculate_stats(zk_ctx* ctx, uint64_t out[3]) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !out) return ZK_ERR_ARG;
    ZkMsmSpec* sp = ctx->msm_spec;
    out[0] = sp ? sp->started : 0; out[1] = sp ? sp->taken : 0; out[2] = sp ? sp->dropped : 0;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_msm_g1(zk_ctx* ctx, const zk_g1_affine* bases, size_t nb, const zk_fr* scalars, size_t ns, zk_g1_projective* out) {
    ZK_API_BEGIN(ctx)
    return msm_host(ctx, 1, bases, nb, nullptr, scalars, ns, out);
    ZK_API_END
}
extern "C" int zk_msm_g2(zk_ctx* ctx, const zk_g2_affine* bases, size_t nb, const zk_fr* scalars, size_t ns, zk_g2_projective* out) {
    ZK_API_BEGIN(ctx)
    return msm_host(ctx, 2, bases, nb, nullptr, scalars, ns, out);
    ZK_API_END
}
extern "C" int zk_msm_g1_strided(zk_ctx* ctx, const void* bases, size_t nb, const zk_affine_layout* layout, const zk_fr* scalars, size_t ns,
                                 zk_g1_projective* out) {
    ZK_API_BEGIN(ctx)
    ZkAffineLayout lay;
    if (!layout_from_abi(layout, &lay)) return ZK_ERR_ARG;
    return msm_host(ctx, 1, bases, nb, &lay, scalars, ns, out);
    ZK_API_END
}
extern "C" int zk_msm_g2_strided(zk_ctx* ctx, const void* bases, size_t nb, const zk_affine_layout* layout, const zk_fr* scalars, size_t ns,
                                 zk_g2_projective* out) {
    ZK_API_BEGIN(ctx)
    ZkAffineLayout lay;
    if (!layout_from_abi(layout, &lay)) return ZK_ERR_ARG;
    return msm_host(ctx, 2, bases, nb, &lay, scalars, ns, out);
    ZK_API_END
}
