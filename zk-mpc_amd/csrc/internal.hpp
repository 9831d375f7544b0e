// internal.hpp -- declarations shared between the translation units of libzkmpc_hip.
#pragma once
#include "ctx.hpp"
#include "ec.cuh"
#include "msm_digits.cuh"
#include "stream_order.hpp"
#include <stddef.h>
#include <stdint.h>
#include <atomic>
#include <chrono>
#include <functional>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

// ntt.hip
void zk_domains_free(zk_ctx* ctx);
void zk_presort_free(zk_ctx* ctx);   // groth16_pipeline.hip: drain and drop the MSM jobs enqueued ahead of a proof (ZkG16Flight)
extern "C" int zk_comm_destroy(zk_ctx* ctx);
extern "C" int zk_fr_sum_parties_dev(zk_ctx* ctx, const void* gathered_dev, size_t n_parties, size_t n, void* out_dev);
int zk_ntt_launch(zk_ctx* ctx, void* buf_dev, uint32_t log_n, int inverse, int coset);
int zk_ntt_launch_batch(zk_ctx* ctx, void* const* bufs_dev, int count, uint32_t log_n, int inverse, int coset);   // count <= 4, same size and kind, one launch per pass
// count transforms of one size and kind in place at base + k * stride elements (stride >= 2^log_n): one launch per pass whatever
// count is (up to 65535 transforms per launch).  tmp: room for min(count, 65535) 2^log_n elements for transforms of more than one pass
// (2^log_n > 2^10), or NULL for the context's grow-only "ntt_tmp" slot
int zk_ntt_launch_strided(zk_ctx* ctx, void* base, size_t count, size_t stride, uint32_t log_n, int inverse, int coset, void* tmp = nullptr);
int zk_ntt_vanishing_inv(zk_ctx* ctx, uint32_t log_n, zk::Fr* out);  // 1/(g^N - 1), internal form
// the elements of the domain of size 2^log_n as the transforms keep them resident (w^i for i < 2^log_n: internal form, nine limbs = 36
// bytes each, devutil.cuh::tab_load) and 1 / 2^log_n in internal form
int zk_ntt_domain_elements(zk_ctx* ctx, uint32_t log_n, const uint32_t** elements_dev, zk::Fr* size_inv);
// poly.hip: out[i] = start * base^i for i < n, base and start in internal form, on ctx->stream; out holds n elements in the
// reference's form (32 bytes each) or n table entries (36 bytes each, tab_load)
enum ZkFrForm { ZK_FR_EXT = 0, ZK_FR_TABLE = 1 };
int zk_fr_powers_launch(zk_ctx* ctx, const zk::Fr& base, const zk::Fr& start, size_t n, void* out, ZkFrForm form);

// The kernel groups whose hipFuncSetAttribute list runs once per context (zk_ctx::lds_attr_done, set by the site once its list succeeded)
enum ZkLdsAttr {
    ZK_LDS_NTT, ZK_LDS_SORT_SMALL, ZK_LDS_SORT_SMALL_GROUP, ZK_LDS_SORT_GROUP, ZK_LDS_SHE, ZK_LDS_LINCOMB, ZK_LDS_SCALE_FOLD,
    ZK_LDS_TERM_FOLD_FULL, ZK_LDS_TERM_FOLD_GLV,      // g1_term_fold.hip: one slot per instantiation (an attribute belongs to ONE function)
    ZK_LDS_SCALE_FOLD_KEYED,                          // groth16_verify_keys.hip
    ZK_LDS_COUNT
};
static_assert(ZK_LDS_COUNT <= sizeof(zk_ctx::lds_attr_done), "zk_ctx::lds_attr_done is too short");

// rng.hip: four little-endian 64-bit words are a canonical field element (< r): what Fr::rand keeps and what a prover accepts from a peer
bool zk_fr_words_valid(const uint64_t l[4]);

// vec_ops.hip
// core.hip: a launch-bound sequence on ONE stream as a captured graph from its third use with the same key (see there)
int zk_graph_run(zk_ctx* ctx, const std::string& key, hipStream_t st, const std::function<int()>& enqueue);
int zk_vec_op_launch(zk_ctx* ctx, int op, const void* a, const void* b, void* out, size_t n);
int zk_vec_scale_launch(zk_ctx* ctx, const void* a, const zk::Fr& k_int, void* out, size_t n);      // constants: internal form
// zk_fr_vec_is_zero_dev without the wait: *verdict points at a page-locked word that is 0 (all zero) or not once ctx->stream has
// passed this point (slot 0..7: tests in flight)
int zk_fr_vec_is_zero_launch(zk_ctx* ctx, const void* v, size_t n, int slot, const uint32_t** verdict);
// out = rp (kc s + ka a + kb b) - z tp, element-wise (Marlin round 2); out may alias s
int zk_fr_outer_q1_launch(zk_ctx* ctx, const void* s, const void* a, const void* b, const void* z, const void* rp, const void* tp,
                          const zk::Fr& ka_int, const zk::Fr& kb_int, const zk::Fr& kc_int, void* out, size_t n);
// out[i] = sum_t k_t p_t[i] (terms with i < ns[t]); constants in internal form; out may not alias a term
int zk_fr_lincomb_launch(zk_ctx* ctx, int terms, const void* const* ps, const size_t* ns, const zk::Fr* k_int, void* out, size_t n_out);
int zk_vec_sub_scale_launch(zk_ctx* ctx, const void* a, const void* b, const zk::Fr& k_int, void* out, size_t n);

// ---- the batched forms: count vectors of one length, proof k's at base + k * stride elements (marlin_prove_batch.hip) ----
// What a step of a batch uploads -- per-proof constants, job arrays: page-locked host memory and a device buffer of the same size,
// both the caller's.  put() copies `bytes` into the host half and enqueues their copy to the device half on ctx->stream; the
// owner calls reset() only behind a host wait for that stream (the host half is rewritten then).
struct ZkStage {
    zk_ctx* ctx = nullptr;
    char *host = nullptr, *dev = nullptr;
    size_t cap = 0, used = 0;
    void reset() { used = 0; }
    int put(const void* src, size_t bytes, const void** dev_out);      // core.hip
};
// poly.hip: zk_poly_divide_by_vanishing_dev for count polynomials of n coefficients; sums: room for count * zk_poly_divv_sums_elems
// elements (none wanted: 0).  On ctx->stream, no wait.
size_t zk_poly_divv_sums_elems(size_t n, uint32_t log_domain);
int zk_poly_divide_by_vanishing_strided(zk_ctx* ctx, const void* c, size_t c_stride, size_t n, uint32_t log_domain, size_t count, void* q, size_t q_stride,
                                        void* rem, size_t rem_stride, void* sums);
// poly.hip: p_k / (X - z_k) for count polynomials of n >= 2 coefficients, the quotients (n - 1 coefficients) at q + k * q_stride; a
// polynomial of one span (n <= 4 096) is one launch whatever count is, a longer one three.  spans: room for 2 * count *
// zk_poly_divlin_spans(n) elements.  The job array goes through `stage` (zk_poly_divlin_job_bytes each).  No wait.
size_t zk_poly_divlin_spans(size_t n);
size_t zk_poly_divlin_job_bytes();
int zk_poly_divide_by_linear_strided(zk_ctx* ctx, const void* c, size_t c_stride, size_t n, const zk::Fr* z_int, size_t count, void* q, size_t q_stride,
                                     void* spans, ZkStage* stage);
// marlin_batch.hip: the element-wise kernels of the Marlin rounds over count vectors (strides in elements; n items each), on
// ctx->stream, no wait.  tab: the step's per-proof constants on the device, proof k's row at tab + k * ts entries (devutil.cuh: FrK,
// internal form unless a kernel says otherwise).  The kernels that read a row of tab or a public per-proof operand take `proofs`
// for a launch over shares: count = lanes * proofs vectors, lane after lane, vector v of proof v mod proofs (0: count proofs, one vector each).
namespace zk { struct FrK; }
int zk_b_copy(zk_ctx* ctx, void* dst, size_t ds, const void* src, size_t ss, size_t n, size_t count);
int zk_b_zero(zk_ctx* ctx, void* dst, size_t ds, size_t n, size_t count);
int zk_b_op(zk_ctx* ctx, int op, const void* a, size_t sa, const void* b, size_t sb, void* out, size_t so, size_t n, size_t count);
int zk_b_scale(zk_ctx* ctx, const void* a, size_t sa, const zk::FrK* tab, size_t ts, void* out, size_t so, size_t n, size_t count,
               size_t proofs = 0);      // a_k * tab_k[0]
int zk_b_gather(zk_ctx* ctx, const void* src, size_t ss, const uint32_t* idx, size_t n, void* out, size_t so, size_t count);
// out_k = p_k + r_k[0] (X^n - 1): n + 1 coefficients
int zk_b_blind(zk_ctx* ctx, const void* p, size_t sp, size_t n, const void* r, size_t sr, void* out, size_t so, size_t count);
// out_k[i] = tab_k[0] - e[i]; tab_k[0]: the bits of the constant's external form
int zk_b_const_minus(zk_ctx* ctx, const zk::FrK* tab, size_t ts, const void* e, size_t n, void* out, size_t so, size_t count);
// zk_fr_outer_q1_launch with tab_k = eta_a, eta_b, eta_c; every vector `stride` elements apart (proofs: rp and tp are one vector per proof)
int zk_b_outer_q1(zk_ctx* ctx, const void* s, const void* a, const void* b, const void* z, const void* rp, const void* tp, size_t stride,
                  const zk::FrK* tab, size_t ts, void* out, size_t n, size_t count, size_t proofs = 0);
// zk_fr_lincomb_launch with tab_k[t] = the coefficient of term t (at most 16 terms); strides[t] = 0: one vector for every proof
// (proofs: bit t of per_proof says that term t is one vector per proof, not one per lane and proof)
int zk_b_lincomb(zk_ctx* ctx, int terms, const void* const* ps, const size_t* strides, const size_t* ns, const zk::FrK* tab, size_t ts, void* out, size_t so,
                 size_t n_out, size_t count, size_t proofs = 0, unsigned per_proof = 0);
// round 3 (marlin.hip's zk_marlin_round3_f_evals_dev in its two halves around the inversion, and _ab_evals_dev): one row of
// ZK_B_R3_ROW constants per proof, filled by zk_b_round3_row (alpha, beta, eta, vv = v_H(alpha) v_H(beta): internal form);
// den: count * 3 k_size elements
constexpr int ZK_B_R3_ROW = 11;
void zk_b_round3_row(const zk::Fr& alpha, const zk::Fr& beta, const zk::Fr eta[3], const zk::Fr& vv, zk::FrK* row);
int zk_b_round3_denoms(zk_ctx* ctx, const zk_marlin_matrix_evals on_k[3], size_t k_size, const zk::FrK* tab, void* den, size_t count);
int zk_b_round3_f(zk_ctx* ctx, const zk_marlin_matrix_evals on_k[3], size_t k_size, const zk::FrK* tab, const void* inv, void* f, size_t f_stride, size_t count);
int zk_b_round3_ab(zk_ctx* ctx, const zk_marlin_matrix_evals on_b[3], size_t b_size, const zk::FrK* tab, void* a_out, void* b_out, size_t stride, size_t count);
// r1cs.hip: zk_r1cs_matvec_dev for count vectors (z_k at z + k * z_stride, the product at out + k * out_stride, out_len elements)
struct zk_r1cs;
int zk_r1cs_matvec_strided(zk_ctx* ctx, const zk_r1cs* r, int which, const void* z, size_t z_stride, size_t count, void* out, size_t out_stride,
                           size_t out_len);

// msm.hip
struct zk_bases {
    int group = 1;             // 1 = G1, 2 = G2
    size_t n = 0;              // number of points
    uint32_t* dev = nullptr;   // packed affine, internal Montgomery form: n * (24|48) words
    bool owned = true;
    // optional window multiples for resident bases: pre[w*n + i] = 2^(c_pre*w) * base_i, w < W_pre (pre[0..n) = dev copy).
    // With them every window of an MSM drops into ONE bucket set (fixed_base.hip: zk_bases_precompute).
    uint32_t* pre = nullptr;
    uint32_t c_pre = 0, W_pre = 0;
    uint32_t pre_stride = 0;   // 32-bit words per point in `pre` (0: packed, 2 * WORDS).  G1: 32 = one 128-byte line per 96-byte point;
                               // 64 = limb form, line 0 the point, line 1 its negative (fixed_base.hip::k_repack_limbs)
    // shifted multiples (Groth16 proving keys): `pre` holds pre_levels + 1 such tables back to back, level m = 2^m times level 0
    // (entry index m * W_pre * n + w * n + i); an MSM over it reduces 2^(c-2) + 2^(c-2-M) buckets instead of 2^(c-1) (msm_digits.cuh)
    uint32_t pre_levels = 0;
    std::string pre_note;      // which layout `pre` has, or why the window multiples were skipped (zk_bases_precompute_note)
};
// hostxfer.hip: caller-owned (pageable) host memory <-> device through the context's page-locked ring; h2d returns once the host
// buffer has been read (the context stream waits for the DMA), d2h once the host buffer is complete
// pinned = the caller's own page-locked memory (zk_host_alloc): one DMA on the context stream, in place
int zk_xfer_h2d(zk_ctx* ctx, void* dev, const void* host, size_t bytes, bool pinned = false);
int zk_xfer_d2h(zk_ctx* ctx, void* host, const void* dev, size_t bytes, bool pinned = false);
// ... with the bytes produced / consumed piece by piece by the ring's thread team (gathers out of and scatters into the caller's own
// struct layouts); fence_ctx = false: on the DMA stream alone (see hostxfer.hip)
using ZkXferFill = std::function<void(char* dst, size_t off, size_t len)>;
using ZkXferDrain = std::function<void(const char* src, size_t off, size_t len)>;
int zk_xfer_h2d_fn(zk_ctx* ctx, void* dev, size_t bytes, const ZkXferFill& fill, bool fence_ctx,
                   const std::function<int(size_t, size_t, hipStream_t)>* after_round);
int zk_xfer_d2h_fn(zk_ctx* ctx, const void* dev, size_t bytes, const ZkXferDrain& drain);
int zk_xfer_stream(zk_ctx* ctx, hipStream_t* st);
void zk_xfer_free(zk_ctx* ctx);
bool zk_host_is_pinned(const void* host);      // page-locked by HIP (hipHostMalloc / hipHostRegister): safe to hand to hipMemcpyAsync
// a host table in the caller's own struct layout (zk_affine_layout of the ABI); off_inf == SIZE_MAX: no flag, all-zero bytes = infinity
struct ZkAffineLayout { size_t stride, off_x, off_y, off_inf; };
int zk_bases_upload_host(zk_ctx* ctx, int group, const void* host, size_t n, const ZkAffineLayout* layout, zk_bases** out);   // msm.hip
// msm.hip: an empty device-form table of n points / its content from the packed ABI form (n * 96 | 192 bytes on the device), on `st`
int zk_bases_alloc_dev(zk_ctx* ctx, int group, size_t n, zk_bases** out);
int zk_bases_import_launch(zk_ctx* ctx, zk_bases* b, const void* raw_dev, hipStream_t st);
// bases_cache.hip: the resident table for a host slice, keyed by CONTENT.  A host table as the caller holds it: packed (stride = 96 |
// 192, off_y = stride / 2, off_inf = off_tag = SIZE_MAX), GroupAffine<P> {x, y, infinity}, or that inside an MpcGroup wrapper whose
// discriminant byte at off_tag must say Public (tag_public) for every element.
struct ZkHostTable {
    int group = 1;
    const void* host = nullptr;
    size_t stride = 0, off_x = 0, off_y = 0, off_inf = SIZE_MAX, off_tag = SIZE_MAX;
    uint8_t tag_public = 0;
};
struct ZkBasesLease {               // a table handed out by zk_bases_cache_get for one call: released by scope, on every exit of the call
    zk_ctx* const ctx;              // the context it was taken on
    const zk_bases* b = nullptr;    // the table to run on
    bool temporary = false;         // made for this call only (cache off / tiny / over budget): freed with the lease
    bool verify = false;            // a hit by fingerprint: zk_bases_cache_verify must confirm it before the result leaves the library
    uint32_t* raw_tmp = nullptr;
    void* stage = nullptr;          // device buffer the caller's slice is compared in
    const void* entry = nullptr;
    explicit ZkBasesLease(zk_ctx* c) : ctx(c) {}
    ~ZkBasesLease();                // bases_cache.hip
    ZkBasesLease(const ZkBasesLease&) = delete;
    ZkBasesLease& operator=(const ZkBasesLease&) = delete;
};
int zk_bases_cache_get(zk_ctx* ctx, const ZkHostTable& t, size_t n, ZkBasesLease* out);
int zk_bases_cache_verify(zk_ctx* ctx, ZkBasesLease* l, const ZkHostTable& t, size_t n, bool* same);
int zk_bases_cache_replace(zk_ctx* ctx, ZkBasesLease* l);
// msm_host.hip: n_lanes MSMs (device scalar vectors of n elements) over ONE host table, through the cache -- verified hit and all
// scalars_fp: a fingerprint of the scalar vector taken from the caller's HOST memory (64 sampled elements and the length; 0 = none):
// what the speculation below recognises a repeated vector by -- a candidate, confirmed word for word on the device before any
// speculative result is handed out
int zk_msm_table_run(zk_ctx* ctx, const ZkHostTable& t, size_t n_table, int n_lanes, const void* const* scalars_dev, size_t n, void* const* outs,
                     uint64_t scalars_fp = 0);
// msm_host.hip: MSMs started ahead for the tables a caller asks for next with the SAME scalar vector (create_proof: A, then B in G1, then B
// in G2 over one `assignment`: src/groth16.rs:137-160).  drop: abandon what is in flight (waits for its kernels); forget: a table is
// leaving the cache or changing content; free: with the context.
void zk_msm_spec_drop(zk_ctx* ctx);
int zk_side_stream(zk_ctx* ctx, hipStream_t* out);                       // core.hip: the context's one side stream (= aux[0])
void zk_msm_spec_forget(zk_ctx* ctx, const zk_bases* b);
void zk_msm_spec_fft_begin(zk_ctx* ctx, const void* dev, size_t N, int kind);            // msm_host.hip: a host-slice transform's output as the next MSM's scalars
void zk_msm_spec_fft_end(zk_ctx* ctx, size_t N, int kind, const std::function<uint64_t(size_t)>& fp_of);
uint64_t zk_scalars_fingerprint(const void* fr, size_t n);                     // msm_host.hip: what zk_msm_g1/_g2 recognise a repeated scalar vector by
void zk_msm_spec_free(zk_ctx* ctx);
int zk_prover_streams(zk_ctx* ctx, size_t k);      // groth16_pipeline.hip: the context's helper streams
int zk_bases_cache_poll(zk_ctx* ctx);            // publish finished window multiples, start the next build (cheap: one event query)
void zk_bases_cache_free(zk_ctx* ctx);
extern "C" int zk_bases_free(zk_ctx* ctx, zk_bases* b);
constexpr size_t ZK_PRECOMP_MIN_POINTS = 256;                    // tables below this keep the plain form (zk_bases_precompute is a no-op)
extern "C" int zk_bases_precompute(zk_ctx* ctx, zk_bases* b);
// ... with `levels` shifted copies (zk_bases::pre_levels), clamped so that a reduce window keeps 2^ZK_MSM_MIN_LOG_NB buckets
constexpr uint32_t ZK_MSM_MAX_LEVELS = 3, ZK_MSM_MIN_LOG_NB = 6;
extern "C" uint32_t zk_msm_mul_levels_clamp(uint32_t c, uint32_t levels);   // fixed_base.hip
uint32_t zk_mul_levels_for_key(zk_ctx* ctx, size_t n);              // fixed_base.hip: what a proving key whose z tables have n points gets
size_t zk_key_tables_bytes(size_t n, uint32_t M, int g1_tables);     // fixed_base.hip: device bytes of such a key's tables with M shifted copies
int zk_bases_precompute_levels(zk_ctx* ctx, zk_bases* b, uint32_t levels);
uint32_t zk_precompute_windows(size_t n);                            // fixed_base.hip: copies a table of n points would get
int zk_bases_precompute_auto(zk_ctx* ctx, zk_bases* b);             // only when ZK_PRECOMP=1 (off by default: see fixed_base.hip)
// fixed_base.hip: the window multiples of a resident table built in slices on a side stream, published by a later call
// (bases_cache.hip drives it: begin = the allocations, step = the next few hundred microseconds of launches, finish = publish / drop)
struct ZkPrecompJob {
    zk_bases* b = nullptr;
    uint32_t c = 0, W = 0, wide_words = 0;
    uint32_t *packed = nullptr, *wide = nullptr, *xy = nullptr, *scr = nullptr;
    int phase = -1;                 // -1: allocations, 0: copy of level 0, 1: levels, 2: re-laid copy, 3: scratch to free, 4: complete
    uint32_t w = 1;
    size_t pos = 0, budget = 0;
    hipError_t err = hipSuccess;
};
int zk_bases_precompute_begin(zk_ctx* ctx, zk_bases* b, size_t budget_bytes, ZkPrecompJob** out);   // *out = NULL: skipped (b->pre_note says why)
hipError_t zk_bases_precompute_step(ZkPrecompJob* j, hipStream_t st, bool* more);
void zk_bases_precompute_finish(ZkPrecompJob* j, bool keep);
int zk_msm_run(zk_ctx* ctx, const zk_bases* bases, size_t base_offset, const void* scalars_dev, size_t n,
               void* out_host_projective);

// event-based phase timer (core.hip; two hipEventRecord per phase on the given stream; resolved lazily)
struct ZkPhaseTimer {
    zk_ctx* ctx;
    hipStream_t stream;
    struct Phase { std::string name; ZkEvent begin{0}, end{0}; };      // (flags 0: events that keep time)
    std::vector<Phase> ev;
    bool enabled;
    bool resolved = false;
    explicit ZkPhaseTimer(zk_ctx* c, hipStream_t st = nullptr);
    void begin(const char* name);
    void end();
    void resolve();  // waits for the recorded end events (not for the stream) and accumulates into ctx->timers
};
// host wall-clock laps: with zk_set_profiling, lap(what) adds the time since the lap before (or since construction) to the
// context's timer "<prefix><what>" -- a lap includes whatever device work the host waited for
struct ZkHostLap {
    zk_ctx* ctx;
    const char* prefix;        // "marlin.", "marlin_verify.", "verify_aggregate."
    std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
    void lap(const char* what) {
        if (!ctx->profiling) return;
        const auto now = std::chrono::steady_clock::now();
        auto& tm = ctx->timers[std::string(prefix) + what];
        tm.ms += (float)std::chrono::duration<double, std::milli>(now - t).count();
        tm.count += 1;
        t = now;
    }
};

inline unsigned zk_blocks64(size_t n) { return (unsigned)((n + 63) / 64); }      // the grid of a launch with one lane per item, one wave per block

// What a context's pinned host buffers are for (the kind of a ZkPin; ctx.hpp: zk_pinned).  idx says which one of the kind.
enum ZkPinKind : uint8_t {
    ZK_PIN_OF_SLOT = 0,       // (a ZkMsmJob's default, never a buffer: the job's results go to MSM_SLOT / MSM_GROUP of its scratch slot)
    ZK_PIN_MSM_SLOT,          // idx = scratch slot: a job's reduce results
    ZK_PIN_MSM_GROUP,         // idx = scratch slot of the group's first job: a group's results
    ZK_PIN_BATCH_JOB,         // idx = position in a zk_msm_batch_dev call: the host reads them all at the end
    ZK_PIN_AHEAD,             // idx = k of a speculative (msm_host.hip) or started-ahead (msm_batch.hip) MSM: see ZK_SLOT_AHEAD
    ZK_PIN_FRONT,             // idx = parity: B in G2 of a chained front (groth16_pipeline.hip)
    ZK_PIN_FRONT_GROUP,       // idx = parity: the G1 group of a chained front
    ZK_PIN_MULTI_Z,           // groth16_multi.hip: the assignment staged for the other devices
    ZK_PIN_STRIDED_UPLOAD,    // msm.hip: a strided host table gathered into the packed form
    ZK_PIN_INV_TOTALS,        // poly.hip: the block totals of a batch inversion
    ZK_PIN_ZERO_VERDICTS,     // vec_ops.hip: the verdicts of zk_fr_vec_is_zero_launch
    ZK_PIN_MARLIN_BATCH,      // marlin_prove_batch.hip: idx 0 = what a step uploads (ZkStage), 1 = what it reads back
};

// The MSM scratch slots: the `slot` of zk_msm_prepare names the "msm_*.<slot>" scratch buffers, and two jobs on one slot share every
// sort and reduce buffer.  A range's users leave nothing in flight when they return unless it says so here.
enum ZkMsmSlot : int {
    ZK_SLOT_RUN = 0,          // (1) zk_msm_run and the host-slice calls' own job: synchronous, one at a time
    // (5) the Groth16 pipeline: the z jobs and H (ZkG16Jobs: slot0 + k).  A presort / begun set / front may be in flight between two calls
    // (ctx->flight).  zk_msm_batch_dev rotates its jobs over the first four of these and therefore drops a pending flight first.
    ZK_SLOT_G16 = 1,
    // (2) MSMs that run beside the caller's own calls: the speculation of the host-slice path (msm_host.hip) and the started-ahead MSMs of
    // zk_marlin_prove (msm_batch.hip), in flight beside jobs of ZK_SLOT_RUN and of zk_msm_batch_dev.  The two share the slots and
    // ZK_PIN_AHEAD because they never coexist: zk_msm_early_begin drops the speculation, nothing starts one until the prover has
    // collected or abandoned its early jobs (only the host-slice entry points speculate; the prover calls none), and the
    // speculation drops itself before its next start.
    ZK_SLOT_AHEAD = 6,
    // (5) the batch prover's five multi-vector jobs (groth16_batch.hip); zk_msm_multi_dev's one job takes the first: both synchronous
    ZK_SLOT_G16_BATCH = 8,
    ZK_SLOT_END = 13,
};
constexpr int ZK_SLOT_G16_COUNT = 5, ZK_SLOT_AHEAD_COUNT = 2;
static_assert(ZK_SLOT_RUN + 1 <= ZK_SLOT_G16 && ZK_SLOT_G16 + ZK_SLOT_G16_COUNT <= ZK_SLOT_AHEAD &&
              ZK_SLOT_AHEAD + ZK_SLOT_AHEAD_COUNT <= ZK_SLOT_G16_BATCH && ZK_SLOT_G16_BATCH + ZK_SLOT_G16_COUNT <= ZK_SLOT_END,
              "the MSM scratch slot ranges overlap");

// What a finished sort leaves for the accumulate kernel and the reduce chain (msm_digits.cuh has the two descriptors).  A job that
// borrows another job's sort takes the whole set.
struct ZkSortProducts {
    uint32_t *sorted = nullptr, *order = nullptr, *ctr = nullptr;
    SegDesc* desc = nullptr;
    HeavyDesc *heavy = nullptr, *heavy2 = nullptr;
};

// An MSM in flight (msm.hip): prepare -> enqueue_sort -> enqueue_accum -> enqueue_reduce -> finish.  Each enqueue ends by setting
// the job's mark of that stage (stream_order.hpp: ZkStageMark) on its stream -- sorted_at once the sort products are final,
// accumulated_at behind the accumulate kernel, reduced_at behind the copy of the partial sums to the host -- and whoever needs a
// stage done calls the mark's order(st): a wait, or nothing where st is the mark's own stream.  The job owns its events and
// timers: it moves, it does not copy.
struct ZkMsmJob {
    int group = 1, slot = 0;
    ZkPin pin = {ZK_PIN_OF_SLOT, 0};  // pinned result buffer; OF_SLOT: the slot's.  Jobs enqueued without a host wait in between need their own
    size_t n = 0, max_segs = 0, max_heavy = 0;
    uint32_t c = 0, W = 0, NB = 0, seg = 0;
    uint16_t off[65] = {0};           // window w covers scalar bits [off[w], off[w+1])
    uint32_t Wb = 0;                  // bucket sets: W, or 1 when the bases carry precomputed window multiples
    uint32_t log_nb = 0, nout = 0;    // reduce phase (msm_reduce.cuh): a window of 2^log_nb buckets leaves nout = log_nb + 1 points for the host
    // shifted multiples (zk_bases::pre_levels): M levels above the table, NB = (2^M + 1) 2^log_nb compact buckets that the reduce
    // takes as red_win = 2^M + 1 windows per bucket set; lvl_stride = table entries between two levels
    uint32_t M = 0, red_win = 1, lvl_stride = 0;
    uint32_t n_tab = 0, tab_off = 0;  // merged mode: table stride and offset of this MSM's first base
    uint32_t stride = 0;              // 32-bit words between consecutive points of bases_dev (the packed 2 * WORDS, or zk_bases::pre_stride)
    const uint32_t* bases_dev = nullptr;
    const void* scalars = nullptr;
    ZkStageMark sorted_at, accumulated_at;
    ZkStageMark reduced_at;           // what finish() waits for (its stream: where the reduce chain and the copy to hw are)
    uint32_t* hw = nullptr;           // partial window sums (XYZZ, internal form) in pinned host memory
    ZkSortProducts sort;              // kept so that a later job over the same scalar vector can reuse them
    size_t max_heavy2 = 0, max_heavy_segs = 0, max_groups = 0;
    std::vector<std::unique_ptr<ZkPhaseTimer>> timers;      // one per stage enqueued (a group's: on its first job); finish() resolves them
    ZkPhaseTimer* add_timer(zk_ctx* ctx, hipStream_t st) { timers.push_back(std::make_unique<ZkPhaseTimer>(ctx, st)); return timers.back().get(); }
    // several scalar vectors over one table (zk_msm_prepare_multi): n = mcount * mn scalars, vector k at scalars + k * mstride
    // elements; Wb = mcount bucket sets of the vector's geometry back to back
    size_t mcount = 0, mn = 0, mstride = 0;
    // zk_diag_msm_plans: the choices made for this job (table, sort, accumulate, fold, reduce), each stored by the code that makes it;
    // the enqueue of the reduce chain adds the geometry and commits the record to the context's ring (msm.hip: msm_plan_commit)
    zk_msm_plan plan = {};
};
static_assert(!std::is_copy_constructible<ZkMsmJob>::value && std::is_move_constructible<ZkMsmJob>::value, "a ZkMsmJob owns its events and timers");
int zk_msm_prepare(zk_ctx* ctx, ZkMsmJob* job, const zk_bases* bases, size_t base_offset, const void* scalars_dev, size_t n, int slot);
int zk_msm_enqueue_sort(zk_ctx* ctx, ZkMsmJob* job, hipStream_t st, const ZkMsmJob* share_sort);
int zk_msm_enqueue_accum(zk_ctx* ctx, ZkMsmJob* job, hipStream_t st);
int zk_msm_enqueue_reduce(zk_ctx* ctx, ZkMsmJob* job, hipStream_t st);
int zk_msm_finish(zk_ctx* ctx, ZkMsmJob* job, void* out_host_projective);
// count vectors of n scalars (stride elements apart) over one table as ONE job: the same launches as one MSM whatever count is.
// Callers keep count * buckets per vector within zk_msm_multi_chunk.  finish_multi writes count projective points.
int zk_msm_prepare_multi(zk_ctx* ctx, ZkMsmJob* job, const zk_bases* bases, size_t base_offset, const void* scalars_dev, size_t n,
                         size_t stride, size_t count, int slot);
size_t zk_msm_multi_chunk(const zk_bases* bases, size_t n);      // vectors of n scalars one multi job takes at most
int zk_msm_finish_multi(zk_ctx* ctx, ZkMsmJob* job, void* outs_host_projective);
// Several SMALL G1 jobs (sorted already, tables of window multiples with the same bucket count) as one accumulate launch and one
// launch per level of the reduce chain; zk_msm_group_ok says whether a set qualifies (else: the per-job calls above)
int zk_msm_finish_many(zk_ctx* ctx, ZkMsmJob* const* jobs, void* const* outs, int count);      // the host halves side by side
bool zk_msm_group_ok(ZkMsmJob* const* jobs, int count);
// (the sorts of such a group as ONE launch, a block per job: every job a one-block sort -- prepared, not yet sorted)
bool zk_msm_sort_group_ok(ZkMsmJob* const* jobs, int count);
int zk_msm_enqueue_sort_group(zk_ctx* ctx, ZkMsmJob* const* jobs, int count, hipStream_t st);
int zk_msm_enqueue_accum_group(zk_ctx* ctx, ZkMsmJob* const* jobs, int count, hipStream_t st);
int zk_msm_enqueue_reduce_group(zk_ctx* ctx, ZkMsmJob* const* jobs, int count, hipStream_t st);

// msm_batch.hip: one or two MSMs over one scalar vector started ahead of a batch (Marlin: the oracles of a round that exist early)
struct ZkEarlyMsm;
int zk_msm_early_begin(zk_ctx* ctx, int count, const zk_bases* bases, const size_t* base_offsets, const void* scalars_dev, size_t len, ZkEarlyMsm** out);
int zk_msm_early_finish(zk_ctx* ctx, ZkEarlyMsm* em, void* const* outs);      // outs = NULL: abandon (waits for its kernels); deletes the handle

// serialize.hip: GroupAffine::deserialize of n compressed points that are on the device already (no subgroup check: zk_subgroup_launch), table form out;
// bad_dev: one word, set if any x is off the curve; bad_each_dev (or NULL): one word per point.  And one point on the host.
int zk_decompress_launch(zk_ctx* ctx, int group, const uint32_t* in_dev, size_t n, uint32_t* out_dev, uint32_t* bad_dev, uint32_t* bad_each_dev);
bool zk_host_decompress_g1(const uint8_t in[48], zk::Affine<zk::G1Field>* out);
bool zk_host_decompress_g2(const uint8_t in[96], zk::Affine<zk::G2Field>* out);

// subgroup.hip: subgroup membership (subgroup.cuh: r P == O through the endomorphisms) of n points that are on the device already, table
// form, one point per lane.  bad_dev: one word, ORed with 1 if any point is outside; bad_each_dev (or NULL): one word per point, 1 =
// outside -- written, or with or_each ORed into what the word holds (the verifier's off-curve flags).  On ctx->stream, no wait.
int zk_subgroup_launch(zk_ctx* ctx, int group, const uint32_t* table_dev, size_t n, uint32_t* bad_dev, uint32_t* bad_each_dev, bool or_each = false);
bool zk_host_in_subgroup_g1(const zk::Affine<zk::G1Field>& p);      // ... and one point on the host (64-bit limbs)
bool zk_host_in_subgroup_g2(const zk::Affine<zk::G2Field>& p);

// pairing.hip: its kernels for every caller whose pairs are on the device already (its own entry points, groth16_verify.hip,
// marlin_verify.hip); on ctx->stream, no wait.  Lanes in one launch at most:
constexpr size_t ZK_PAIRING_MAX_LANES = (size_t)1 << 22;
// the scratch of n pairs: "pair_p" (n G1 points), "pair_q" (n G2 points), "pair_ml" (n Miller values); a NULL pointer skips its slot
int zk_pair_scratch(zk_ctx* ctx, size_t n, uint32_t** p_dev, uint32_t** q_dev, uint32_t** ml_dev);
// n pairs, table form (ext: the ABI's structs, Montgomery words of the reference) -> n Miller values, packed (pairing.cuh: FQ12_WORDS each)
int zk_miller_launch(zk_ctx* ctx, const uint32_t* p_dev, const uint32_t* q_dev, size_t n, uint32_t* ml_dev, bool ext = false);
// product k of `pairs` consecutive Miller values, k < count, through the final exponentiation.  gt_dev (or NULL): the GT values in the
// ABI's form.  ok_dev (or NULL): ok[k] = product k equals want_dev (packed, internal form) and bad_dev[k] (or NULL) is clear.
// want_slot_dev (or NULL): product k is held to value want_slot_dev[k] of want_dev instead of to its first one.
int zk_pairing_finish_launch(zk_ctx* ctx, const uint32_t* ml_dev, size_t pairs, size_t count, uint32_t* gt_dev, const uint32_t* want_dev,
                             const uint32_t* bad_dev, int* ok_dev, const uint32_t* want_slot_dev = nullptr);
// FE(the product of the n packed Miller values at ml_dev), n as large as a launch: folded on the device down to at most 64 partial
// products (k_fq12_fold), those copied back, their product and the final exponentiation on the host (pairing.cuh over Fq264Field).
// Waits for ctx->stream.  A caller that keeps timers passes both: with zk_set_profiling the fold launches go to tm as
// "<lap->prefix>k_fold", the wait for the partials and the host's part to lap as "wait_miller" and "host_finish".
// zk_fold_scratch: the fold's two buffers ("agg_fold_a" / "agg_fold_b") for n values.  zk_miller_product takes them itself; a caller
// with device work in flight by then reserves them beforehand (a = b = NULL), because a slot that has to grow waits for the stream.
namespace zk { template <class F2> struct Fq12; struct Fq264Field; }
int zk_fold_scratch(zk_ctx* ctx, size_t n, uint32_t** a_dev, uint32_t** b_dev);
int zk_miller_product(zk_ctx* ctx, const uint32_t* ml_dev, size_t n, zk::Fq12<zk::Fq264Field>* out, ZkPhaseTimer* tm = nullptr,
                      ZkHostLap* lap = nullptr);
// groth16_verify.hip: k_g1_scale_fold.  Lane g < n: point g in_step of `in` (affine table form, or XYZZ with in_xyzz) times the 128-bit
// coeffs[4 g ..] (NULL: times one); out_aff (or NULL): the n products as affine points; out_part (or NULL): one XYZZ sum per block of
// 64 lanes.  zk_g1_sum_down: the m XYZZ partials in a summed down to at most 64 (a and b: room for m and m / 64 + 1 points); *res says
// where they are.  Both on ctx->stream, no wait.
int zk_g1_scale_fold_launch(zk_ctx* ctx, const uint32_t* in, uint32_t in_step, bool in_xyzz, const uint32_t* coeffs, size_t n, uint32_t* out_aff,
                            uint32_t* out_part);
int zk_g1_sum_down(zk_ctx* ctx, uint32_t* a, uint32_t* b, size_t* m, uint32_t** res);
// g1_term_fold.hip: k_g1_term_fold, the sum of many G1 terms with FULL-WIDTH scalars, one term per lane.  Lane g < n: point g in_step of
// `in` (affine table form) times words[8 g ..] -- ZK_TERM_FULL: a raw 256-bit scalar, low word first, never reduced (any point);
// ZK_TERM_GLV: k1 | k2, four words each, for (k1 + k2 lambda) P through the endomorphism (points of the prime-order subgroup only).
// out_aff / out_part as above.  n <= 2^22.  On ctx->stream, no wait.  A mode that is not built: ZK_ERR_ARG.
enum ZkTermMode : int { ZK_TERM_FULL = 0, ZK_TERM_GLV = 1 };
// what zk_marlin_verify_aggregate runs: every point is in the subgroup by then, and the kernel alone is 1.44 - 1.48 times as fast as
// ZK_TERM_FULL at 13 328 and 213 008 lanes (DESIGN 6 "Aggregated Marlin verification")
constexpr int ZK_TERM_DEFAULT = ZK_TERM_GLV;
int zk_g1_term_fold_launch(zk_ctx* ctx, int mode, const uint32_t* in, uint32_t in_step, const uint32_t* words, size_t n, uint32_t* out_aff,
                           uint32_t* out_part);
// g1_lincomb.hip: n_segments short linear combinations of G1 points in one launch, one term per lane.  Lane g holds point
// point_index[g] of points_dev (table form; n_points of them) and the raw 256-bit scalar scalars_dev[8 g ..]; segment s is the lanes
// seg_offsets[s] .. seg_offsets[s + 1] - 1, which must lie in one wave of 64 (ZkLincombPack lays the lanes out so); seg_offsets[0] = 0,
// seg_offsets[n_segments] = n_lanes.  Out: segment s as an affine point (table form) and its infinity flag.  On st (NULL: ctx->stream), no wait.
int zk_g1_lincomb_launch(zk_ctx* ctx, const uint32_t* points_dev, size_t n_points, const uint32_t* point_index_dev, const uint32_t* scalars_dev,
                         const uint32_t* seg_offsets_dev, size_t n_segments, size_t n_lanes, uint32_t* out_affine_dev, uint32_t* out_is_inf_dev,
                         hipStream_t st = nullptr);
// The lane layout of such a launch, built on the host segment by segment: a segment that would straddle a wave starts the next one, and
// the lanes left over join the segment before them with a zero scalar.  add() refuses more than 64 terms.
struct ZkLincombPack {
    std::vector<uint32_t> point_index, scalars, seg_off;      // per lane; 8 words per lane; per segment (finish() appends the end)
    size_t lanes() const { return point_index.size(); }
    bool add(const uint32_t* idx, const uint32_t* k8, size_t len);
    void finish() { seg_off.push_back((uint32_t)lanes()); }
};

// fixed_base.hip: n G1 points XYZZ -> affine table form (Montgomery's trick; scr_dev: n Fq elements), on ctx->stream, no wait
int zk_g1_batch_affine_launch(zk_ctx* ctx, const uint32_t* in_xyzz_dev, uint32_t* out_affine_dev, uint32_t* scr_dev, size_t n);
// g1_ntt.hip: `count` radix-2 transforms of 2^log_n G1 points that share their twiddles, one butterfly per lane, log_n butterfly
// launches and one load launch whatever count is.  The input is affine (table form): vector v reads points in_dev[v in_vstride + i]
// for i < n_in and infinity beyond; with `scale` point i of vector v is first multiplied by the raw 256-bit scalar number
// scale->base[v] + i scale->step[v] of scale->k (count <= 2 then).  The result is left in work_xyzz_dev (count 2^log_n XYZZ points,
// vector after vector, natural order) for zk_g1_batch_affine_launch.  On ctx->stream, no wait.
struct ZkG1NttScale { const uint32_t* k; uint32_t base[2], step[2]; };
int zk_g1_ntt_twiddles(zk_ctx* ctx, uint32_t log_n, int inverse_root, const uint32_t** twiddles_dev);   // 2^(log_n - 1) raw scalars in the "g1ntt_tw" slot
int zk_g1_ntt_launch(zk_ctx* ctx, const uint32_t* in_dev, size_t n_in, size_t in_vstride, const ZkG1NttScale* scale, uint32_t log_n, size_t count,
                     const uint32_t* twiddles_dev, uint32_t* work_xyzz_dev);
int zk_g1_sub_launch(zk_ctx* ctx, const uint32_t* a_affine_dev, const uint32_t* b_affine_dev, uint32_t* out_xyzz_dev, size_t n);   // a[i] - b[i]

// msm_sort.hip: the bucket sort (msm_digits.cuh declares its interface)

// msm_g2pair.hip: the G2 accumulate kernel with two lanes per point addition
void zk_launch_accum_g2pair(hipStream_t st, size_t segments, const uint32_t* bases, const uint32_t* sorted, const SegDesc* desc,
                            const uint32_t* order, const uint32_t* ctr, uint32_t* sums, bool quads);
// test hooks (diag.hip): one small launch over a padded case array, the real device functions of the file that defines it.
// `lanes` is a whole number of waves; in / out hold in_w / out_w words per case (diag.hip documents the layouts).
void zk_diag_launch_fq2_pair(hipStream_t st, int op, const uint32_t* in, uint32_t* out, unsigned lanes);   // msm_g2pair.hip
void zk_diag_launch_g1_dual(hipStream_t st, int op, const uint32_t* in, uint32_t* out, unsigned lanes);    // msm.hip
void zk_diag_launch_f7l(hipStream_t st, int op, const uint32_t* in, uint32_t* out, unsigned lanes);        // she.hip
struct ZkG2PairReduce {   // the arguments of msm.hip's reduce chain
    const HeavyDesc *heavy, *heavy2; const uint32_t* ctr; uint32_t* done;
    uint32_t *sums, *rowP, *colP, *bits;
    uint32_t log_nb, n_win, light_blocks, heavy_blocks;
    bool quads = false;          // a small job: the fold on lane quads (the grid kernels choose by the bucket count)
    zk_msm_plan* plan = nullptr; // the job's record (zk_diag_msm_plans): the fold's lanes and the reduce policy are stored where they are chosen
};
int zk_launch_reduce_g2pair(zk_ctx* ctx, hipStream_t st, const ZkG2PairReduce& a);
constexpr uint32_t ZK_G2PAIR_RED_PTS = 128;   // points (lane pairs) per block of the G2 reduce kernels
