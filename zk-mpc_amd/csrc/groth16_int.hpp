// groth16_int.hpp -- what the Groth16 translation units share: the device-side constraint system and proving key, the state of a
// jobs of a proof that were enqueued ahead of it (ZkG16Flight), and the pipeline's internal entry points.
//   r1cs.hip             constraint system upload, sparse mat-vec, R1CStoQAP::witness_map          (src/groth16.rs:205-306)
//   groth16_key.hip      proving key upload / accessors, generate_parameters with known toxic waste (generator.rs:44-231)
//   key_io.hip           CanonicalSerialize framing of keys and SRS                                (data_structures.rs:133-151)
//   groth16_pipeline.hip the five MSMs of create_proof as a stream pipeline, fronts, presorts       (src/groth16.rs:106-160)
//   msm_batch.hip        several independent MSMs enqueued in one go (Marlin's commitment rounds)
//   groth16_prove.hip    create_proof for a local prover                                           (src/groth16.rs:68-183)
//   groth16_batch.hip    create_proof for many assignments of one key in one call
//   groth16_multi.hip    one prover's MSMs spread over several devices
//   groth16_shared.hip   create_proof over additive / SPDZ shares as one call (its host algebra: groth16_shared_int.hpp)
//   groth16_shared_batch.hip  the same for many shared assignments of one key, with the exchanges of one proof
//   groth16_verify.hip   Groth16::verify on the host, prepare_inputs, the staging of a batch's proofs        (verifier.rs:13-61)
//   groth16_verify_keys.hip  batches on the device, proof by proof or folded, over one key or several in one call
#pragma once
#include "hostfr.hpp"
#include "hostgroup.hpp"
#include "hostfield64.hpp"
#include "internal.hpp"
#include "pairing.cuh"
#include "../../include/zkmpc_hip.h"
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <vector>

struct zk_r1cs {
    size_t nc = 0, ni = 0, nw = 0;
    uint32_t log_d = 0;
    struct Mat {
        uint32_t* row_ptr = nullptr;
        uint32_t* col = nullptr;
        uint32_t* coeff = nullptr;  // nnz * 8 words, internal form
        size_t nnz = 0;
        bool all_one = false;       // every coefficient is 1: the product is skipped (src/groth16.rs:220-224)
        std::vector<uint32_t> h_row_ptr, h_col;
        std::vector<zk::Fr> h_coeff;    // internal form (empty when all_one)
    } m[3];
};

struct zk_pk {
    zk_bases *a = nullptr, *b_g1 = nullptr, *b_g2 = nullptr, *h = nullptr, *l = nullptr, *gamma_abc = nullptr;
    // l_query behind as many points at infinity as a_query has entries for the instance (l_pad[ni + j] = l[j]), so that the
    // L job indexes its table by the position in z like A and B do and reuses their sort of z[1..]; the instance part adds
    // infinity, which the complete addition skips.  Only the prover's pipeline reads it.
    zk_bases* l_pad = nullptr;
    // H over coset values: with e = a o b on the coset, sum_i h_i H_i = sum_j e_j H'_j - sum_k z_k K_k, where H' is the
    // transpose of coset_ifft and of the division by Z(g) applied to h_query, and K is h_query through the transposes of ifft and
    // of C.  h_eval = the D points H'_j; l_eval_pad = l_pad with L_k - K_k in the witness slots and -K_k in the instance slots
    // (slot 0, the constant's, is read by the proof tail: l_eval_0).  Built by zk_groth16_setup, where the trapdoor gives their
    // scalars; a key that was loaded has neither and its proofs take the quotient's coefficients over h_query as before.
    zk_bases *h_eval = nullptr, *l_eval_pad = nullptr;
    zk::Affine<zk::G1Field> l_eval_0;
    // every point is a multiple of the generators (zk_groth16_setup): the proof tail may use the endomorphism (hostfield64.hpp:
    // host64_scalar_mul_glv); a deserialised key is not checked for subgroup membership and keeps the plain scalar multiplication
    // (zk_pk_check_subgroups reports on a loaded key; it does not switch the key's proofs to another path)
    bool points_in_subgroup = false;
    // shifted copies of the window multiples its tables were asked to carry (zk_mul_levels_for_key; zk_bases::pre_levels is what each got)
    uint32_t mul_levels = 0;
    zk::Affine<zk::G1Field> alpha_g1, beta_g1, delta_g1, a0, b0_g1;
    zk::Affine<zk::G2Field> beta_g2, delta_g2, gamma_g2, b0_g2;
    // the verifier's view of this key (groth16_vkey.hip: zk_pk_vkey), made by the first verification through the key under this
    // mutex and freed with the key: the pk forms of the verifiers are the vkey forms on it
    mutable std::mutex vkey_mu;
    mutable zk_vkey* vkey = nullptr;
};

// arkworks' PreparedVerifyingKey (verifier.rs: prepare_verifying_key) resident on the device, and what prepare_inputs needs beyond it.
struct zk_vkey {
    zk::Affine<zk::G1Field> alpha_g1;
    zk::Affine<zk::G2Field> beta_g2, gamma_g2, delta_g2, neg_gamma_g2, neg_delta_g2;
    zk_bases* gamma_abc = nullptr;           // owned: ninp + 1 points, table form
    std::vector<uint32_t> abc_host;          // the same words on the host (the folded form's key multiplications, gamma_abc[0])
    // window multiples of gamma_abc[j], j >= 1 (g1_prepare_inputs.hip): entry ((j - 1) 64 + w) 8 + m - 1 = m 16^w gamma_abc[j], affine,
    // table form.  NULL: the key has no public input, or the table would be larger than the context's limit when the key was made
    // (zk_groth16_prepare_table_limit) -- then the sums go through the multi-vector MSM over gamma_abc.
    uint32_t* win = nullptr;
    bool points_in_subgroup = false;         // every point is known to be in its subgroup: the folded form's host multiplications take the endomorphism
    uint32_t e_alpha_beta[zk::FQ12_WORDS];   // e(alpha, beta) as the finish kernel compares it (12 Fq, internal form, packed)
    size_t ninp() const { return gamma_abc->n - 1; }
};
// groth16_vkey.hip.  zk_vkey_make: the object from its parts (g2s = beta, gamma, delta); abc is CONSUMED, on failure too.
// zk_pk_vkey: the key's own vkey, built on first use; `entry` names the caller in the refusal of a key without verifying-key parts.
int zk_vkey_make(zk_ctx* ctx, const zk::Affine<zk::G1Field>& alpha, const zk::Affine<zk::G2Field> g2s[3], zk_bases* abc, bool in_subgroup,
                 zk_vkey** out);
int zk_pk_vkey(zk_ctx* ctx, const zk_pk* pk, const char* entry, const zk_vkey** out);
// groth16_verify.hip: a host verifying key for ninp public inputs -- its parts there, gamma_abc of ninp + 1 points, every coordinate
// word below q (what zk_groth16_verify_host accepts)
bool zk_vk_host_ok(const zk_vk_host* vk, size_t ninp);
// g1_prepare_inputs.hip, on ctx->stream, no wait.  The table of a key's window multiples (abc_dev: ninp + 1 points; win_dev: ninp x
// ZK_PREP_ENTRIES points), one entry per lane; and prepare_inputs for count proofs: inputs_dev = count x ninp elements in the
// reference's form, digits_dev = room for as many recoded scalars (8 words each), out = count affine points and infinity flags.
// win_dev may be NULL when ninp = 0.
constexpr size_t ZK_PREP_WINDOWS = 64, ZK_PREP_ENTRIES = ZK_PREP_WINDOWS * 8;      // signed 4-bit digits: 64 windows x (1 .. 8) P
int zk_g1_window_table_launch(zk_ctx* ctx, const uint32_t* abc_dev, size_t ninp, uint32_t* win_dev);
int zk_g1_prepare_inputs_launch(zk_ctx* ctx, const uint32_t* inputs_dev, size_t count, size_t ninp, const uint32_t* win_dev, const uint32_t* abc_dev,
                                uint32_t* digits_dev, uint32_t* out_aff_dev, uint32_t* out_inf_dev);

// The five MSM jobs of ONE proof, in ZkG16Jobs order (0 = B in G2, 1 = A, 2 = B in G1, 3 = L, 4 = H), and how far each has been
// enqueued.  run_msms drives its own proof's flight through the stages; one that was started AHEAD of its proof is owned by the
// context (zk_ctx::flight) until run_msms takes it over or zk_presort_free drains and drops it:
//   at[0] == SORTED alone: a sort of z[1..] (shared by the B-in-G2 / A / B-in-G1 / L jobs).  The collaborative prover calls zk_groth16_
//     msms_presort_dev right after the local half of the witness map: the sort runs under the Beaver open, not in front of the first accumulate.
//   at[0] == REDUCED, at[1..3] == ACCUMULATED (zk_groth16_msms_begin_dev): not only the sort of z but the four MSMs over z are under
//     way; zk_groth16_msms_dev then adds the H job and collects all five.  The collaborative prover calls it before its Beaver open:
//     the exchange and the second half of the witness map run under 12 ms of accumulate kernels that do not need h.
//   at[0] == SORTED, at[4] == SORTED, h and wm_done set: the whole FRONT of the next local proof (zk_groth16_hint_next_dev) --
//     besides the sort of z also its witness map and the H job's sort, enqueued behind the current proof's last kernels so that
//     they run under its reduce tail and the host time between two proofs.
//   all five REDUCED: a SMALL local proof's front carries its whole device chain -- besides the sorts and the witness map also the
//     accumulate launches and reduce chains of all five jobs are enqueued behind the current proof's; the device goes from one
//     proof's chain into the next while the host still finishes the first.
struct ZkG16Flight {
    const zk_pk* pk; const zk_r1cs* r; const void* z;      // whose proof
    void* h;                           // where its witness map wrote (NULL: none ran; the caller brings h)
    ZkMsmJob J[5];
    ZkMsmJob* const g1[4] = {&J[1], &J[2], &J[3], &J[4]};      // the four G1 jobs, as the group calls take them
    enum Stage : uint8_t { NONE, SORTED, ACCUMULATED, REDUCED } at[5] = {NONE, NONE, NONE, NONE, NONE};
    ZkEvent wm_done;                   // recorded behind the witness map: gates the first accumulate kernel (and a late sort of L)
    bool grouped = false;              // jobs 1..4 go / went out as one group launch
    bool beyond_sort_z() const { return at[1] || at[2] || at[3] || at[4]; }      // (then zk_presort_free drains more than the sort stream)
    ZkG16Flight(const zk_pk* pk_, const zk_r1cs* r_, const void* z_, void* h_) : pk(pk_), r(r_), z(z_), h(h_) {}
    ZkG16Flight(const ZkG16Flight&) = delete; ZkG16Flight& operator=(const ZkG16Flight&) = delete;      // (g1 points into this object)
};

// the context's helper streams: aux[0..k) and the accumulate stream (created on first use)
int zk_prover_streams(zk_ctx* ctx, size_t k);
// The five MSMs of create_proof as one pipeline (groth16_pipeline.hip).  h_in: the quotient's coefficients when the caller has them
// (the collaborative provers), else NULL and the witness map runs here into h_scratch.  out_g1 = H, L, A, B-in-G1 sums;
// after_abc runs on the calling thread as soon as A, B-in-G1 and B-in-G2 have delivered.
int zk_groth16_run_msms(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* z, const void* h_in, void* h_scratch,
                        zk_g1_projective out_g1[4], zk_g2_projective* out_g2, const std::function<void()>& after_abc = nullptr);
int zk_pk_make_l_pad(zk_ctx* ctx, zk_pk* pk);     // groth16_key.hip: see zk_pk::l_pad
int zk_pk_precompute(zk_ctx* ctx, zk_pk* pk);     // groth16_key.hip: window multiples of every query, then l_pad
// ZK_G16_EVAL_H=0 in the environment (read once): no key gets h_eval / l_eval_pad and no prover reads them
inline bool zk_g16_eval_h_enabled() {
    static const bool on = [] { const char* e = getenv("ZK_G16_EVAL_H"); return !(e && *e && atoi(e) == 0); }();
    return on;
}
// r1cs.hip: the witness map of count assignments (count x m elements back to back) with launches that do not grow with count;
// abc = room for 6 count D elements, the count quotients in its first count D on return
int zk_groth16_witness_map_batch(zk_ctx* ctx, const zk_r1cs* r, size_t count, const void* z, void* abc);
// ... and its two halves, between which it multiplies (the collaborative batch prover puts the Beaver product there): pre leaves
// abc = a | b on the coset and c in coefficient form (tmp: 3 count D elements of scratch), post turns the count products into the
// count quotients (tmp: count D elements)
int zk_groth16_witness_map_batch_pre(zk_ctx* ctx, const zk_r1cs* r, size_t count, const void* z, void* abc, void* tmp);
int zk_groth16_witness_map_batch_post(zk_ctx* ctx, const zk_r1cs* r, size_t count, void* ab, const void* c, void* tmp);
// r1cs.hip: the witness map that ends at e = a o b on the coset (two mat-vecs, ifft and coset_fft of a and b, the product): what the
// H job of a key with h_eval multiplies (zk_pk::h_eval).  The batch form takes the same abc and leaves the count e vectors in its
// first count D elements.
int zk_groth16_witness_map_eval_dev(zk_ctx* ctx, const zk_r1cs* r, const void* z, void* e);
int zk_groth16_witness_map_eval_batch(zk_ctx* ctx, const zk_r1cs* r, size_t count, const void* z, void* abc);
// every prover's check of the key against the system (groth16_pipeline.hip): the tables there, an instance, the four lengths
int zk_groth16_key_matches(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r);
int zk_next_z_drop(zk_ctx* ctx, bool drain);      // groth16_pipeline.hip: forget an announced next assignment (drain: its front and upload first)
// groth16_pipeline.hip: z was produced on the context stream -- the waiters go on behind what that stream carries now
int zk_behind_context_stream(zk_ctx* ctx, const hipStream_t* waiters, int count);

// The one statement of the five MSMs of create_proof (src/groth16.rs:160, :137, :148, :110, :106), in the fixed order 0 = B in G2, 1 = A,
// 2 = B in G1, 3 = L, 4 = H: every prover reads its tables, offsets, scalars and lengths here.  z, h may be NULL where only the
// lengths are wanted.  pad_l = false keeps L on l_query (the several-device prover cuts it by terms of the witness part).
// The table also says WHICH witness map feeds job 4: with eval_h (a key with h_eval / l_eval_pad, the environment not against it, L
// padded, and the caller not bringing a quotient of its own: quotient_given) job 4 is h_eval over the coset values e, job 3 is
// l_eval_pad and the tail adds l_const; witness_map / witness_map_batch run the map that goes with the jobs.
struct ZkG16Jobs {
    struct Job {
        const zk_bases* tab;
        size_t off;             // first base
        const char* scal;
        size_t n;
    } j[5];
    size_t m, D;                // elements between two assignments / two quotients of a batch
    bool l_shared;              // L over l_pad reads z[1..] like jobs 0..2 (the instance meets infinity) and borrows their sort
    bool eval_h;                // job 4 = h_eval x e, job 3 = l_eval_pad x z[1..] (sharing the sort as l_pad does)
    const zk::Affine<zk::G1Field>* l_const = nullptr;      // eval_h: -K_0, the constant variable's term of L, for zk_tail_finish
    const zk_r1cs* r;
    ZkG16Jobs(const zk_pk* pk, const zk_r1cs* r_, const void* z, const void* h, bool pad_l = true, bool quotient_given = false)
        : m(r_->ni + r_->nw), D((size_t)1 << r_->log_d), r(r_) {
        const size_t nvars = m - 1;
        const char *z1 = z ? (const char*)z + 32 : nullptr, *zw = z ? (const char*)z + r->ni * 32 : nullptr;
        auto like_a = [&](const zk_bases* t) {
            return t && t->n == nvars + 1 && (t->pre != nullptr) == (pk->a->pre != nullptr) && t->c_pre == pk->a->c_pre && t->pre_levels == pk->a->pre_levels;
        };
        l_shared = pad_l && like_a(pk->l_pad);
        eval_h = pad_l && !quotient_given && zk_g16_eval_h_enabled() && pk->h_eval && pk->h_eval->n == D && like_a(pk->l_eval_pad);
        j[0] = {pk->b_g2, 1, z1, nvars};        // query[1..] x z[1..]
        j[1] = {pk->a, 1, z1, nvars};
        j[2] = {pk->b_g1, 1, z1, nvars};
        j[3] = l_shared ? Job{pk->l_pad, 1, z1, nvars} : Job{pk->l, 0, zw, r->nw};        // aux_assignment against l_query
        j[4] = {pk->h, 0, (const char*)h, std::min(pk->h->n, D)};        // min(len) rule (variable_base.rs:15-17): h_query has D-1 entries, h has D
        if (eval_h) {
            l_shared = true;
            j[3] = {pk->l_eval_pad, 1, z1, nvars};
            j[4] = {pk->h_eval, 0, (const char*)h, D};
            l_const = &pk->l_eval_0;
        }
    }
    // the witness map whose output job 4 reads, into h (one proof) or into abc (count proofs: zk_groth16_witness_map_batch's layout)
    int witness_map(zk_ctx* ctx, const void* z, void* h) const {
        return eval_h ? zk_groth16_witness_map_eval_dev(ctx, r, z, h) : zk_groth16_witness_map_dev(ctx, r, z, h);
    }
    int witness_map_batch(zk_ctx* ctx, size_t count, const void* z, void* abc) const {
        return eval_h ? zk_groth16_witness_map_eval_batch(ctx, r, count, z, abc) : zk_groth16_witness_map_batch(ctx, r, count, z, abc);
    }
    // job k into scratch slot slot0 + k: of one proof (multi = 0), or as a multi-vector job of `multi` >= 1 proofs (assignments m,
    // quotients D elements apart; a batch's last chunk may be one proof and is collected as a multi job all the same)
    int prepare(zk_ctx* ctx, int k, ZkMsmJob* job, ZkMsmSlot slot0, size_t multi = 0) const {
        if (!multi) return zk_msm_prepare(ctx, job, j[k].tab, j[k].off, j[k].scal, j[k].n, slot0 + k);
        return zk_msm_prepare_multi(ctx, job, j[k].tab, j[k].off, j[k].scal, j[k].n, k == 4 ? D : m, multi, slot0 + k);
    }
    // The z jobs J[0..3] prepared and their sorts enqueued on st: job 0 sorts, A borrows its sort, B in G1 and a
    // shared L borrow from the lender.  have0: J[0] is prepared and sorted already; njobs = 1: job 0 alone.  An L of its own is sorted by the caller.
    int sort_z(zk_ctx* ctx, ZkMsmJob* J, hipStream_t st, ZkMsmSlot slot0, size_t multi = 0, bool have0 = false, int njobs = 4) const {
        for (int k = have0 ? 1 : 0; k < njobs; k++) ZK_TRY(prepare(ctx, k, &J[k], slot0, multi));
        if (!have0) ZK_TRY(zk_msm_enqueue_sort(ctx, &J[0], st, nullptr));
        if (njobs == 1) return ZK_OK;
        ZK_TRY(zk_msm_enqueue_sort(ctx, &J[1], st, &J[0]));
        // (the G2 table may carry windows of another width than the G1 tables: then A sorts for itself and the other G1 jobs borrow A's)
        const ZkMsmJob* lender = J[0].c == J[1].c ? &J[0] : &J[1];
        ZK_TRY(zk_msm_enqueue_sort(ctx, &J[2], st, lender));
        return l_shared ? zk_msm_enqueue_sort(ctx, &J[3], st, lender) : ZK_OK;
    }
};

// The O(1) host tail of a proof (groth16_prove.hip), cut where it can be scheduled: three terms that need only the key and r, s;
// three chains that need the A, B-in-G1 and B-in-G2 sums; the finish.  Every proof of the library is these functions.
struct ZkTail {
    using X1 = zk::XYZZ<zk::Fq64Field>;
    uint32_t rw[8], sw[8];
    X1 r_g1, r_s_delta, s_g1;                        // delta r, delta r s, delta s
    zk::XYZZ<zk::Fq264Field> s_g2;                   // delta_2 s
    X1 g_a, s_g_a, r_g1_b;
    zk::Affine<zk::Fq264Field> b_aff;
};
void zk_tail_begin(const zk_fr* r, const zk_fr* s, ZkTail* t);
void zk_tail_pre_a(const zk_pk* pk, ZkTail* t);      // independent of each other
void zk_tail_pre_b(const zk_pk* pk, ZkTail* t);
void zk_tail_pre_2(const zk_pk* pk, ZkTail* t);
void zk_tail_chain_a(const zk_pk* pk, ZkTail* t, const zk_g1_projective& a_sum);       // after pre_a
void zk_tail_chain_b(const zk_pk* pk, ZkTail* t, const zk_g1_projective& b1_sum);      // after pre_b
void zk_tail_chain_2(const zk_pk* pk, ZkTail* t, const zk_g2_projective& b2_sum);      // after pre_2
// (l_const: ZkG16Jobs::l_const of the table the sums came from, NULL without)
void zk_tail_finish(const ZkTail& t, const zk_g1_projective& h_sum, const zk_g1_projective& l_sum, uint8_t proof[192],
                    const zk::Affine<zk::G1Field>* l_const = nullptr);

// The tail of a single proof: the pre terms start with the proof on the context's helper threads, under the device's work; the chains
// as soon as A, B-in-G1 and B-in-G2 have delivered (abc_ready), while the devices still work on L and H.  The tasks reference this
// object: declare it after the MSM sums it reads; the destructor joins.  (A batch runs the same functions over ranges of proofs.)
class ZkProofTail {
    zk_ctx* ctx;
    const zk_pk* pk;
    ZkTail t;
    ZkTask<void> pre_a, pre_b, pre_2;                // (the chains wait for them; declared first = joined last)
    ZkTask<void> chain_a, chain_b, chain_g2;         // (last members: joined before the fields the chains write go)

   public:
    ZkProofTail(zk_ctx* c, const zk_pk* pk, const zk_fr* r_, const zk_fr* s_);
    void abc_ready(const zk_g1_projective& a_sum, const zk_g1_projective& b1_sum, const zk_g2_projective& b2_sum);
    void join();
    void finish(const zk_g1_projective& h_sum, const zk_g1_projective& l_sum, uint8_t proof[192], const zk::Affine<zk::G1Field>* l_const = nullptr);
};

// ---- what the batch provers share (groth16_batch.hip, groth16_shared_batch.hip) ----
// f(lo, hi) over [0, count) in at most `tasks` contiguous ranges on the context's pool (the first range on this thread)
template <class Fn>
void zk_over_ranges(zk_ctx* ctx, size_t count, size_t tasks, const Fn& f) {
    const size_t nt = std::min(count, tasks), per = (count + nt - 1) / nt;
    std::vector<ZkTask<void>> ts;
    for (size_t t = 1; t < nt; t++) {
        const size_t lo = t * per, hi = std::min(count, lo + per);
        if (lo < hi) ts.push_back(zk_async(ctx, [&f, lo, hi] { f(lo, hi); }));
    }
    f(0, std::min(count, per));
    for (auto& t : ts) t.get();
}
// a device allocation of this call only (a batch's buffers grow with count: not kept in the context's grow-only scratch arena)
struct ZkCallMem {
    zk_ctx* ctx;
    void* p = nullptr;
    ~ZkCallMem() {
        if (!p) return;
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(p);
    }
};
// groth16_batch.hip: the proofs per MSM chunk of a batch of count (every job's bucket spaces within what one multi job takes) and
// the device bytes the five jobs of one such chunk need; quotient_given as in ZkG16Jobs
void zk_g16_batch_chunk(const zk_pk* pk, const zk_r1cs* r, size_t count, bool quotient_given, size_t* chunk, size_t* chunk_bytes);
// The batch provers' memory rule: count * per_proof bytes of buffers and one chunk's MSM scratch against 90 % of the free device
// memory -- otherwise ZK_ERR_NOMEM, before any device work
int zk_g16_batch_fits(zk_ctx* ctx, size_t count, double per_proof, size_t chunk_bytes);

// ---- the ABI's affine structs (x | y in the reference's Montgomery words) and its GT value as host-field values (valid words:
// zk_words_below_q) ----
inline zk::Affine<zk::Fq64Field> zk_host_g1(const zk_g1_affine* p) {
    return zk::Affine<zk::Fq64Field>{zk::host64_coord<zk::Fq64Field>(p->x.l), zk::host64_coord<zk::Fq64Field>(p->y.l)};
}
inline zk::Fq12<zk::Fq264Field> zk_host_gt(const zk_gt* g) {
    uint32_t w[zk::FQ12_WORDS];
    memcpy(w, g, sizeof w);
    return zk::fq12_from_ext<zk::Fq264Field>(w);
}
inline void zk_host_gt_out(zk_gt* g, const zk::Fq12<zk::Fq264Field>& f) {
    uint32_t w[zk::FQ12_WORDS];
    zk::fq12_to_ext<zk::Fq264Field>(w, f);
    memcpy(g, w, sizeof w);
}
inline zk::Affine<zk::Fq264Field> zk_host_g2(const zk_g2_affine* p) {
    return zk::Affine<zk::Fq264Field>{zk::host64_coord<zk::Fq264Field>((const uint64_t*)p->x), zk::host64_coord<zk::Fq264Field>((const uint64_t*)p->y)};
}

namespace zk {
template <class F>
inline int first_point(zk_ctx* ctx, const zk_bases* b, Affine<F>* out) {
    if (!b || b->n == 0) { *out = aff_inf<F>(); return ZK_OK; }
    uint32_t w[2 * F::WORDS];
    ZK_HIP(ctx, hipMemcpy(w, b->dev, sizeof w, hipMemcpyDeviceToHost));
    *out = aff_load<F>(w);
    return ZK_OK;
}

}  // namespace zk
