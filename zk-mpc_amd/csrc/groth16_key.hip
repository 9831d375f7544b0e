// groth16_key.hip -- the proving key on the device: upload, accessors, and generate_parameters with explicit toxic waste.
//
// Replaces (reference):
//   generate_parameters                               arkworks/groth16/src/generator.rs:44-231
//   R1CStoQAP::instance_map_with_evaluation           arkworks/groth16/src/r1cs_to_qap.rs:47-92
//   ProvingKey / VerifyingKey                         arkworks/groth16/src/data_structures.rs:10-151
// The proving key's five queries are zk_bases tables (resident, with window multiples from 2^16 points on).
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "g1_lincomb.cuh"

using namespace zk;

namespace {

// upload a host vector of internal-form Fr as reference-form device vector
int upload_fr(zk_ctx* ctx, const std::vector<HF>& v, const char* slot, void** dev) {
    std::vector<uint32_t> packed(v.size() * 8 + 8);
    for (size_t i = 0; i < v.size(); i++) fp_pack<FrParams>(&packed[8 * i], fp_int_to_ext<FrParams>(v[i].v));
    ZK_TRY(zk_scratch(ctx, slot, v.size() * 32 + 32, dev));
    ZK_HIP(ctx, hipMemcpyAsync(*dev, packed.data(), v.size() * 32, hipMemcpyHostToDevice, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

template <class F>
Affine<F> host_gen_mul(const Affine<F>& g, const HF& k) {
    uint32_t kw[8];
    k.canon_words(kw);
    return xyzz_to_affine<F>(xyzz_scalar_mul<F>(g, kw, 8));
}

Affine<G1Field> g1_gen() { return Affine<G1Field>{fp_const<FqParams>(FqParams::G1_GEN_X), fp_const<FqParams>(FqParams::G1_GEN_Y)}; }
Affine<G2Field> g2_gen() {
    return Affine<G2Field>{Fq2{fp_const<FqParams>(FqParams::G2_GEN_X0), fp_const<FqParams>(FqParams::G2_GEN_X1)},
                           Fq2{fp_const<FqParams>(FqParams::G2_GEN_Y0), fp_const<FqParams>(FqParams::G2_GEN_Y1)}};
}

}  // namespace

// see zk_pk::l_pad
int zk_pk_make_l_pad(zk_ctx* ctx, zk_pk* pk) {
    if (!pk->a || !pk->l || pk->l->n == 0 || pk->a->n <= pk->l->n) return ZK_OK;
    const size_t n = pk->a->n, front = n - pk->l->n, PW = 2 * G1Field::WORDS * 4;
    zk_bases* b = new zk_bases();
    b->group = 1;
    b->n = n;
    if (hipMalloc((void**)&b->dev, n * PW) != hipSuccess) { delete b; (void)hipGetLastError(); return ZK_OK; }   // no memory: L keeps its own sort
    pk->l_pad = b;
    ZK_HIP(ctx, hipMemsetAsync(b->dev, 0, front * PW, ctx->stream));
    ZK_HIP(ctx, hipMemcpyAsync((char*)b->dev + front * PW, pk->l->dev, pk->l->n * PW, hipMemcpyDeviceToDevice, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return zk_bases_precompute_levels(ctx, b, pk->mul_levels);
}

// The window multiples of the five queries and the padded l_query, with the key's shifted copies (zk_pk::mul_levels): every way a key
// becomes resident (upload, setup, deserialize) ends here
int zk_pk_precompute(zk_ctx* ctx, zk_pk* pk) {
    pk->mul_levels = pk->a ? zk_mul_levels_for_key(ctx, pk->a->n) : 0;
    for (zk_bases* q : {pk->a, pk->b_g1, pk->b_g2, pk->h, pk->l, pk->h_eval, pk->l_eval_pad}) ZK_TRY(zk_bases_precompute_levels(ctx, q, pk->mul_levels));
    return zk_pk_make_l_pad(ctx, pk);
}
extern "C" int zk_pk_eval_h(const zk_pk* pk, const zk_r1cs* r) {
    ZK_API_BEGIN_NOCTX
    return pk && r && pk->a && pk->h && pk->l && r->ni + r->nw == pk->a->n && ZkG16Jobs(pk, r, nullptr, nullptr).eval_h ? 1 : 0;
    ZK_API_END
}
extern "C" uint32_t zk_pk_mul_levels(const zk_pk* pk) { return pk && pk->a ? pk->a->pre_levels : 0u; }
extern "C" int zk_msm_mul_levels(zk_ctx* ctx, int levels) {
    ZK_API_BEGIN(ctx)
    if (!ctx || levels < -1 || levels > (int)ZK_MSM_MAX_LEVELS) return ZK_ERR_ARG;
    ctx->mul_levels = levels;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_pk_free(zk_ctx* ctx, zk_pk* pk) {
    ZK_API_BEGIN(ctx)
    if (!pk) return ZK_OK;
    // a pending presort / front (ZkG16Flight) is matched by address: it must not outlive the objects it points to, or a new
    // key allocated at the same address would adopt a sort of the old key's tables
    zk_presort_free(ctx);
    zk_bases* all[9] = {pk->a, pk->b_g1, pk->b_g2, pk->h, pk->l, pk->gamma_abc, pk->l_pad, pk->h_eval, pk->l_eval_pad};
    for (auto* b : all) zk_bases_free(ctx, b);
    zk_vkey_free(ctx, pk->vkey);
    delete pk;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_pk_upload(zk_ctx* ctx, const zk_pk_host* h, zk_pk** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !h || !out) return ZK_ERR_ARG;
    zk_pk* pk = new zk_pk();
    int rc = zk_bases_upload_g1(ctx, h->a_query, h->a_len, &pk->a);
    if (rc == ZK_OK) rc = zk_bases_upload_g1(ctx, h->b_g1_query, h->b_g1_len, &pk->b_g1);
    if (rc == ZK_OK) rc = zk_bases_upload_g2(ctx, h->b_g2_query, h->b_g2_len, &pk->b_g2);
    if (rc == ZK_OK) rc = zk_bases_upload_g1(ctx, h->h_query, h->h_len, &pk->h);
    if (rc == ZK_OK) rc = zk_bases_upload_g1(ctx, h->l_query, h->l_len, &pk->l);
    if (rc == ZK_OK) rc = zk_pk_precompute(ctx, pk);
    if (rc != ZK_OK) { zk_pk_free(ctx, pk); return rc; }
    pk->alpha_g1 = host_aff_from_abi<G1Field>((const uint64_t*)&h->alpha_g1);
    pk->beta_g1 = host_aff_from_abi<G1Field>((const uint64_t*)&h->beta_g1);
    pk->delta_g1 = host_aff_from_abi<G1Field>((const uint64_t*)&h->delta_g1);
    pk->beta_g2 = host_aff_from_abi<G2Field>((const uint64_t*)&h->beta_g2);
    pk->delta_g2 = host_aff_from_abi<G2Field>((const uint64_t*)&h->delta_g2);
    pk->gamma_g2 = aff_inf<G2Field>();
    pk->a0 = h->a_len ? host_aff_from_abi<G1Field>((const uint64_t*)&h->a_query[0]) : aff_inf<G1Field>();
    pk->b0_g1 = h->b_g1_len ? host_aff_from_abi<G1Field>((const uint64_t*)&h->b_g1_query[0]) : aff_inf<G1Field>();
    pk->b0_g2 = h->b_g2_len ? host_aff_from_abi<G2Field>((const uint64_t*)&h->b_g2_query[0]) : aff_inf<G2Field>();
    *out = pk;
    return ZK_OK;
    ZK_API_END
}

extern "C" size_t zk_pk_query_len(const zk_pk* pk, int which) {
    if (!pk) return 0;
    const zk_bases* all[6] = {pk->a, pk->b_g1, pk->b_g2, pk->h, pk->l, pk->gamma_abc};
    return (which >= 0 && which < 6 && all[which]) ? all[which]->n : 0;
}
// Borrowed handle to one query table of a resident key (valid until zk_pk_free; do not free it).
extern "C" const zk_bases* zk_pk_query_bases(const zk_pk* pk, int which) {
    if (!pk || which < 0 || which > 5) return nullptr;
    const zk_bases* all[6] = {pk->a, pk->b_g1, pk->b_g2, pk->h, pk->l, pk->gamma_abc};
    return all[which];
}
extern "C" int zk_pk_download_g1(zk_ctx* ctx, const zk_pk* pk, int which, size_t off, size_t n, zk_g1_affine* out) {
    ZK_API_BEGIN(ctx)
    if (!pk || which == 2 || which < 0 || which > 5) return ZK_ERR_ARG;
    const zk_bases* all[6] = {pk->a, pk->b_g1, pk->b_g2, pk->h, pk->l, pk->gamma_abc};
    return zk_bases_download_g1(ctx, all[which], off, n, out);
    ZK_API_END
}
extern "C" int zk_pk_download_g2(zk_ctx* ctx, const zk_pk* pk, int which, size_t off, size_t n, zk_g2_affine* out) {
    ZK_API_BEGIN(ctx)
    if (!pk || which != 2) return ZK_ERR_ARG;
    return zk_bases_download_g2(ctx, pk->b_g2, off, n, out);
    ZK_API_END
}
extern "C" int zk_pk_vk_g1(const zk_pk* pk, int which, zk_g1_affine* out) {
    ZK_API_BEGIN_NOCTX
    if (!pk || !out || which < 0 || which > 2) return ZK_ERR_ARG;
    const Affine<G1Field>* v[3] = {&pk->alpha_g1, &pk->beta_g1, &pk->delta_g1};
    host_aff_to_abi<G1Field>((uint64_t*)out, *v[which]);
    return ZK_OK;
    ZK_API_END
}
extern "C" int zk_pk_vk_g2(const zk_pk* pk, int which, zk_g2_affine* out) {
    ZK_API_BEGIN_NOCTX
    if (!pk || !out || which < 0 || which > 2) return ZK_ERR_ARG;
    const Affine<G2Field>* v[3] = {&pk->beta_g2, &pk->delta_g2, &pk->gamma_g2};
    host_aff_to_abi<G2Field>((uint64_t*)out, *v[which]);
    return ZK_OK;
    ZK_API_END
}

// generate_parameters with explicit toxic waste (generator.rs:44-231)
extern "C" int zk_groth16_setup(zk_ctx* ctx, const zk_r1cs* r, const zk_fr* alpha_, const zk_fr* beta_, const zk_fr* gamma_,
                                const zk_fr* delta_, const zk_fr* tau_, const zk_fr* g1_k, const zk_fr* g2_k, zk_pk** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !r || !alpha_ || !beta_ || !gamma_ || !delta_ || !tau_ || !g1_k || !g2_k || !out) return ZK_ERR_ARG;
    const HF alpha = HF::from_abi(*alpha_), beta = HF::from_abi(*beta_), gamma = HF::from_abi(*gamma_), delta = HF::from_abi(*delta_), t = HF::from_abi(*tau_);
    const HF one = HF::one();
    const size_t D = (size_t)1 << r->log_d, nc = r->nc, ni = r->ni;
    const size_t nvars = (ni - 1) + r->nw;
    if (gamma.is_zero() || delta.is_zero()) ZK_FAIL(ctx, ZK_ERR_ARG, "setup: gamma/delta must be non-zero");

    // domain constants
    const HF w = HF::domain_root(r->log_d), size_inv = HF::from_u64(D).inv();
    const HF zt = t.pow(D) - one;  // evaluate_vanishing_polynomial(t)
    if (zt.is_zero()) ZK_FAIL(ctx, ZK_ERR_ARG, "setup: tau lies in the evaluation domain");

    // evaluate_all_lagrange_coefficients(t): u_i = (zt/D) w^i / (t - w^i)   (radix2/mod.rs:116-165)
    std::vector<HF> u(D), den(D);
    {
        HF l = zt * size_inv, rr = one;
        for (size_t i = 0; i < D; i++) {
            den[i] = t - rr;
            u[i] = l;
            l = l * w;
            rr = rr * w;
        }
        HF::batch_inverse(den.data(), D);
        for (size_t i = 0; i < D; i++) u[i] = u[i] * den[i];
        den.clear(); den.shrink_to_fit();
    }
    // instance_map_with_evaluation (r1cs_to_qap.rs:47-92)
    std::vector<HF> a(nvars + 1, HF::zero()), b(nvars + 1, HF::zero()), c(nvars + 1, HF::zero());
    for (size_t i = 0; i < ni; i++) a[i] = u[nc + i];
    std::vector<HF>* abc[3] = {&a, &b, &c};
    for (int k = 0; k < 3; k++) {
        const auto& m = r->m[k];
        auto& dst = *abc[k];
        for (size_t i = 0; i < nc; i++)
            for (uint32_t e = m.h_row_ptr[i]; e < m.h_row_ptr[i + 1]; e++)
                dst[m.h_col[e]] = dst[m.h_col[e]] + (m.all_one ? u[i] : u[i] * HF{m.h_coeff[e]});
    }
    const HF gamma_inv = gamma.inv(), delta_inv = delta.inv();
    std::vector<HF> gamma_abc(ni), l(nvars + 1 - ni);
    for (size_t i = 0; i <= nvars; i++) {
        const HF s = beta * a[i] + alpha * b[i] + c[i];
        if (i < ni) gamma_abc[i] = s * gamma_inv;
        else l[i - ni] = s * delta_inv;
    }
    c.clear(); c.shrink_to_fit();
    std::vector<HF> hq(D - 1);
    {
        HF p = zt * delta_inv;
        for (size_t i = 0; i + 1 < D; i++) { hq[i] = p; p = p * t; }
    }
    // H over coset values (zk_pk::h_eval).  With H_i = t^i zt / delta for i <= D-2 and zinv = 1 / Z(g):
    //   h_eval[j]     = zinv sum_i M_ij H_i,  M_ij = g^-i w^-ij / D: the ifft of (zinv zt / delta) (t/g)^i, i <= D-2, then 0
    //   V_r           = sum_i w^-ir / D H_i   = -(u_r / delta) (1 - t^(D-1) w^r)      (the geometric sum; u_r as above)
    //   l_eval_pad[k] = (k >= ni ? l[k - ni] : 0) - zinv sum_r C_rk V_r
    // The two tables are a gain of a few per cent per proof and never take the last memory: they are built where the key with them
    // (six G1 tables instead of four) leaves half of the free device memory free.
    bool eval_h = zk_g16_eval_h_enabled() && D >= 2;
    if (eval_h) {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 0; }
        eval_h = zk_key_tables_bytes(nvars + 1, zk_mul_levels_for_key(ctx, nvars + 1), 6) <= mem_free / 2;
    }
    std::vector<HF> he, le;
    if (eval_h) {
        HF zinv;
        ZK_TRY(zk_ntt_vanishing_inv(ctx, r->log_d, &zinv.v));
        const HF k = zinv * delta_inv, t_top = t.pow(D - 1);
        std::vector<HF> nv(nc);                                       // -zinv V_r for the rows of C
        HF rr = one;
        for (size_t i = 0; i < nc; i++) {
            nv[i] = u[i] * k * (one - t_top * rr);
            rr = rr * w;
        }
        le.assign(nvars + 1, HF::zero());
        for (size_t i = ni; i <= nvars; i++) le[i] = l[i - ni];
        const auto& mc = r->m[2];
        for (size_t i = 0; i < nc; i++)
            for (uint32_t e = mc.h_row_ptr[i]; e < mc.h_row_ptr[i + 1]; e++)
                le[mc.h_col[e]] = le[mc.h_col[e]] + (mc.all_one ? nv[i] : nv[i] * HF{mc.h_coeff[e]});
        he.assign(D, HF::zero());
        const HF q = t * HF{fp_const<FrParams>(FrParams::GENERATOR_INV)};
        HF p = zinv * (zt * delta_inv);
        for (size_t i = 0; i + 1 < D; i++) { he[i] = p; p = p * q; }
    }
    u.clear(); u.shrink_to_fit();

    zk_pk* pk = new zk_pk();
    void* dev;
    int rc = upload_fr(ctx, a, "setup_scalars", &dev);
    if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, a.size(), &pk->a);
    if (rc == ZK_OK) rc = upload_fr(ctx, b, "setup_scalars", &dev);
    if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, b.size(), &pk->b_g1);
    if (rc == ZK_OK) rc = zk_fixed_base_g2_dev(ctx, g2_k, dev, b.size(), &pk->b_g2);
    if (rc == ZK_OK) rc = upload_fr(ctx, hq, "setup_scalars", &dev);
    if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, hq.size(), &pk->h);
    if (rc == ZK_OK) rc = upload_fr(ctx, l, "setup_scalars", &dev);
    if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, l.size(), &pk->l);
    if (rc == ZK_OK) rc = upload_fr(ctx, gamma_abc, "setup_scalars", &dev);
    if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, gamma_abc.size(), &pk->gamma_abc);
    if (eval_h) {
        if (rc == ZK_OK) rc = upload_fr(ctx, he, "setup_scalars", &dev);
        if (rc == ZK_OK) rc = zk_ntt_launch(ctx, dev, r->log_d, 1, 0);
        if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, D, &pk->h_eval);
        if (rc == ZK_OK) rc = upload_fr(ctx, le, "setup_scalars", &dev);
        if (rc == ZK_OK) rc = zk_fixed_base_g1_dev(ctx, g1_k, dev, le.size(), &pk->l_eval_pad);
        if (rc == ZK_OK) rc = first_point<G1Field>(ctx, pk->l_eval_pad, &pk->l_eval_0);
    }
    if (rc == ZK_OK) rc = zk_pk_precompute(ctx, pk);
    if (rc != ZK_OK) { zk_pk_free(ctx, pk); return rc; }
    pk->points_in_subgroup = true;            // every point of this key is a scalar multiple of a generator

    const Affine<G1Field> g1 = host_gen_mul<G1Field>(g1_gen(), HF::from_abi(*g1_k));
    const Affine<G2Field> g2 = host_gen_mul<G2Field>(g2_gen(), HF::from_abi(*g2_k));
    pk->alpha_g1 = host_gen_mul<G1Field>(g1, alpha);
    pk->beta_g1 = host_gen_mul<G1Field>(g1, beta);
    pk->delta_g1 = host_gen_mul<G1Field>(g1, delta);
    pk->beta_g2 = host_gen_mul<G2Field>(g2, beta);
    pk->delta_g2 = host_gen_mul<G2Field>(g2, delta);
    pk->gamma_g2 = host_gen_mul<G2Field>(g2, gamma);
    rc = first_point<G1Field>(ctx, pk->a, &pk->a0);
    if (rc == ZK_OK) rc = first_point<G1Field>(ctx, pk->b_g1, &pk->b0_g1);
    if (rc == ZK_OK) rc = first_point<G2Field>(ctx, pk->b_g2, &pk->b0_g2);
    if (rc != ZK_OK) { zk_pk_free(ctx, pk); return rc; }
    *out = pk;
    return ZK_OK;
    ZK_API_END
}

// ---- H over coset values for a key that was LOADED: the two tables from the key's own points -----------------------------------

namespace {

struct DevBuf {                                                        // device memory of one call (the scratch slots are never given back)
    void* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(zk_ctx* ctx, size_t bytes) {
        if (hipMalloc(&p, bytes ? bytes : 16) != hipSuccess) { p = nullptr; (void)hipGetLastError(); ZK_FAIL(ctx, ZK_ERR_NOMEM, "zk_pk_derive_eval_h: hipMalloc failed"); }
        return ZK_OK;
    }
    uint32_t* w() const { return (uint32_t*)p; }
};
int upload_words(zk_ctx* ctx, DevBuf* d, const std::vector<uint32_t>& v) {
    ZK_TRY(d->alloc(ctx, v.size() * 4));
    ZK_HIP(ctx, hipMemcpyAsync(d->p, v.data(), v.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    return ZK_OK;
}

// K_k = sum_r C_rk W_r for every column k < m of C (W: D affine points, table form): one segment of zk_g1_lincomb_launch per chunk of
// at most 64 terms of a column, then launches that add the partial sums of a column (scalar 1) until every column is one point.
// K: m affine points.
int transposed_c_product(zk_ctx* ctx, const zk_r1cs* r, const uint32_t* W, size_t D, DevBuf* K) {
    const auto& mc = r->m[2];
    const size_t m = r->ni + r->nw, nnz = mc.h_col.size();
    std::vector<uint32_t> start(m + 1, 0), rows(nnz), scal(nnz * 8, 0);
    for (size_t e = 0; e < nnz; e++) start[mc.h_col[e] + 1]++;
    for (size_t k = 0; k < m; k++) start[k + 1] += start[k];
    {
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (size_t i = 0; i < r->nc; i++)
            for (uint32_t e = mc.h_row_ptr[i]; e < mc.h_row_ptr[i + 1]; e++) {
                const uint32_t at = fill[mc.h_col[e]]++;
                rows[at] = (uint32_t)i;
                if (mc.all_one) scal[8 * (size_t)at] = 1;
                else fp_pack<FrParams>(&scal[8 * (size_t)at], fp_int_to_canon<FrParams>(mc.h_coeff[e]));
            }
    }
    std::vector<uint32_t> len(m);                                      // terms of column k at this level
    for (size_t k = 0; k < m; k++) len[k] = start[k + 1] - start[k];
    DevBuf pts_prev;                                                   // the level before's partial sums
    const uint32_t* pts = W;
    size_t n_pts = D;
    for (bool first = true;; first = false) {
        ZkLincombPack pack;
        std::vector<uint32_t> idx, ones;
        size_t at = 0, most = 0;
        for (size_t k = 0; k < m; k++) {
            for (size_t lo = 0; lo < len[k] || lo == 0; lo += LINCOMB_MAX_TERMS) {
                const size_t n = std::min<size_t>(LINCOMB_MAX_TERMS, len[k] - lo);
                bool ok;
                if (first) ok = pack.add(rows.data() + at + lo, scal.data() + 8 * (at + lo), n);
                else {
                    idx.resize(n); ones.assign(8 * n, 0);
                    for (size_t t = 0; t < n; t++) { idx[t] = (uint32_t)(at + lo + t); ones[8 * t] = 1; }
                    ok = pack.add(idx.data(), ones.data(), n);
                }
                if (!ok) ZK_FAIL(ctx, ZK_ERR_STATE, "zk_pk_derive_eval_h: a segment of more than 64 terms");
            }
            at += len[k];
            len[k] = len[k] ? (uint32_t)((len[k] + LINCOMB_MAX_TERMS - 1) / LINCOMB_MAX_TERMS) : 1u;
            most = std::max<size_t>(most, len[k]);
        }
        pack.finish();
        const size_t n_seg = pack.seg_off.size() - 1;
        DevBuf d_idx, d_k, d_off, d_inf, out;
        ZK_TRY(upload_words(ctx, &d_idx, pack.point_index));
        ZK_TRY(upload_words(ctx, &d_k, pack.scalars));
        ZK_TRY(upload_words(ctx, &d_off, pack.seg_off));
        ZK_TRY(d_inf.alloc(ctx, n_seg * 4));
        ZK_TRY(out.alloc(ctx, n_seg * 96));
        ZK_TRY(zk_g1_lincomb_launch(ctx, pts, n_pts, d_idx.w(), d_k.w(), d_off.w(), n_seg, pack.lanes(), out.w(), d_inf.w()));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));                // (the pack is a local)
        std::swap(pts_prev.p, out.p);                                  // (out now frees the level before's)
        pts = pts_prev.w();
        n_pts = n_seg;
        if (most == 1) break;
    }
    std::swap(K->p, pts_prev.p);
    return n_pts == m ? ZK_OK : ZK_ERR_STATE;
}

}  // namespace

// The tables of "H over coset values" (zk_pk::h_eval, l_eval_pad, l_eval_0) for a key that came in through zk_pk_upload or
// zk_pk_deserialize, from the key's own points -- nobody holds the trapdoor of such a key.  With H_i = h_query[i] (H_(D-1) = O),
// zinv = 1 / Z(g), w the domain generator, g the coset generator:
//   h_eval[j]     = sum_i w^(-ij) (zinv g^(-i) / D) H_i        a size-D transform over POINTS with root 1/w (g1_ntt.hip)
//   W_r           = sum_i w^(-ir) (zinv / D) H_i               the same transform of the second vector of that batch
//   l_eval_pad[k] = l_pad[k] - sum_r C_rk W_r                  the transposed sparse product, one short linear combination per column
// -- the group elements zk_groth16_setup makes from the trapdoor, hence the same canonical words and the same proof bytes.  Before the
// tables are published the call proves the identity on an assignment of its own (z_0 = 1, the rest random: the identity is linear,
// the assignment need not satisfy anything): h_query x h + l_pad x z against h_eval x e + l_eval_pad x z + l_eval_0.  A key whose
// h_query / l_query are not what a setup produces -- a point with a component outside the prime-order subgroup breaks the transform's
// algebra -- fails it: the tables are dropped, the key stays exactly as it was, ZK_ERR_ARG.
// ZK_OK and nothing done: the key has the tables already, or ZK_G16_EVAL_H=0.  ZK_ERR_ARG: a null pointer, a system of another size
// (ni + nw != a_query's length, h_query not D - 1 points, l_query not nw points, D < 2), a key without l_pad.  ZK_ERR_NOMEM: the key
// with six G1 tables at its mul_levels would not fit in half of the device memory that is free when the key's present tables are
// counted as free (zk_groth16_setup's rule); the key is unchanged.  A pending presort / front is dropped.  With zk_set_profiling
// the phases' wall times are left in the context's timers ("derive.transforms", ".product", ".tables", ".check").
extern "C" int zk_pk_derive_eval_h(zk_ctx* ctx, zk_pk* pk, const zk_r1cs* r) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r) return ZK_ERR_ARG;
    const size_t D = (size_t)1 << r->log_d, m = r->ni + r->nw;
    if (!pk->a || !pk->h || !pk->l || m != pk->a->n || r->log_d < 1 || pk->h->n != D - 1 || pk->l->n != r->nw)
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_pk_derive_eval_h: the key does not belong to this constraint system");
    if (pk->h_eval && pk->l_eval_pad) return ZK_OK;
    if (!zk_g16_eval_h_enabled()) return ZK_OK;
    if (!pk->l_pad || pk->l_pad->n != m) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_pk_derive_eval_h: the key has no padded l_query");
    {
        size_t mem_free = 0, mem_total = 0;
        if (hipMemGetInfo(&mem_free, &mem_total) != hipSuccess) { (void)hipGetLastError(); mem_free = 0; }
        if (zk_key_tables_bytes(m, pk->mul_levels, 6) > (mem_free + zk_key_tables_bytes(m, pk->mul_levels, 4)) / 2)
            ZK_FAIL(ctx, ZK_ERR_NOMEM, "zk_pk_derive_eval_h: the key with the two tables would take more than half of the device memory");
    }
    zk_presort_free(ctx);
    using Clock = std::chrono::steady_clock;
    auto t0 = Clock::now();
    auto lap = [&](const char* name) {
        if (!ctx->profiling) return;
        auto& t = ctx->timers[name];
        const auto now = Clock::now();
        t.ms += std::chrono::duration<float, std::milli>(now - t0).count();
        t.count += 1;
        t0 = now;
    };
    struct Tables {                                                    // the two tables until they are published
        zk_ctx* ctx;
        zk_bases *he = nullptr, *le = nullptr;
        ~Tables() { zk_bases_free(ctx, he); zk_bases_free(ctx, le); }
    } tb{ctx};

    // the pre-scales zinv g^(-i) / D (i < D) and zinv / D as raw scalars
    HF c;
    ZK_TRY(zk_ntt_vanishing_inv(ctx, r->log_d, &c.v));
    c = c * HF::from_u64(D).inv();
    {
        std::vector<uint32_t> sc((D + 1) * 8);
        const HF ginv{fp_const<FrParams>(FrParams::GENERATOR_INV)};
        HF p = c;
        for (size_t i = 0; i < D; i++) { p.canon_words(&sc[8 * i]); p = p * ginv; }
        c.canon_words(&sc[8 * D]);
        DevBuf d_sc, work, scr, W, K;
        const uint32_t* tw;
        ZK_TRY(upload_words(ctx, &d_sc, sc));
        ZK_TRY(zk_g1_ntt_twiddles(ctx, r->log_d, 1, &tw));           // (waits: sc has been read)
        ZK_TRY(work.alloc(ctx, std::max(2 * D, m) * 192));
        ZK_TRY(scr.alloc(ctx, std::max(D, m) * 48));
        ZK_TRY(W.alloc(ctx, D * 96));
        ZK_TRY(zk_bases_alloc_dev(ctx, 1, D, &tb.he));
        const ZkG1NttScale scale{d_sc.w(), {0u, (uint32_t)D}, {1u, 0u}};
        ZK_TRY(zk_g1_ntt_launch(ctx, pk->h->dev, D - 1, 0, &scale, r->log_d, 2, tw, work.w()));
        ZK_TRY(zk_g1_batch_affine_launch(ctx, work.w(), tb.he->dev, scr.w(), D));
        ZK_TRY(zk_g1_batch_affine_launch(ctx, work.w() + D * 48, W.w(), scr.w(), D));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        lap("derive.transforms");
        ZK_TRY(transposed_c_product(ctx, r, W.w(), D, &K));
        ZK_TRY(zk_bases_alloc_dev(ctx, 1, m, &tb.le));
        ZK_TRY(zk_g1_sub_launch(ctx, pk->l_pad->dev, K.w(), work.w(), m));
        ZK_TRY(zk_g1_batch_affine_launch(ctx, work.w(), tb.le->dev, scr.w(), m));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        lap("derive.product");
    }
    ZK_TRY(zk_bases_precompute_levels(ctx, tb.he, pk->mul_levels));
    ZK_TRY(zk_bases_precompute_levels(ctx, tb.le, pk->mul_levels));
    Affine<G1Field> le0;
    ZK_TRY(first_point<G1Field>(ctx, tb.le, &le0));
    lap("derive.tables");

    // the identity on an assignment of the call's own, over the key's tables and over the new ones
    {
        DevBuf z, h;
        ZK_TRY(z.alloc(ctx, m * 32));
        ZK_TRY(h.alloc(ctx, D * 32));
        ZK_TRY(zk_fr_random_dev(ctx, nullptr, 0, z.p, m));
        uint32_t one[8];
        fp_pack<FrParams>(one, fp_int_to_ext<FrParams>(fp_one<FrParams>()));
        ZK_HIP(ctx, hipMemcpyAsync(z.p, one, 32, hipMemcpyHostToDevice, ctx->stream));
        ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        zk_g1_projective s_h, s_l, s_he, s_le;
        ZK_TRY(zk_groth16_witness_map_dev(ctx, r, z.p, h.p));
        ZK_TRY(zk_msm_run(ctx, pk->h, 0, h.p, D - 1, &s_h));
        ZK_TRY(zk_msm_run(ctx, pk->l_pad, 1, (const char*)z.p + 32, m - 1, &s_l));
        ZK_TRY(zk_groth16_witness_map_eval_dev(ctx, r, z.p, h.p));
        ZK_TRY(zk_msm_run(ctx, tb.he, 0, h.p, D, &s_he));
        ZK_TRY(zk_msm_run(ctx, tb.le, 1, (const char*)z.p + 32, m - 1, &s_le));
        using H = Fq64Field;
        const Affine<H> lhs = xyzz_to_affine<H>(xyzz_add<H>(host64_proj_from_abi<H>((const uint64_t*)&s_h), host64_proj_from_abi<H>((const uint64_t*)&s_l)));
        const Affine<H> rhs = xyzz_to_affine<H>(xyzz_madd<H>(
            xyzz_add<H>(host64_proj_from_abi<H>((const uint64_t*)&s_he), host64_proj_from_abi<H>((const uint64_t*)&s_le)), aff_to_host64<G1Field>(le0)));
        lap("derive.check");
        if (!H::eq(lhs.x, rhs.x) || !H::eq(lhs.y, rhs.y))
            ZK_FAIL(ctx, ZK_ERR_ARG,
                    "zk_pk_derive_eval_h: the key's h_query / l_query do not satisfy the identity of H over coset values (points outside the "
                    "prime-order subgroup, or a key of another system); the key is unchanged");
    }
    zk_presort_free(ctx);
    pk->h_eval = tb.he;
    pk->l_eval_pad = tb.le;
    pk->l_eval_0 = le0;
    tb.he = tb.le = nullptr;
    if (!ZkG16Jobs(pk, r, nullptr, nullptr).eval_h) {                  // (a table that got fewer shifted copies than the key's: no memory for them)
        zk_bases_free(ctx, pk->h_eval); zk_bases_free(ctx, pk->l_eval_pad);
        pk->h_eval = pk->l_eval_pad = nullptr;
        ZK_FAIL(ctx, ZK_ERR_NOMEM, "zk_pk_derive_eval_h: no memory for the window multiples of the two tables; the key is unchanged");
    }
    return ZK_OK;
    ZK_API_END
}

// h_eval (which = 0: D points), l_eval_pad (1: ni + nw points) or l_eval_0 (2: one point) of a key that carries them
extern "C" int zk_pk_download_eval_g1(zk_ctx* ctx, const zk_pk* pk, int which, size_t off, size_t n, zk_g1_affine* out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !pk->h_eval || !pk->l_eval_pad || which < 0 || which > 2 || (n && !out)) return ZK_ERR_ARG;
    if (which == 2) {
        if (off + n > 1) return ZK_ERR_ARG;
        if (n) host_aff_to_abi<G1Field>((uint64_t*)out, pk->l_eval_0);
        return ZK_OK;
    }
    return zk_bases_download_g1(ctx, which == 0 ? pk->h_eval : pk->l_eval_pad, off, n, out);
    ZK_API_END
}
