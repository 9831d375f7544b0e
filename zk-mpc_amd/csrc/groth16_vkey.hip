// groth16_vkey.hip -- the verifier's own key on the device: arkworks' PreparedVerifyingKey with the window multiples prepare_inputs
// reads (g1_prepare_inputs.hip).
//
// Replaces (reference):
//   prepare_verifying_key, PreparedVerifyingKey     arkworks/groth16/src/verifier.rs:9-16, data_structures.rs:60-75
// Every way a zk_vkey comes to be -- a host view, its bytes (key_io.hip), a resident proving key, the vkey a zk_pk owns for its own
// verifier entry points -- ends in zk_vkey_make.
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "pairing.cuh"

using namespace zk;

namespace {

constexpr size_t PREP_TABLE_LIMIT_DEFAULT = (size_t)256 << 20;

int vkey_fill(zk_ctx* ctx, zk_vkey* v, const Affine<G1Field>& alpha, const Affine<G2Field> g2s[3], bool in_subgroup) {
    if (!v->gamma_abc || v->gamma_abc->group != 1 || v->gamma_abc->n == 0) ZK_FAIL(ctx, ZK_ERR_ARG, "verifying key: gamma_abc_g1 is empty");
    if (aff_is_inf<G2Field>(g2s[1])) ZK_FAIL(ctx, ZK_ERR_ARG, "verifying key: gamma_g2 is the point at infinity");
    v->alpha_g1 = alpha;
    v->beta_g2 = g2s[0];
    v->gamma_g2 = g2s[1];
    v->delta_g2 = g2s[2];
    v->neg_gamma_g2 = aff_neg<G2Field>(g2s[1]);
    v->neg_delta_g2 = aff_neg<G2Field>(g2s[2]);
    v->points_in_subgroup = in_subgroup;
    const Affine<Fq64Field> a = aff_to_host64<G1Field>(alpha);
    const Affine<Fq264Field> b = aff_to_host64<G2Field>(g2s[0]);
    Fq12<Fq264Field> e;
    pairing_product<Fq264Field>(e, &a, &b, 1);
    fq12_host_to_packed(v->e_alpha_beta, e);
    const size_t n = v->gamma_abc->n, ninp = n - 1, bytes = ninp * ZK_PREP_ENTRIES * 96;
    v->abc_host.resize(n * 24);
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ZK_HIP(ctx, hipMemcpy(v->abc_host.data(), v->gamma_abc->dev, n * 96, hipMemcpyDeviceToHost));
    if (!ninp || bytes > ctx->prepare_table_limit) return ZK_OK;
    if (hipMalloc((void**)&v->win, bytes) != hipSuccess) {      // no memory for the table: the key works without (the MSM path)
        (void)hipGetLastError();
        v->win = nullptr;
        return ZK_OK;
    }
    ZK_TRY(zk_g1_window_table_launch(ctx, v->gamma_abc->dev, ninp, v->win));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return ZK_OK;
}

bool pk_has_vk_parts(const zk_pk* pk) { return pk->gamma_abc && pk->gamma_abc->n != 0 && !aff_is_inf<G2Field>(pk->gamma_g2); }

int vkey_of_pk(zk_ctx* ctx, const zk_pk* pk, zk_vkey** out) {
    const size_t n = pk->gamma_abc->n;
    zk_bases* b = nullptr;
    ZK_TRY(zk_bases_alloc_dev(ctx, 1, n, &b));
    if (hipMemcpy(b->dev, pk->gamma_abc->dev, n * 96, hipMemcpyDeviceToDevice) != hipSuccess) {
        zk_bases_free(ctx, b);
        ZK_FAIL(ctx, ZK_ERR_HIP, "verifying key: the copy of gamma_abc_g1 failed");
    }
    const Affine<G2Field> g2s[3] = {pk->beta_g2, pk->gamma_g2, pk->delta_g2};
    return zk_vkey_make(ctx, pk->alpha_g1, g2s, b, pk->points_in_subgroup, out);
}

}  // namespace

int zk_vkey_make(zk_ctx* ctx, const Affine<G1Field>& alpha, const Affine<G2Field> g2s[3], zk_bases* abc, bool in_subgroup, zk_vkey** out) {
    zk_vkey* v = new zk_vkey();
    v->gamma_abc = abc;
    const int rc = vkey_fill(ctx, v, alpha, g2s, in_subgroup);
    if (rc != ZK_OK) {
        const std::string why = ctx->last_error;
        zk_vkey_free(ctx, v);
        ctx->last_error = why;
        return rc;
    }
    *out = v;
    return ZK_OK;
}

int zk_pk_vkey(zk_ctx* ctx, const zk_pk* pk, const char* entry, const zk_vkey** out) {
    if (!pk_has_vk_parts(pk)) ZK_FAIL(ctx, ZK_ERR_ARG, std::string(entry) + ": the key has no verifying-key parts (gamma_g2, gamma_abc_g1)");
    std::lock_guard<std::mutex> g(pk->vkey_mu);
    if (!pk->vkey) ZK_TRY(vkey_of_pk(ctx, pk, &pk->vkey));
    *out = pk->vkey;
    return ZK_OK;
}

extern "C" int zk_vkey_from_pk(zk_ctx* ctx, const zk_pk* pk, zk_vkey** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !out) return ZK_ERR_ARG;
    if (!pk_has_vk_parts(pk)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_vkey_from_pk: the key has no verifying-key parts (gamma_g2, gamma_abc_g1)");
    return vkey_of_pk(ctx, pk, out);
    ZK_API_END
}

extern "C" int zk_vkey_upload(zk_ctx* ctx, const zk_vk_host* vk, int check_subgroup, zk_vkey** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !vk || !out) return ZK_ERR_ARG;
    if (!vk->gamma_abc_len || !zk_vk_host_ok(vk, vk->gamma_abc_len - 1))
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_vkey_upload: not a verifying key (no gamma_abc_g1, or a coordinate word that is not below q)");
    const Affine<G1Field> alpha = host_aff_from_abi<G1Field>((const uint64_t*)&vk->alpha_g1);
    const Affine<G2Field> g2s[3] = {host_aff_from_abi<G2Field>((const uint64_t*)&vk->beta_g2), host_aff_from_abi<G2Field>((const uint64_t*)&vk->gamma_g2),
                                    host_aff_from_abi<G2Field>((const uint64_t*)&vk->delta_g2)};
    if (check_subgroup) {
        static const char* const names[3] = {"beta_g2", "gamma_g2", "delta_g2"};
        if (!zk_host_in_subgroup_g1(alpha)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_vkey_upload: alpha_g1 is outside the subgroup");
        for (int i = 0; i < 3; i++)
            if (!zk_host_in_subgroup_g2(g2s[i])) ZK_FAIL(ctx, ZK_ERR_ARG, std::string("zk_vkey_upload: ") + names[i] + " is outside the subgroup");
    }
    zk_bases* b = nullptr;
    ZK_TRY(zk_bases_upload_g1(ctx, vk->gamma_abc_g1, vk->gamma_abc_len, &b));
    if (check_subgroup) {
        size_t n_outside = 0, first = 0;
        const int rc = zk_bases_subgroup_check(ctx, b, 0, b->n, nullptr, &n_outside, &first);
        if (rc != ZK_OK || n_outside) {
            zk_bases_free(ctx, b);
            if (rc != ZK_OK) return rc;
            ZK_FAIL(ctx, ZK_ERR_ARG, "zk_vkey_upload: gamma_abc_g1[" + std::to_string(first) + "] is outside the subgroup");
        }
    }
    return zk_vkey_make(ctx, alpha, g2s, b, false, out);      // (a host view is not held to the curve equation: no endomorphism on its points)
    ZK_API_END
}

extern "C" size_t zk_vkey_num_inputs(const zk_vkey* vkey) { return vkey ? vkey->ninp() : 0; }

extern "C" int zk_vkey_free(zk_ctx* ctx, zk_vkey* vkey) {
    ZK_API_BEGIN(ctx)
    if (!vkey) return ZK_OK;
    if (vkey->win) {
        if (ctx) (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(vkey->win);
    }
    zk_bases_free(ctx, vkey->gamma_abc);
    delete vkey;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_groth16_prepare_table_limit(zk_ctx* ctx, size_t bytes) {
    ZK_API_BEGIN(ctx)
    if (!ctx) return ZK_ERR_ARG;
    ctx->prepare_table_limit = bytes == (size_t)-1 ? PREP_TABLE_LIMIT_DEFAULT : bytes;
    return ZK_OK;
    ZK_API_END
}
