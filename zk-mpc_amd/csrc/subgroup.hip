// subgroup.hip -- subgroup membership of whole point tables on the device, and the checked loaders built on it.
//
// Replaces (reference): the is_in_correct_subgroup_assuming_on_curve call inside GroupAffine::deserialize / deserialize_uncompressed
// (arkworks/algebra/ec/src/models/short_weierstrass_jacobian.rs:146-149, :888-940), which every ProvingKey, VerifyingKey, Proof and
// KZG10 UniversalParams the reference reads from bytes passes through.  The arithmetic is subgroup.cuh.
//
//   k_subgroup<F>   one point per lane over a table in the form zk_bases keeps (packed affine, internal Montgomery form): one flag
//                   word per point (1 = outside the subgroup) and "some point outside" ORed into one word
// No LDS, no runtime-indexed register arrays: the accumulator, the point and the formulas' temporaries are registers (DESIGN 5b''''
// has the figures from the compiler's metadata for both instantiations).
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "subgroup.cuh"
#include <string.h>

using namespace zk;

namespace {

// OR_EACH: the per-point word keeps what it holds and gains the flag (a caller that has flags of its own there: the verifier's
// off-curve flags); else it is written
template <class F, bool OR_EACH>
__global__ void __launch_bounds__(64) k_subgroup(const uint32_t* __restrict__ tab, size_t n, uint32_t* __restrict__ bad, uint32_t* bad_each) {
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    if (i >= n) return;
    const bool in = in_subgroup<F>(aff_load16<F>(tab, i));
    const uint32_t flag = in ? 0u : 1u;
    if (bad_each) bad_each[i] = OR_EACH ? (bad_each[i] | flag) : flag;
    if (flag && bad) atomicOr(bad, 1u);
}

constexpr size_t NONE = (size_t)-1;

// the flags of points [offset, offset + n) of a table: how many are outside, the first of them (relative to offset), each one's
// verdict (1 = inside) if the caller wants it.  One launch and one 4-byte copy when every point is inside; when some point is
// outside (the error path of the loaders) a second copy brings the n flag words back and the host counts them.
int table_check(zk_ctx* ctx, const zk_bases* b, size_t offset, size_t n, uint8_t* in_each, size_t* n_outside, size_t* first_outside) {
    *n_outside = 0;
    *first_outside = NONE;
    if (!n) return ZK_OK;
    uint32_t* flags;
    ZK_TRY(zk_scratch(ctx, "subgroup_flags", (n + 1) * 4, (void**)&flags));
    ZK_HIP(ctx, hipMemsetAsync(flags, 0, 4, ctx->stream));
    ZK_TRY(zk_subgroup_launch(ctx, b->group, b->dev + offset * (b->group == 2 ? 2 * G2Field::WORDS : 2 * G1Field::WORDS), n, flags, flags + 1));
    uint32_t any = 0;
    ZK_HIP(ctx, hipMemcpyAsync(&any, flags, 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!any && !in_each) return ZK_OK;
    if (!any) { memset(in_each, 1, n); return ZK_OK; }
    std::vector<uint32_t> h(n);
    ZK_HIP(ctx, hipMemcpyAsync(h.data(), flags + 1, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (size_t i = 0; i < n; i++) {
        if (h[i]) {
            if (*first_outside == NONE) *first_outside = i;
            ++*n_outside;
        }
        if (in_each) in_each[i] = h[i] ? 0 : 1;
    }
    return ZK_OK;
}

const char* const PK_PART_NAMES[ZK_PK_SUBGROUP_PARTS] = {"a_query", "b_g1_query", "b_g2_query", "h_query", "l_query", "gamma_abc_g1", "the single points"};

int pk_check(zk_ctx* ctx, const zk_pk* pk, zk_pk_subgroup_report* rep) {
    const zk_bases* tabs[6] = {pk->a, pk->b_g1, pk->b_g2, pk->h, pk->l, pk->gamma_abc};
    for (int k = 0; k < 6; k++) {
        rep->outside[k] = 0;
        rep->first[k] = NONE;
        if (tabs[k] && tabs[k]->n) ZK_TRY(table_check(ctx, tabs[k], 0, tabs[k]->n, nullptr, &rep->outside[k], &rep->first[k]));
    }
    // alpha_g1, beta_g1, delta_g1, beta_g2, gamma_g2, delta_g2 (in that order): a handful of points, on the host
    const bool single[6] = {in_subgroup<Fq64Field>(aff_to_host64<G1Field>(pk->alpha_g1)), in_subgroup<Fq64Field>(aff_to_host64<G1Field>(pk->beta_g1)),
                            in_subgroup<Fq64Field>(aff_to_host64<G1Field>(pk->delta_g1)), in_subgroup<Fq264Field>(aff_to_host64<G2Field>(pk->beta_g2)),
                            in_subgroup<Fq264Field>(aff_to_host64<G2Field>(pk->gamma_g2)), in_subgroup<Fq264Field>(aff_to_host64<G2Field>(pk->delta_g2))};
    rep->outside[6] = 0;
    rep->first[6] = NONE;
    for (size_t i = 0; i < 6; i++)
        if (!single[i]) {
            if (rep->first[6] == NONE) rep->first[6] = i;
            ++rep->outside[6];
        }
    return ZK_OK;
}
bool report_clean(const zk_pk_subgroup_report& rep, int* part) {
    for (int k = 0; k < ZK_PK_SUBGROUP_PARTS; k++)
        if (rep.outside[k]) { *part = k; return false; }
    return true;
}

}  // namespace

// the kernel for a caller that holds its points on the device already (pairing.hip): table form, n points; bad_dev: one word, ORed
// with 1 if a point is outside; bad_each_dev (or NULL): one word per point, written -- or, with or_each, ORed.  On ctx->stream, no wait.
int zk_subgroup_launch(zk_ctx* ctx, int group, const uint32_t* table_dev, size_t n, uint32_t* bad_dev, uint32_t* bad_each_dev, bool or_each) {
    if (!n) return ZK_OK;
    if (n > ((size_t)1 << 37)) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_subgroup_launch: too many points for one launch");
    const unsigned blocks = zk_blocks64(n);
    if (group == 2 && or_each) hipLaunchKernelGGL((k_subgroup<G2Field, true>), blocks, 64, 0, ctx->stream, table_dev, n, bad_dev, bad_each_dev);
    else if (group == 2) hipLaunchKernelGGL((k_subgroup<G2Field, false>), blocks, 64, 0, ctx->stream, table_dev, n, bad_dev, bad_each_dev);
    else if (or_each) hipLaunchKernelGGL((k_subgroup<G1Field, true>), blocks, 64, 0, ctx->stream, table_dev, n, bad_dev, bad_each_dev);
    else hipLaunchKernelGGL((k_subgroup<G1Field, false>), blocks, 64, 0, ctx->stream, table_dev, n, bad_dev, bad_each_dev);
    ZK_HIP(ctx, hipGetLastError());
    return ZK_OK;
}
bool zk_host_in_subgroup_g1(const Affine<G1Field>& p) { return in_subgroup<Fq64Field>(aff_to_host64<G1Field>(p)); }
bool zk_host_in_subgroup_g2(const Affine<G2Field>& p) { return in_subgroup<Fq264Field>(aff_to_host64<G2Field>(p)); }

extern "C" int zk_g1_in_subgroup_host(const zk_g1_affine* points, size_t n, uint8_t* flags) {
    ZK_API_BEGIN_NOCTX
    if ((n && !points) || (n && !flags)) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&points[i], 2)) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++) flags[i] = in_subgroup<Fq64Field>(zk_host_g1(&points[i])) ? 1 : 0;
    return ZK_OK;
    ZK_API_END
}
extern "C" int zk_g2_in_subgroup_host(const zk_g2_affine* points, size_t n, uint8_t* flags) {
    ZK_API_BEGIN_NOCTX
    if ((n && !points) || (n && !flags)) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++)
        if (!zk_words_below_q((const uint64_t*)&points[i], 4)) return ZK_ERR_ARG;
    for (size_t i = 0; i < n; i++) flags[i] = in_subgroup<Fq264Field>(zk_host_g2(&points[i])) ? 1 : 0;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_bases_subgroup_check(zk_ctx* ctx, const zk_bases* bases, size_t offset, size_t n, uint8_t* in_each_host, size_t* n_outside,
                                       size_t* first_outside) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !bases || !n_outside || !first_outside) return ZK_ERR_ARG;
    if (offset > bases->n || n > bases->n - offset) ZK_FAIL(ctx, ZK_ERR_ARG, "zk_bases_subgroup_check: range out of bounds");
    return table_check(ctx, bases, offset, n, in_each_host, n_outside, first_outside);
    ZK_API_END
}

extern "C" int zk_bases_deserialize_checked(zk_ctx* ctx, int group, const uint8_t* bytes_host, size_t n, int compressed, zk_bases** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !out || (n && !bytes_host) || (group != 1 && group != 2)) return ZK_ERR_ARG;
    zk_bases* b = nullptr;
    ZK_TRY(compressed ? zk_bases_deserialize_compressed(ctx, group, bytes_host, n, &b) : zk_bases_deserialize_uncompressed(ctx, group, bytes_host, n, &b));
    size_t outside = 0, first = NONE;
    const int rc = table_check(ctx, b, 0, n, nullptr, &outside, &first);
    if (rc != ZK_OK || outside) {
        zk_bases_free(ctx, b);
        if (rc != ZK_OK) return rc;
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_bases_deserialize_checked: point " + std::to_string(first) + " is not in the prime-order subgroup (" +
                                     std::to_string(outside) + " of " + std::to_string(n) + " are not; SerializationError::InvalidData)");
    }
    *out = b;
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_kzg_srs_deserialize_checked(zk_ctx* ctx, const uint8_t* bytes_host, size_t len, int compressed, zk_bases** powers_g,
                                              zk_bases** powers_gamma_g, zk_g2_affine* h, zk_g2_affine* beta_h) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !bytes_host || !powers_g || !powers_gamma_g || !h || !beta_h) return ZK_ERR_ARG;
    zk_bases *pg = nullptr, *pgg = nullptr;
    zk_g2_affine hs[2];
    ZK_TRY(zk_kzg_srs_deserialize(ctx, bytes_host, len, compressed, &pg, &pgg, &hs[0], &hs[1]));
    std::string what;
    size_t outside = 0, first = NONE;
    int rc = table_check(ctx, pg, 0, pg->n, nullptr, &outside, &first);
    if (rc == ZK_OK && outside) what = "powers_of_g[" + std::to_string(first) + "]";
    if (rc == ZK_OK && what.empty()) {
        rc = table_check(ctx, pgg, 0, pgg->n, nullptr, &outside, &first);
        if (rc == ZK_OK && outside) what = "powers_of_gamma_g[" + std::to_string(first) + "]";
    }
    if (rc == ZK_OK && what.empty()) {
        if (!in_subgroup<Fq264Field>(zk_host_g2(&hs[0]))) what = "h";
        else if (!in_subgroup<Fq264Field>(zk_host_g2(&hs[1]))) what = "beta_h";
    }
    if (rc != ZK_OK || !what.empty()) {
        zk_bases_free(ctx, pg);
        zk_bases_free(ctx, pgg);
        if (rc != ZK_OK) return rc;
        ZK_FAIL(ctx, ZK_ERR_ARG, "zk_kzg_srs_deserialize_checked: " + what + " is not in the prime-order subgroup (SerializationError::InvalidData)");
    }
    *powers_g = pg;
    *powers_gamma_g = pgg;
    *h = hs[0];
    *beta_h = hs[1];
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_pk_check_subgroups(zk_ctx* ctx, const zk_pk* pk, zk_pk_subgroup_report* report) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !report) return ZK_ERR_ARG;
    ZK_TRY(pk_check(ctx, pk, report));
    return ZK_OK;
    ZK_API_END
}

extern "C" int zk_pk_points_in_subgroup(const zk_pk* pk) {
    ZK_API_BEGIN_NOCTX
    return (pk && pk->points_in_subgroup) ? 1 : 0;
    ZK_API_END
}

extern "C" int zk_pk_deserialize_checked(zk_ctx* ctx, const uint8_t* bytes_host, size_t len, int compressed, zk_pk** out) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !bytes_host || !out) return ZK_ERR_ARG;
    zk_pk* pk = nullptr;
    ZK_TRY(zk_pk_deserialize(ctx, bytes_host, len, compressed, &pk));
    zk_pk_subgroup_report rep;
    const int rc = pk_check(ctx, pk, &rep);
    int part = 0;
    if (rc != ZK_OK || !report_clean(rep, &part)) {
        zk_pk_free(ctx, pk);
        if (rc != ZK_OK) return rc;
        ZK_FAIL(ctx, ZK_ERR_ARG, std::string("zk_pk_deserialize_checked: ") + PK_PART_NAMES[part] + ": point " + std::to_string(rep.first[part]) +
                                     " is not in the prime-order subgroup (" + std::to_string(rep.outside[part]) + " of that part are not; SerializationError::InvalidData)");
    }
    *out = pk;
    return ZK_OK;
    ZK_API_END
}
