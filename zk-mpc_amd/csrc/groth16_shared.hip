// groth16_shared.hip -- create_proof over additive / SPDZ shares as one C-ABI call.
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "groth16_shared_int.hpp"
#include "sharednet.hpp"

using namespace zk;

// ---- the collaborative prover as ONE entry point ---------------------------------------------------------------------------------
// create_proof::<MpcPairingEngine, C> over additive shares (src/groth16.rs:68-183): what mpc.py::Party.create_proof_shared
// sequences from ~40 calls, for a host that cannot call Python.  This file is the protocol; the transport, the Beaver product
// with its vector opens and the small open (wire layout, validation of peers' payloads, MAC check) are sharednet.hpp's, the host
// algebra of a proof is groth16_shared_int.hpp's (the batch prover, groth16_shared_batch.hip, runs the same).  Opens
// happen in the fused order of create_proof_shared: the nine small opens of the three GroupShare::scale calls
// (share/group.rs:72-111, DummyGroupTripleSource) and of Proof::reveal travel in two small opens; every opened value is the
// reference's, and so are the 192 bytes.
namespace {

namespace sh = zk_shared;
using sh::SX1;

// LANES = 1: additive shares (AdditiveFieldShare / AdditiveGroupShare); LANES = 2: SPDZ (share lane, MAC lane), every open
// MAC-checked.  z / rs / ss / tx..tz are indexed by lane.
template <int LANES>
int prove_shared_impl(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* const z[2], const zk_fr* const rs[2],
                      const zk_fr* const ss[2], const void* const tx[2], const void* const ty[2], const void* const tz[2],
                      const zk_net_vtable* net, uint8_t proof[192], uint64_t* bytes_sent) {
    if (zk_shared_triple_given(LANES, tx, ty, tz) < 0) ZK_FAIL(ctx, ZK_ERR_ARG, "prove_shared: give a whole Beaver triple (every lane) or none");
    const bool leader = ctx->party_id == 0;
    const size_t D = (size_t)1 << r->log_d;
    ZkSharedNet nt{ctx, net};
    const sh::Key K(pk, leader);
    sh::Proof P;
    sh::begin(LANES, rs, ss, &P);
    // public point x shared scalar, under the device work
    ZkTask<void> f_r_g1[2], f_s_g1[2], f_s_g2[2];      // (joining handles: the tasks reference this frame and are waited for when it is left)
    for (int l = 0; l < LANES; l++) {
        f_r_g1[l] = zk_async(ctx, [&, l] { sh::pre_r_g1(K, &P, l); });
        f_s_g1[l] = zk_async(ctx, [&, l] { sh::pre_s_g1(K, &P, l); });
        f_s_g2[l] = zk_async(ctx, [&, l] { sh::pre_s_g2(K, &P, l); });
    }
    void *a[2], *b[2], *c[2];
    char nm[32];
    for (int l = 0; l < LANES; l++) {
        const char* names[3] = {"shared_a%d", "shared_b%d", "shared_c%d"};
        void** dst[3] = {&a[l], &b[l], &c[l]};
        for (int k = 0; k < 3; k++) { snprintf(nm, sizeof nm, names[k], l); ZK_TRY(zk_scratch(ctx, nm, D * 32, dst[k])); }
    }
    for (int l = 0; l < LANES; l++) ZK_TRY(zk_groth16_witness_map_pre_dev(ctx, r, z[l], 1, a[l], b[l], c[l]));     // local: linear in the shares
    ZK_TRY(zk_groth16_msms_begin_dev(ctx, pk, r, z[0]));                          // the share lane's four MSMs over z run under the opens
    // FieldShare::batch_mul of the D-element product (share/field.rs:97-129): open(s + x), open(o + y), the local tail -- per lane
    {
        const void* xa[2] = {a[0], LANES == 2 ? a[1] : nullptr};
        const void* yb[2] = {b[0], LANES == 2 ? b[1] : nullptr};
        void* oa[2] = {a[0], LANES == 2 ? a[1] : nullptr};
        ZK_TRY(zk_shared_beaver_mul(nt, LANES, xa, yb, oa, D, tx, ty, tz, "shared_bv"));
    }
    zk_g1_projective m1[2][4];
    zk_g2_projective m2[2];
    for (int l = 0; l < LANES; l++) {
        ZK_TRY(zk_groth16_witness_map_post_dev(ctx, r, a[l], c[l]));                    // h shares in a[l]
        ZK_TRY(zk_groth16_msms_dev(ctx, pk, r, z[l], a[l], m1[l], &m2[l]));            // party-local MSMs (multi_scale_pub_group; spdz.rs:482-488: twice)
    }
    for (int l = 0; l < LANES; l++) {
        f_r_g1[l].get(); f_s_g1[l].get(); f_s_g2[l].get();
        sh::coeff(K, &P, l, m1[l], m2[l]);
    }
    ZkSmallItems fused[2], opened;
    for (int l = 0; l < LANES; l++) {
        fused[l].fr.resize(2); fused[l].g1.resize(3); fused[l].g2.resize(1);
        sh::fused_items(K, P, l, fused[l].fr.data(), fused[l].g1.data(), fused[l].g2.data());
    }
    ZK_TRY(zk_shared_open_small(nt, LANES, fused, &opened));
    const zk_fr oy_s = opened.fr[0], oy_r = opened.fr[1];
    const SX1 sx_rd = sh::point1(opened.g1[0]), sx_a = sh::point1(opened.g1[1]), sx_b = sh::point1(opened.g1[2]);
    auto p0 = zk_async(ctx, [&] { return sh::scale_finish(leader, sx_rd, oy_s); });       // r s delta            (:115)
    auto p1 = zk_async(ctx, [&] { return sh::scale_finish(leader, sx_a, oy_s); });        // s A                  (:140)
    const SX1 part2 = sh::scale_finish(leader, sx_b, oy_r);                          // r B1                 (:161)
    const SX1 s_a = p1.get();
    const SX1 t = sh::scaled_sum(p0.get(), s_a, part2);
    ZkSmallItems c_share[2], c_opened;                                   // Proof::reveal of C (A and B were opened above)
    for (int l = 0; l < LANES; l++) c_share[l].g1 = {sh::c_share(P, l, t)};
    ZK_TRY(zk_shared_open_small(nt, LANES, c_share, &c_opened));
    sh::write_proof(opened.g1[1], opened.g2[0], c_opened.g1[0], proof);
    if (bytes_sent) *bytes_sent = nt.bytes;
    return ZK_OK;
}

}  // namespace

extern "C" int zk_groth16_prove_shared(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* z_share, const zk_fr* r_share,
                                       const zk_fr* s_share, const void* tx, const void* ty, const void* tz, const zk_net_vtable* net,
                                       uint8_t proof[192], uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !z_share || !r_share || !s_share || !proof) return ZK_ERR_ARG;
    const void* z[2] = {z_share, nullptr};
    const zk_fr *rs[2] = {r_share, nullptr}, *ss[2] = {s_share, nullptr};
    const void *txs[2] = {tx, nullptr}, *tys[2] = {ty, nullptr}, *tzs[2] = {tz, nullptr};
    return prove_shared_impl<1>(ctx, pk, r, z, rs, ss, txs, tys, tzs, net, proof, bytes_sent);
    ZK_API_END
}

extern "C" int zk_groth16_prove_shared_spdz(zk_ctx* ctx, const zk_pk* pk, const zk_r1cs* r, const void* const z_lanes[2],
                                            const zk_fr r_lanes[2], const zk_fr s_lanes[2], const void* const tx_lanes[2],
                                            const void* const ty_lanes[2], const void* const tz_lanes[2], const zk_net_vtable* net,
                                            uint8_t proof[192], uint64_t* bytes_sent) {
    ZK_API_BEGIN(ctx)
    if (!ctx || !pk || !r || !z_lanes || !z_lanes[0] || !z_lanes[1] || !r_lanes || !s_lanes || !proof) return ZK_ERR_ARG;
    const zk_fr *rs[2] = {&r_lanes[0], &r_lanes[1]}, *ss[2] = {&s_lanes[0], &s_lanes[1]};
    const void* none[2] = {nullptr, nullptr};
    return prove_shared_impl<2>(ctx, pk, r, z_lanes, rs, ss, tx_lanes ? tx_lanes : none, ty_lanes ? ty_lanes : none,
                                tz_lanes ? tz_lanes : none, net, proof, bytes_sent);
    ZK_API_END
}

