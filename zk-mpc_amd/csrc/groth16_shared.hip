// groth16_shared.hip -- create_proof over additive / SPDZ shares as one C-ABI call.
#include "../../include/zkmpc_hip.h"
#include "groth16_int.hpp"
#include "sharednet.hpp"

using namespace zk;

// ---- the collaborative prover as ONE entry point ---------------------------------------------------------------------------------
// create_proof::<MpcPairingEngine, C> over additive shares (src/groth16.rs:68-183): what mpc.py::Party.create_proof_shared
// sequences from ~40 calls, for a host that cannot call Python.  This file is the protocol; the transport, the Beaver product
// with its vector opens and the small open (wire layout, validation of peers' payloads, MAC check) are sharednet.hpp's.  Opens
// happen in the fused order of create_proof_shared: the nine small opens of the three GroupShare::scale calls
// (share/group.rs:72-111, DummyGroupTripleSource) and of Proof::reveal travel in two small opens; every opened value is the
// reference's, and so are the 192 bytes.
namespace {

using SH1 = Fq64Field;
using SH2 = Fq264Field;
using SX1 = XYZZ<SH1>;
using SX2 = XYZZ<SH2>;

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
    uint32_t rw[2][8], sw[2][8];
    for (int l = 0; l < LANES; l++) { fr_abi_to_canon_words(rs[l]->l, rw[l]); fr_abi_to_canon_words(ss[l]->l, sw[l]); }
    const SX1 delta1 = xyzz_from_affine<SH1>(aff_to_host64<G1Field>(pk->delta_g1));
    const SX2 delta2 = xyzz_from_affine<SH2>(aff_to_host64<G2Field>(pk->delta_g2));
    // public point x shared scalar: local host arithmetic (scale_pub_group, share/additive.rs:502-508), under the device work
    ZkTask<SX1> f_r_g1[2], f_s_g1[2];                  // (joining handles: the tasks reference this frame and are waited for when it is left)
    ZkTask<SX2> f_s_g2[2];
    for (int l = 0; l < LANES; l++) {
        f_r_g1[l] = zk_async(ctx, [&, l] { return host64_scalar_mul<SH1>(delta1, rw[l]); });
        f_s_g1[l] = zk_async(ctx, [&, l] { return host64_scalar_mul<SH1>(delta1, sw[l]); });
        f_s_g2[l] = zk_async(ctx, [&, l] { return host64_scalar_mul<SH2>(delta2, sw[l]); });
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
    auto pub1 = [&](const Affine<G1Field>& p) { return leader ? xyzz_from_affine<SH1>(aff_to_host64<G1Field>(p)) : xyzz_inf<SH1>(); };   // shift(): leader only
    auto pub2 = [&](const Affine<G2Field>& p) { return leader ? xyzz_from_affine<SH2>(aff_to_host64<G2Field>(p)) : xyzz_inf<SH2>(); };
    SX1 h_acc[2], l_acc[2], r_g1[2], g_a[2], g1_b[2];
    SX2 g2_b[2];
    for (int l = 0; l < LANES; l++) {
        h_acc[l] = host64_proj_from_abi<SH1>((const uint64_t*)&m1[l][0]);
        l_acc[l] = host64_proj_from_abi<SH1>((const uint64_t*)&m1[l][1]);
        const SX1 a_acc = host64_proj_from_abi<SH1>((const uint64_t*)&m1[l][2]), b1_acc = host64_proj_from_abi<SH1>((const uint64_t*)&m1[l][3]);
        const SX2 b2_acc = host64_proj_from_abi<SH2>((const uint64_t*)&m2[l]);
        r_g1[l] = f_r_g1[l].get();
        g_a[l] = xyzz_add<SH1>(xyzz_add<SH1>(xyzz_add<SH1>(r_g1[l], pub1(pk->a0)), a_acc), pub1(pk->alpha_g1));                 // calculate_coeff (:185-201)
        g1_b[l] = xyzz_add<SH1>(xyzz_add<SH1>(xyzz_add<SH1>(f_s_g1[l].get(), pub1(pk->b0_g1)), b1_acc), pub1(pk->beta_g1));
        g2_b[l] = xyzz_add<SH2>(xyzz_add<SH2>(xyzz_add<SH2>(f_s_g2[l].get(), pub2(pk->b0_g2)), b2_acc), pub2(pk->beta_g2));
    }
    // the fused open: open(o + y) for o = s, r (y = the leader's 1: the dummy group triple; from_add_shared: mac = share), open(s + x)
    // for the three scaled points (x = 0) and the reveal of B
    const Fr y = leader ? fp_mul<FrParams>(fp_one<FrParams>(), fp_const<FrParams>(FrParams::INT_TO_EXT)) : fp_zero<FrParams>();
    auto plus_y = [&](const zk_fr* v) { zk_fr o; host_store_ext<FrParams>(o.l, fp_add<FrParams>(host_load_ext<FrParams>(v->l), y)); return o; };
    auto abi1 = [](const SX1& p) { zk_g1_projective o; host64_write_projective<SH1>(xyzz_to_affine<SH1>(p), (uint64_t*)&o); return o; };
    auto abi2 = [](const SX2& p) { zk_g2_projective o; host64_write_projective<SH2>(xyzz_to_affine<SH2>(p), (uint64_t*)&o); return o; };
    auto point1 = [](const zk_g1_projective& p) { return host64_proj_from_abi<SH1>((const uint64_t*)&p); };
    ZkSmallItems fused[2], opened;
    for (int l = 0; l < LANES; l++) fused[l] = {{plus_y(ss[l]), plus_y(rs[l])}, {abi1(r_g1[l]), abi1(g_a[l]), abi1(g1_b[l])}, {abi2(g2_b[l])}};
    ZK_TRY(zk_shared_open_small(nt, LANES, fused, &opened));
    const Fr oy_s = host_load_ext<FrParams>(opened.fr[0].l), oy_r = host_load_ext<FrParams>(opened.fr[1].l);
    const SX1 sx_rd = point1(opened.g1[0]), sx_a = point1(opened.g1[1]), sx_b = point1(opened.g1[2]);
    // the local part of GroupShare::scale behind its two opens: z - sx*y (+ sx*oy on the leader), z = 0, y = [leader]; both SPDZ
    // lanes hold the same value (key 1)
    auto scale_finish = [&](const SX1& sxp, const Fr& oyv) {
        if (!leader) return xyzz_inf<SH1>();
        uint64_t l4[4];
        uint32_t kw[8];
        host_store_ext<FrParams>(l4, oyv);
        fr_abi_to_canon_words(l4, kw);
        return xyzz_add<SH1>(host64_scalar_mul<SH1>(sxp, kw), xyzz_neg<SH1>(sxp));
    };
    auto p0 = zk_async(ctx, [&] { return scale_finish(sx_rd, oy_s); });       // r s delta            (:115)
    auto p1 = zk_async(ctx, [&] { return scale_finish(sx_a, oy_s); });        // s A                  (:140)
    const SX1 part2 = scale_finish(sx_b, oy_r);                          // r B1                 (:161)
    SX1 t = xyzz_add<SH1>(p1.get(), part2);
    t = xyzz_add<SH1>(t, xyzz_neg<SH1>(p0.get()));
    ZkSmallItems c_share[2], c_opened;                                   // Proof::reveal of C (A and B were opened above)
    for (int l = 0; l < LANES; l++) c_share[l].g1 = {abi1(xyzz_add<SH1>(xyzz_add<SH1>(t, l_acc[l]), h_acc[l]))};      // :169-174
    ZK_TRY(zk_shared_open_small(nt, LANES, c_share, &c_opened));
    // (opened points come normalised: zz = zzz = 1 or all zero, so x and y are the affine point)
    const SX2 B = host64_proj_from_abi<SH2>((const uint64_t*)&opened.g2[0]);
    const SX1 C = point1(c_opened.g1[0]);
    g1_serialize(aff_from_host64<G1Field>(Affine<SH1>{sx_a.x, sx_a.y}), proof);
    g2_serialize(aff_from_host64<G2Field>(Affine<SH2>{B.x, B.y}), proof + 48);
    g1_serialize(aff_from_host64<G1Field>(Affine<SH1>{C.x, C.y}), proof + 144);
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

