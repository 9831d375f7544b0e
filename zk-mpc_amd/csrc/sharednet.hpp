// sharednet.hpp -- what the collaborative provers (groth16_shared.hip, marlin_prove.hip, mpc_host.hip) share, defined in sharednet.hip: the
// party's transport behind zk_net_vtable, the MAC-checked vector open, the vector Beaver product, and the ONE small open of O(1) scalars, G1 and
// G2 points with its wire layout, its validation of what peers sent and its MAC check.  Replaces MpcSerNet::broadcast (mpc-algebra/src/
// channel.rs:12-28), AdditiveFieldShare / SpdzFieldShare::batch_open (share/additive.rs:124-131, share/spdz.rs:177-196), the group shares' open
// (share/spdz.rs:312-336) and FieldShare::batch_mul (share/field.rs:97-129).
#pragma once
#include "../../include/zkmpc_hip.h"
#include "ctx.hpp"
#include <string.h>
#include <vector>

struct ZkSharedNet {
    zk_ctx* ctx;
    const zk_net_vtable* vt;
    size_t bytes = 0;                       // payload bytes this party contributed to opens
    int parties() const { return ctx->n_parties; }
    bool leader() const { return ctx->party_id == 0; }
    // all[p * len ..] = party p's bytes (MpcNet::broadcast_bytes); a single party needs no transport
    int gather(const uint8_t* mine, size_t len, std::vector<uint8_t>& all) {
        all.resize((size_t)parties() * len);
        bytes += len;
        if (parties() == 1) { memcpy(all.data(), mine, len); return ZK_OK; }
        if (!vt || !vt->all_gather_bytes) ZK_FAIL(ctx, ZK_ERR_ARG, "collaborative prover: several parties need zk_net_vtable::all_gather_bytes");
        if (vt->all_gather_bytes(vt->user, mine, len, all.data()) != 0) ZK_FAIL(ctx, ZK_ERR_STATE, "collaborative prover: all_gather_bytes failed");
        return ZK_OK;
    }
    // out = sum over parties of v (n field elements on the device); out may alias v
    int open_vec(const void* v, size_t n, void* out) {
        bytes += n * 32;
        if (vt && vt->open_sum_fr_dev) {
            ZK_HIP(ctx, hipStreamSynchronize(ctx->stream));             // the callback may use its own stream
            if (vt->open_sum_fr_dev(vt->user, v, n, out) != 0) ZK_FAIL(ctx, ZK_ERR_STATE, "collaborative prover: open_sum_fr_dev callback failed");
            return ZK_OK;
        }
        if (parties() == 1) {
            if (out != v) ZK_HIP(ctx, hipMemcpyAsync(out, v, n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            return ZK_OK;
        }
        return zk_open_sum_fr_dev(ctx, v, n, out);
    }
};

// SpdzFieldShare::batch_open on a device vector (key alpha = 1 held by the leader): out = open(share lane); then every party
// publishes [leader ? out : 0] - mac (into dx, n elements of scratch) and the sum must vanish -- otherwise ZK_ERR_MAC.
int zk_shared_spdz_open_vec(ZkSharedNet& nt, const void* sh, const void* mac, size_t n, void* out, void* dx);
// A whole Beaver triple (every lane) or none: 1 = given, 0 = none (DummyFieldTripleSource), -1 = some pointers only (ZK_ERR_ARG)
int zk_shared_triple_given(int lanes, const void* const tx[2], const void* const ty[2], const void* const tz[2]);
// FieldShare::batch_mul on device vectors, lanes = 1 (additive) or 2 (SPDZ: share lane, MAC lane): out[l] = shares of x * y.
// tx / ty / tz: this party's Beaver triple shares per lane, or all NULL for DummyFieldTripleSource (the leader holds 1 in every
// lane).  out[l] may alias x[l].  scratch: 2 * lanes + 3 vectors of n elements, named by `tag` in the context's arena.
int zk_shared_beaver_mul(ZkSharedNet& nt, int lanes, const void* const x[2], const void* const y[2], void* const out[2], size_t n,
                         const void* const tx[2], const void* const ty[2], const void* const tz[2], const char* tag);
// The same with the scratch in a buffer of the caller's: (2 * lanes + 3) * n elements (a batch's product grows with its count and
// is an allocation of that call, not of the arena)
int zk_shared_beaver_mul_in(ZkSharedNet& nt, int lanes, const void* const x[2], const void* const y[2], void* const out[2], size_t n,
                            const void* const tx[2], const void* const ty[2], const void* const tz[2], void* scratch);

// ---- the small open: O(1) values per exchange, summed over the parties ----------------------------------------------------------
// Items travel in ABI form, which is the wire form: fr | g1 | g2 at 4 / 18 / 36 words per item (mpc.py: Party._open_many).
struct ZkSmallItems {
    std::vector<zk_fr> fr;
    std::vector<zk_g1_projective> g1;
    std::vector<zk_g2_projective> g2;
};
// The codec: host arithmetic only -- no context, no transport, no HIP call.
namespace zk_small {
enum Verdict { OK, BAD_SCALAR, BAD_POINT };      // a peer's scalar not below r / a peer's point that is not a valid group element
inline size_t words(size_t nf, size_t n1, size_t n2) { return 4 * nf + 18 * n1 + 36 * n2; }
void pack(const ZkSmallItems& items, uint64_t* msg);
// all = `parties` messages of words(nf, n1, n2) back to back; out = the sums, points normalised (host64_write_projective).  What a PEER sent
// must be: scalars below r; coordinates below q, Z = 0 or Montgomery one, on the curve and -- `subgroup`: under SPDZ -- in the prime-order
// subgroup (hostfield64.hpp: host64_peer_point).  The slot of `self` is this party's own output and taken as is.
Verdict sum(const uint8_t* all, int parties, int self, bool subgroup, size_t nf, size_t n1, size_t n2, ZkSmallItems* out);
// The same for the items [lo[k], hi[k]) of each kind k = 0 (fr), 1 (g1), 2 (g2) alone, into *out sized for all of them already: items are
// validated and summed one by one, so disjoint ranges may run side by side (zk_shared_open_small: a batch's open over the helper threads)
Verdict sum_range(const uint8_t* all, int parties, int self, bool subgroup, size_t nf, size_t n1, size_t n2, const size_t lo[3],
                  const size_t hi[3], ZkSmallItems* out);
void mac_delta(bool leader, const ZkSmallItems& opened, const ZkSmallItems& mac, ZkSmallItems* delta);   // [leader ? opened : 0] - mac
bool all_zero(const ZkSmallItems& items);
}  // namespace zk_small
// The driver: items[0] = this party's shares, ONE gather of 8 * words bytes, *opened = the sums (Additive{Field,Group}Share::open).  lanes = 2
// (SPDZ): items[1] = the MAC shares; a second gather publishes the deltas and every sum must vanish (SpdzFieldShare::batch_open, SpdzGroupShare::
// open, key alpha = 1 held by the leader) -- otherwise ZK_ERR_MAC.  An invalid payload from a peer is ZK_ERR_STATE.  No items: no exchange.
// An open of ZK_SMALL_PARALLEL_POINTS points or more (a batch's) validates and sums over ranges of items on at most 16 helper threads.
constexpr size_t ZK_SMALL_PARALLEL_POINTS = 8;
int zk_shared_open_small(ZkSharedNet& nt, int lanes, const ZkSmallItems items[2], ZkSmallItems* opened);
