// sharednet.hip -- what the collaborative provers share (sharednet.hpp): the vector opens and Beaver product, the small open and its test hook
#include "devutil.cuh"
#include "hostfield64.hpp"
#include "internal.hpp"
#include "sharednet.hpp"

using namespace zk;

namespace {

__global__ void __launch_bounds__(256) k_vec_add_const(const void* a, FrK k, void* out, size_t n) {
    const Fr kk = frk(k);
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        fr_store(out, i, fr_add(fr_load(a, i), kk));
}

__global__ void __launch_bounds__(256) k_vec_neg(const void* a, void* out, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        fr_store(out, i, fr_sub(fp_zero<FrParams>(), fr_load(a, i)));
}

}  // namespace
int zk_shared_spdz_open_vec(ZkSharedNet& nt, const void* sh, const void* mac, size_t n, void* out, void* dx) {
    zk_ctx* ctx = nt.ctx;
    ZK_TRY(nt.open_vec(sh, n, out));
    if (ctx->party_id == 0) {
        ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_SUB, out, mac, dx, n));
    } else {
        hipLaunchKernelGGL(k_vec_neg, zk_grid(n, 256), 256, 0, ctx->stream, mac, dx, n);
        ZK_HIP(ctx, hipGetLastError());
    }
    ZK_TRY(nt.open_vec(dx, n, dx));
    int zero = 0;
    ZK_TRY(zk_fr_vec_is_zero_dev(ctx, dx, n, &zero));
    if (!zero) ZK_FAIL(ctx, ZK_ERR_MAC, "SPDZ MAC check failed on a vector open");
    return ZK_OK;
}

int zk_shared_triple_given(int lanes, const void* const tx[2], const void* const ty[2], const void* const tz[2]) {
    const bool dummy = !tx[0] && !ty[0] && !tz[0];
    for (int l = 0; l < lanes; l++)
        if (dummy ? (tx[l] || ty[l] || tz[l]) : (!tx[l] || !ty[l] || !tz[l])) return -1;
    return dummy ? 0 : 1;
}

namespace {
struct BeaverScratch { void *sxl[2], *oyl[2], *sx, *oy, *dx; };      // 2 * lanes + 3 vectors of n elements
int beaver_mul(ZkSharedNet& nt, int lanes, const void* const x[2], const void* const y[2], void* const out[2], size_t n,
               const void* const tx[2], const void* const ty[2], const void* const tz[2], const BeaverScratch& S);
}  // namespace

int zk_shared_beaver_mul(ZkSharedNet& nt, int lanes, const void* const x[2], const void* const y[2], void* const out[2], size_t n,
                         const void* const tx[2], const void* const ty[2], const void* const tz[2], const char* tag) {
    zk_ctx* ctx = nt.ctx;
    if (zk_shared_triple_given(lanes, tx, ty, tz) < 0) ZK_FAIL(ctx, ZK_ERR_ARG, "batch_mul: give a whole Beaver triple (every lane) or none");
    BeaverScratch S;
    char nm[64];
    auto buf = [&](const char* what, int l, void** p) { snprintf(nm, sizeof nm, "%s.%s%d", tag, what, l); return zk_scratch(ctx, nm, n * 32, p); };
    for (int l = 0; l < lanes; l++) { ZK_TRY(buf("sxl", l, &S.sxl[l])); ZK_TRY(buf("oyl", l, &S.oyl[l])); }
    ZK_TRY(buf("sx", 0, &S.sx)); ZK_TRY(buf("oy", 0, &S.oy)); ZK_TRY(buf("dx", 0, &S.dx));
    return beaver_mul(nt, lanes, x, y, out, n, tx, ty, tz, S);
}

int zk_shared_beaver_mul_in(ZkSharedNet& nt, int lanes, const void* const x[2], const void* const y[2], void* const out[2], size_t n,
                            const void* const tx[2], const void* const ty[2], const void* const tz[2], void* scratch) {
    if (zk_shared_triple_given(lanes, tx, ty, tz) < 0) ZK_FAIL(nt.ctx, ZK_ERR_ARG, "batch_mul: give a whole Beaver triple (every lane) or none");
    BeaverScratch S;
    char* p = (char*)scratch;
    auto cut = [&] { void* v = p; p += n * 32; return v; };
    for (int l = 0; l < lanes; l++) { S.sxl[l] = cut(); S.oyl[l] = cut(); }
    S.sx = cut(); S.oy = cut(); S.dx = cut();
    return beaver_mul(nt, lanes, x, y, out, n, tx, ty, tz, S);
}

namespace {
int beaver_mul(ZkSharedNet& nt, int lanes, const void* const x[2], const void* const y[2], void* const out[2], size_t n,
               const void* const tx[2], const void* const ty[2], const void* const tz[2], const BeaverScratch& S) {
    zk_ctx* ctx = nt.ctx;
    const bool dummy = !zk_shared_triple_given(lanes, tx, ty, tz);
    void* const* sxl = S.sxl;
    void* const* oyl = S.oyl;
    void *sx = S.sx, *oy = S.oy, *dx = S.dx;
    const Fr one_ext = fp_mul<FrParams>(fp_one<FrParams>(), fp_const<FrParams>(FrParams::INT_TO_EXT));
    for (int l = 0; l < lanes; l++) {
        if (dummy) {                                      // DummyFieldTripleSource: the leader holds 1 (in both lanes), the rest 0 (wire/field.rs:49-63)
            if (nt.leader()) {
                hipLaunchKernelGGL(k_vec_add_const, zk_grid(n, 256), 256, 0, ctx->stream, x[l], to_frk(one_ext), sxl[l], n);
                hipLaunchKernelGGL(k_vec_add_const, zk_grid(n, 256), 256, 0, ctx->stream, y[l], to_frk(one_ext), oyl[l], n);
                ZK_HIP(ctx, hipGetLastError());
            } else {
                ZK_HIP(ctx, hipMemcpyAsync(sxl[l], x[l], n * 32, hipMemcpyDeviceToDevice, ctx->stream));
                ZK_HIP(ctx, hipMemcpyAsync(oyl[l], y[l], n * 32, hipMemcpyDeviceToDevice, ctx->stream));
            }
        } else {
            ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_ADD, x[l], tx[l], sxl[l], n));
            ZK_TRY(zk_vec_op_launch(ctx, ZK_OP_ADD, y[l], ty[l], oyl[l], n));
        }
    }
    if (lanes == 1) {
        ZK_TRY(nt.open_vec(sxl[0], n, sx));               // open(s + x), open(o + y)
        ZK_TRY(nt.open_vec(oyl[0], n, oy));
    } else {
        ZK_TRY(zk_shared_spdz_open_vec(nt, sxl[0], sxl[1], n, sx, dx));
        ZK_TRY(zk_shared_spdz_open_vec(nt, oyl[0], oyl[1], n, oy, dx));
    }
    // the local tail; the shift of sx * oy lands on the leader in BOTH lanes (mac_share = 1 there)
    for (int l = 0; l < lanes; l++) ZK_TRY(zk_beaver_combine_dev(ctx, sx, oy, tx[l], ty[l], tz[l], out[l], n));
    return ZK_OK;
}
}  // namespace

// ---- the small open's codec -------------------------------------------------------------------------------------------------------
namespace zk_small {
using H1 = Fq64Field;
using H2 = Fq264Field;
void pack(const ZkSmallItems& it, uint64_t* msg) {
    auto put = [&](const void* src, size_t bytes) { if (bytes) memcpy(msg, src, bytes); msg += bytes / 8; };
    put(it.fr.data(), it.fr.size() * sizeof(zk_fr));
    put(it.g1.data(), it.g1.size() * sizeof(zk_g1_projective));
    put(it.g2.data(), it.g2.size() * sizeof(zk_g2_projective));
}
// one group's points of party p's message w added into acc; false: a peer's point is not a valid group element
template <class H>
bool add_points(const uint8_t* msg, size_t n, bool peer, bool subgroup, std::vector<XYZZ<H>>& acc) {
    bool ok = true;
    uint64_t w[3 * H::WORDS / 2];
    for (size_t i = 0; i < n; i++, msg += sizeof w) {
        memcpy(w, msg, sizeof w);
        acc[i] = xyzz_add<H>(acc[i], peer ? host64_peer_point<H>(w, subgroup, ok) : host64_proj_from_abi<H>(w));
    }
    return ok;
}
template <class H, class P>
void write_points(const std::vector<XYZZ<H>>& acc, P* out) {
    const std::vector<Affine<H>> aff = host64_batch_to_affine<H>(acc);
    for (size_t i = 0; i < acc.size(); i++) host64_write_projective<H>(aff[i], (uint64_t*)&out[i]);
}
template <class H, class P>
void write_points(const std::vector<XYZZ<H>>& acc, std::vector<P>& out) {
    out.resize(acc.size());
    write_points<H, P>(acc, out.data());
}
Verdict sum_range(const uint8_t* all, int parties, int self, bool subgroup, size_t nf, size_t n1, size_t n2, const size_t lo[3],
                  const size_t hi[3], ZkSmallItems* out) {
    const size_t len = words(nf, n1, n2) * 8;
    std::vector<Fr> f(hi[0] - lo[0], fp_zero<FrParams>());
    std::vector<XYZZ<H1>> g1(hi[1] - lo[1], xyzz_inf<H1>());
    std::vector<XYZZ<H2>> g2(hi[2] - lo[2], xyzz_inf<H2>());
    for (int p = 0; p < parties; p++) {
        const bool peer = p != self;
        const uint8_t* msg = all + (size_t)p * len;
        for (size_t i = 0; i < f.size(); i++) {
            uint64_t w[4];
            memcpy(w, msg + 32 * (lo[0] + i), 32);
            if (peer && !zk_fr_words_valid(w)) return BAD_SCALAR;
            f[i] = fp_add<FrParams>(f[i], host_load_ext<FrParams>(w));
        }
        if (!add_points<H1>(msg + 32 * nf + 144 * lo[1], g1.size(), peer, subgroup, g1) ||
            !add_points<H2>(msg + 32 * nf + 144 * n1 + 288 * lo[2], g2.size(), peer, subgroup, g2))
            return BAD_POINT;
    }
    for (size_t i = 0; i < f.size(); i++) host_store_ext<FrParams>(out->fr[lo[0] + i].l, f[i]);
    write_points<H1>(g1, out->g1.data() + lo[1]);
    write_points<H2>(g2, out->g2.data() + lo[2]);
    return OK;
}
Verdict sum(const uint8_t* all, int parties, int self, bool subgroup, size_t nf, size_t n1, size_t n2, ZkSmallItems* out) {
    const size_t lo[3] = {0, 0, 0}, hi[3] = {nf, n1, n2};
    out->fr.resize(nf); out->g1.resize(n1); out->g2.resize(n2);
    return sum_range(all, parties, self, subgroup, nf, n1, n2, lo, hi, out);
}
template <class H, class P>
void delta_points(bool leader, const std::vector<P>& opened, const std::vector<P>& mac, std::vector<P>& delta) {
    std::vector<XYZZ<H>> d(opened.size());
    for (size_t i = 0; i < d.size(); i++)
        d[i] = xyzz_add<H>(leader ? host64_proj_from_abi<H>((const uint64_t*)&opened[i]) : xyzz_inf<H>(),
                           xyzz_neg<H>(host64_proj_from_abi<H>((const uint64_t*)&mac[i])));
    write_points<H>(d, delta);
}
void mac_delta(bool leader, const ZkSmallItems& opened, const ZkSmallItems& mac, ZkSmallItems* delta) {
    delta->fr.resize(opened.fr.size());
    for (size_t i = 0; i < opened.fr.size(); i++)
        host_store_ext<FrParams>(delta->fr[i].l, fp_sub<FrParams>(leader ? host_load_ext<FrParams>(opened.fr[i].l) : fp_zero<FrParams>(),
                                                                  host_load_ext<FrParams>(mac.fr[i].l)));
    delta_points<H1>(leader, opened.g1, mac.g1, delta->g1);
    delta_points<H2>(leader, opened.g2, mac.g2, delta->g2);
}
bool all_zero(const ZkSmallItems& it) {
    bool zero = true;
    for (const zk_fr& f : it.fr) zero = zero && fp_is_zero<FrParams>(host_load_ext<FrParams>(f.l));
    for (const zk_g1_projective& p : it.g1) zero = zero && xyzz_is_inf<H1>(host64_proj_from_abi<H1>((const uint64_t*)&p));
    for (const zk_g2_projective& p : it.g2) zero = zero && xyzz_is_inf<H2>(host64_proj_from_abi<H2>((const uint64_t*)&p));
    return zero;
}
}  // namespace zk_small

int zk_shared_open_small(ZkSharedNet& nt, int lanes, const ZkSmallItems items[2], ZkSmallItems* opened) {
    zk_ctx* ctx = nt.ctx;
    const size_t nf = items[0].fr.size(), n1 = items[0].g1.size(), n2 = items[0].g2.size(), words = zk_small::words(nf, n1, n2);
    *opened = ZkSmallItems{};
    if (!words) return ZK_OK;
    std::vector<uint64_t> msg(words);
    std::vector<uint8_t> all;
    auto exchange = [&](const ZkSmallItems& mine, ZkSmallItems* sums) -> int {
        zk_small::pack(mine, msg.data());
        ZK_TRY(nt.gather((const uint8_t*)msg.data(), words * 8, all));
        zk_small::Verdict v = zk_small::OK;
        if (nt.parties() > 1 && n1 + n2 >= ZK_SMALL_PARALLEL_POINTS) {
            // a batch's open: what peers sent is validated item by item (under SPDZ with the subgroup test), over ranges of items
            const size_t tasks = std::min<size_t>(16, std::max(n1, n2));
            std::vector<zk_small::Verdict> vs(tasks, zk_small::OK);
            sums->fr.resize(nf); sums->g1.resize(n1); sums->g2.resize(n2);
            std::vector<ZkTask<void>> ts;
            auto part = [&](size_t t) {
                const size_t lo[3] = {nf * t / tasks, n1 * t / tasks, n2 * t / tasks};
                const size_t hi[3] = {nf * (t + 1) / tasks, n1 * (t + 1) / tasks, n2 * (t + 1) / tasks};
                vs[t] = zk_small::sum_range(all.data(), nt.parties(), ctx->party_id, lanes == 2, nf, n1, n2, lo, hi, sums);
            };
            for (size_t t = 1; t < tasks; t++) ts.push_back(zk_async(ctx, [&part, t] { part(t); }));
            part(0);
            for (auto& t : ts) t.get();
            for (const zk_small::Verdict x : vs) v = std::max(v, x);      // (a bad point outranks a bad scalar: either is ZK_ERR_STATE)
        } else {
            v = zk_small::sum(all.data(), nt.parties(), ctx->party_id, lanes == 2, nf, n1, n2, sums);
        }
        if (v == zk_small::BAD_SCALAR) ZK_FAIL(ctx, ZK_ERR_STATE, "small open: a party sent a non-canonical field element");
        if (v == zk_small::BAD_POINT) ZK_FAIL(ctx, ZK_ERR_STATE, "small open: a party sent a point that is not a valid group element");
        return ZK_OK;
    };
    ZK_TRY(exchange(items[0], opened));
    if (lanes == 2) {
        ZkSmallItems delta, check;
        zk_small::mac_delta(nt.leader(), *opened, items[1], &delta);
        ZK_TRY(exchange(delta, &check));
        if (!zk_small::all_zero(check)) ZK_FAIL(ctx, ZK_ERR_MAC, "SPDZ MAC check failed on a small open");
    }
    return ZK_OK;
}

// ---- the test hook: the exchange(s) of one small open as party `self` sees them, through the codec alone ---------------------------
extern "C" int zk_diag_small_open_host(int parties, int self, int lanes, int subgroup, size_t nf, size_t n1, size_t n2, const uint64_t* shares,
                                       uint64_t* opened, int* verdict) {
    ZK_API_BEGIN_NOCTX
    const size_t words = zk_small::words(nf, n1, n2);
    if (parties < 1 || self < 0 || self >= parties || lanes < 1 || lanes > 2 || !words || words > 4096 || !shares || !opened || !verdict) return ZK_ERR_ARG;
    auto items_of = [&](int lane, int p) {
        const uint64_t* w = shares + ((size_t)lane * parties + p) * words;
        ZkSmallItems it;
        it.fr.resize(nf); it.g1.resize(n1); it.g2.resize(n2);
        if (nf) memcpy(it.fr.data(), w, 32 * nf);
        if (n1) memcpy(it.g1.data(), w + 4 * nf, 144 * n1);
        if (n2) memcpy(it.g2.data(), w + 4 * nf + 18 * n1, 288 * n2);
        return it;
    };
    std::vector<uint64_t> all((size_t)parties * words);
    auto play = [&](const std::vector<ZkSmallItems>& msgs, ZkSmallItems* sums) {
        for (int p = 0; p < parties; p++) zk_small::pack(msgs[p], &all[(size_t)p * words]);
        return zk_small::sum((const uint8_t*)all.data(), parties, self, subgroup != 0, nf, n1, n2, sums) == zk_small::OK;
    };
    std::vector<ZkSmallItems> msgs(parties);
    ZkSmallItems sums, check;
    *verdict = ZK_ERR_STATE;
    for (int p = 0; p < parties; p++) msgs[p] = items_of(0, p);
    if (!play(msgs, &sums)) return ZK_OK;
    zk_small::pack(sums, opened);
    if (lanes == 2) {
        for (int p = 0; p < parties; p++) zk_small::mac_delta(p == 0, sums, items_of(1, p), &msgs[p]);
        if (!play(msgs, &check)) return ZK_OK;
        if (!zk_small::all_zero(check)) { *verdict = ZK_ERR_MAC; return ZK_OK; }
    }
    *verdict = ZK_OK;
    return ZK_OK;
    ZK_API_END
}
