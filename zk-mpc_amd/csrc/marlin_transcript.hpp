// marlin_transcript.hpp -- Marlin's Fiat-Shamir transcript, which prover and verifier must derive alike (arkworks/marlin/src/lib.rs:
// 152-319 and 324-442, ahp/verifier.rs:42-95): the seed "MARLIN-2019" | index_vk | public input; round 1's commitments -> alpha
// outside H, eta_a, eta_b, eta_c; round 2's -> beta outside H; round 3's -> gamma; the evaluations -> xi = u128::rand.  The provers
// (marlin_prove_int.hpp: ProofState) and the verifier (marlin_verify.hip: build_equations) go through this one statement, and rng.hip's
// zk_rng_next_fr draws its field elements with fr_rand.  Host code only.
#pragma once
#include "fsrng.hpp"
#include "marlin_bytes.hpp"
#include "marlin_lc.hpp"
#include <vector>

namespace zk {
namespace marlin {

// F::rand for Fr (ff/src/fields/arithmetic.rs:200-219): four u64 in limb order, the top 3 bits masked away, rejected unless below the
// modulus; the accepted words ARE the element's in-memory (Montgomery) form.
inline zk_fr fr_rand(zkfs::ChaChaRng& r) {
    for (;;) {
        zk_fr o;
        for (int i = 0; i < 4; i++) o.l[i] = r.next_u64();
        o.l[3] &= 0xffffffffffffffffull >> 3;
        if (HF::words_below_r(o.l)) return o;
    }
}

struct Transcript {
    zkfs::FiatShamirRng fs{};
    struct Round1 { HF alpha, eta[3]; };              // eta: a, b, c

    Transcript() = default;
    // pub: the public input, its leading 1 included
    Transcript(const uint8_t* ivk, size_t ivk_len, const std::vector<HF>& pub) {
        const char* name = "MARLIN-2019";
        std::vector<uint8_t> seed(name, name + 11);
        seed.insert(seed.end(), ivk, ivk + ivk_len);
        for (size_t i = 1; i < pub.size(); i++) pub[i].bytes(seed);
        fs = zkfs::FiatShamirRng::from_seed(seed.data(), seed.size());
    }
    // comms: the round's commitments in the order the round commits them
    Round1 round1(const Comm* comms, size_t n, const Dom& H) {
        absorb(comms, n);
        Round1 c;
        c.alpha = outside(H);
        for (HF& e : c.eta) e = next();
        return c;
    }
    HF round2(const Comm* comms, size_t n, const Dom& H) { absorb(comms, n); return outside(H); }
    HF round3(const Comm* comms, size_t n) { absorb(comms, n); return next(); }
    // the evaluations as the proof writes them (32 canonical bytes each); the opening challenge: u128::rand(&mut fs_rng).into(), low half first
    HF evaluations(const uint8_t* bytes, size_t len) {
        fs.absorb(bytes, len);
        const uint64_t w[2] = {fs.r.next_u64(), fs.r.next_u64()};
        return HF::from_u128(w);
    }
    HF evaluations(const std::vector<HF>& ev) {
        std::vector<uint8_t> bytes;
        for (const HF& e : ev) e.bytes(bytes);
        return evaluations(bytes.data(), bytes.size());
    }

private:
    HF next() { return HF::from_abi(fr_rand(fs.r)); }
    HF outside(const Dom& d) {                        // sampled until v_d(t) != 0 (the challenges alpha, beta)
        HF t = next();
        while (d.vanishing(t).is_zero()) t = next();
        return t;
    }
    void absorb(const Comm* comms, size_t n) {        // to_bytes![comms, EmptyMessage]
        std::vector<uint8_t> bytes;
        for (size_t i = 0; i < n; i++) comm_tobytes(comms[i], bytes);
        fs.absorb(bytes);
    }
};

}  // namespace marlin
}  // namespace zk
