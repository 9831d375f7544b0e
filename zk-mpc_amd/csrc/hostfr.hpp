// hostfr.hpp -- Fr on the host, in the internal Montgomery form of the device arithmetic: the one place for the conversions (the
// ABI struct, a 64-bit integer, nine limbs), the 64-bit power, the domain roots and Montgomery's trick.  Every host computation over
// Fr in the library goes through HF; the kernels share fp_pow_u64 (fp29.cuh) and the limb movers (devutil.cuh) with it.
#pragma once
#include "devutil.cuh"
#include "../../include/zkmpc_hip.h"
#include <vector>

namespace zk {

struct HF {
    Fr v;
    static HF zero() { return HF{fp_zero<FrParams>()}; }
    static HF one() { return HF{fp_one<FrParams>()}; }
    static HF from_u64(uint64_t x) {
        Fr t = fp_zero<FrParams>();
        t.l[0] = (uint32_t)(x & MASK29); t.l[1] = (uint32_t)((x >> 29) & MASK29); t.l[2] = (uint32_t)(x >> 58);
        return HF{fp_canon_to_int<FrParams>(t)};
    }
    static HF from_u128(const uint64_t c[2]) {              // lo + 2^64 hi: a fold coefficient of the aggregated verifiers
        static const HF two64 = from_u64((uint64_t)1 << 32).sqr();
        return from_u64(c[0]) + from_u64(c[1]) * two64;
    }
    static HF from_canon_words(const uint32_t w[8]) { return HF{fp_canon_to_int<FrParams>(fp_unpack<FrParams>(w))}; }   // a plain integer below r
    static HF from_abi(const zk_fr& a) { return HF{fp_ext_to_int<FrParams>(host_load_ext<FrParams>(a.l))}; }
    zk_fr abi() const { zk_fr o; host_store_ext<FrParams>(o.l, fp_int_to_ext<FrParams>(v)); return o; }
    static HF from_limbs(const uint32_t* l) { return HF{limbs_get(l)}; }     // nine limbs, as the device keeps a constant
    void limbs(uint32_t* l) const { limbs_put(l, v); }
    HF operator+(const HF& b) const { return HF{fp_add<FrParams>(v, b.v)}; }
    HF operator-(const HF& b) const { return HF{fp_sub<FrParams>(v, b.v)}; }
    HF operator*(const HF& b) const { return HF{fp_mul<FrParams>(v, b.v)}; }
    HF sqr() const { return HF{fp_sqr<FrParams>(v)}; }
    HF neg() const { return HF{fp_neg<FrParams>(v)}; }
    HF inv() const { return HF{fp_inv<FrParams>(v)}; }
    bool is_zero() const { return fp_is_zero<FrParams>(v); }
    bool operator==(const HF& b) const { return fp_eq<FrParams>(v, b.v); }
    HF pow(uint64_t e) const { return HF{fp_pow_u64<FrParams>(v, e)}; }
    // the generator of the subgroup of order 2^log: two_adic_root^(2^(47 - log))   (ff get_root_of_unity; radix2/mod.rs:67-69)
    static HF domain_root(uint32_t log) {
        Fr w = fp_const<FrParams>(FrParams::TWO_ADIC_ROOT);
        for (uint32_t i = log; i < (uint32_t)FR_TWO_ADICITY; i++) w = fp_sqr<FrParams>(w);
        return HF{w};
    }
    // v[i] <- 1 / v[i] by Montgomery's trick (ff/src/fields/mod.rs:597-659): one inversion; zeros stay zero
    static void batch_inverse(HF* v, size_t n) {
        std::vector<HF> pre(n);
        HF run = one();
        for (size_t i = 0; i < n; i++) {
            pre[i] = run;
            if (!v[i].is_zero()) run = run * v[i];
        }
        HF inv = run.inv();
        for (size_t i = n; i-- > 0;) {
            if (v[i].is_zero()) continue;
            const HF t = inv * pre[i];
            inv = inv * v[i];
            v[i] = t;
        }
    }
    void bytes(std::vector<uint8_t>& out) const {          // Fp::write: into_repr(), little endian
        uint32_t w[8];
        canon_words(w);
        for (int i = 0; i < 8; i++) for (int b = 0; b < 4; b++) out.push_back((uint8_t)(w[i] >> (8 * b)));
    }
    void canon_words(uint32_t w[8]) const { fp_pack<FrParams>(w, fp_int_to_canon<FrParams>(v)); }   // the plain integer below r
    // four little-endian 64-bit words are below r (is_valid, ff/src/fields/macros.rs:255-260; r from the generated constants, where
    // rng.hip's zk_fr_words_valid has it typed in)
    static bool words_below_r(const uint64_t l[4]) {
        uint32_t r[8];
        fp_pack<FrParams>(r, fp_const<FrParams>(FrParams::P));
        for (int i = 3; i >= 0; i--) {
            const uint64_t ri = r[2 * i] | ((uint64_t)r[2 * i + 1] << 32);
            if (l[i] != ri) return l[i] < ri;
        }
        return false;
    }
};

}  // namespace zk
