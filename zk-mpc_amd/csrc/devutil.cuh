// devutil.cuh -- device-side load/store helpers (16-byte vector accesses) and host conversions.
#pragma once
#include "ec.cuh"

namespace zk {

// ---- Fr in the reference's layout: 8 x u32 (= 4 x u64 LE), Montgomery R = 2^256 ("ext") ----
__device__ __forceinline__ Fr fr_load(const void* base, size_t i) {
    const uint4* p = reinterpret_cast<const uint4*>(base) + 2 * i;
    uint4 a = p[0], b = p[1];
    uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    return fp_unpack<FrParams>(w);
}

__device__ __forceinline__ void fr_store(void* base, size_t i, const Fr& v) {
    uint32_t w[8];
    fp_pack<FrParams>(w, v);
    uint4* p = reinterpret_cast<uint4*>(base) + 2 * i;
    p[0] = make_uint4(w[0], w[1], w[2], w[3]);
    p[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

__device__ __forceinline__ Fr fr_mul(const Fr& a, const Fr& b) { return fp_mul<FrParams>(a, b); }
__device__ __forceinline__ Fr fr_add(const Fr& a, const Fr& b) { return fp_add<FrParams>(a, b); }
__device__ __forceinline__ Fr fr_sub(const Fr& a, const Fr& b) { return fp_sub<FrParams>(a, b); }

// ---- the nine limbs of an internal-form element as plain words: kernel arguments, job structs, chunk totals, table entries ----
ZK_HD Fr limbs_get(const uint32_t* l) {
    Fr r;
#pragma unroll
    for (int i = 0; i < 9; i++) r.l[i] = l[i];
    return r;
}
ZK_HD void limbs_put(uint32_t* l, const Fr& v) {
#pragma unroll
    for (int i = 0; i < 9; i++) l[i] = v.l[i];
}

// ---- a field constant passed to a kernel by value (internal form: nine limbs) ----
struct FrK { uint32_t l[9]; };
__device__ __forceinline__ Fr frk(const FrK& k) { return limbs_get(k.l); }
inline FrK to_frk(const Fr& a) {
    FrK k;
    limbs_put(k.l, a);
    return k;
}

// ---- tables of field constants (ntt.hip: twiddles, coset scales) ----
// Table entries (twiddles, coset scales) are kept as their nine 29-bit limbs, 36 B each: a product takes them as they are
// (re-slicing eight packed words into nine limbs was ~25 instructions in front of every twiddle product).
struct __attribute__((packed, aligned(4))) Limbs9 { uint32_t l[9]; };
__device__ __forceinline__ Fr tab_load(const uint32_t* tab, size_t i) {
    const Limbs9 t = reinterpret_cast<const Limbs9*>(tab)[i];
    return limbs_get(t.l);
}
__device__ __forceinline__ void tab_store(uint32_t* tab, size_t i, const Fr& v) {
    Limbs9 t;
    limbs_put(t.l, v);
    reinterpret_cast<Limbs9*>(tab)[i] = t;
}

// ---- a [9][256] LDS tile of a 256-thread block, limb-major (a wave's b32 accesses hit 64 consecutive words): column get and put ----
__device__ __forceinline__ Fr tile_get(const uint32_t (*t)[256], uint32_t col) {
    Fr r;
#pragma unroll
    for (int k = 0; k < 9; k++) r.l[k] = t[k][col];
    return r;
}
__device__ __forceinline__ void tile_put(uint32_t (*t)[256], uint32_t col, const Fr& v) {
#pragma unroll
    for (int k = 0; k < 9; k++) t[k][col] = v.l[k];
}

// ---- the recurrences of poly.hip's scans, one copy each ----
// Horner over c[lo .. hi) from the top: acc <- acc z + c[i], with each(i, acc) after every step (the division writes Q_i there)
template <class Each>
__device__ __forceinline__ Fr horner_fold(const void* c, size_t lo, size_t hi, const Fr& z, Fr acc, Each each) {
    for (size_t i = hi; i > lo; i--) {
        acc = fr_add(fr_mul(acc, z), fr_load(c, i - 1));
        each(i - 1, acc);
    }
    return acc;
}
__device__ __forceinline__ Fr horner_fold(const void* c, size_t lo, size_t hi, const Fr& z, Fr acc) {
    return horner_fold(c, lo, hi, z, acc, [](size_t, const Fr&) {});
}
// Montgomery's trick over v[lo .. hi) (ext form), zeros stay zero (ff/src/fields/mod.rs:632-658).  Forward: scratch[i] = the
// product of the non-zero elements before i, internal form; returns the chunk's total (one for a chunk of zeros).  Backward: with
// inv = 1 / total, v[i] <- 1 / v[i].
__device__ __forceinline__ Fr inv_chunk_fwd(const void* v, size_t lo, size_t hi, uint32_t* scratch) {
    Fr run = fp_one<FrParams>();
    for (size_t i = lo; i < hi; i++) {
        fr_store(scratch, i, run);
        Fr x = fp_ext_to_int<FrParams>(fr_load(v, i));
        if (!fp_is_zero<FrParams>(x)) run = fr_mul(run, x);
    }
    return run;
}
__device__ __forceinline__ void inv_chunk_bwd(void* v, size_t lo, size_t hi, const uint32_t* scratch, Fr inv) {
    for (size_t i = hi; i-- > lo;) {
        Fr x = fp_ext_to_int<FrParams>(fr_load(v, i));
        if (fp_is_zero<FrParams>(x)) continue;
        Fr xi = fr_mul(inv, fr_load(scratch, i));                            // 1/x, internal form
        inv = fr_mul(inv, x);
        fr_store(v, i, fp_int_to_ext<FrParams>(xi));
    }
}

// ---- packed points (internal form) via 16-byte loads; F::WORDS is a multiple of 4 ----
template <class F>
__device__ __forceinline__ typename F::T felt_load16(const uint32_t* w) {
    uint32_t t[F::WORDS];
    const uint4* p = reinterpret_cast<const uint4*>(w);
#pragma unroll
    for (int i = 0; i < F::WORDS / 4; i++) {
        uint4 v = p[i];
        t[4 * i] = v.x; t[4 * i + 1] = v.y; t[4 * i + 2] = v.z; t[4 * i + 3] = v.w;
    }
    return F::load(t);
}

template <class F>
__device__ __forceinline__ void felt_store16(uint32_t* w, const typename F::T& a) {
    uint32_t t[F::WORDS];
    F::store(t, a);
    uint4* p = reinterpret_cast<uint4*>(w);
#pragma unroll
    for (int i = 0; i < F::WORDS / 4; i++) p[i] = make_uint4(t[4 * i], t[4 * i + 1], t[4 * i + 2], t[4 * i + 3]);
}

template <class F>
__device__ __forceinline__ Affine<F> aff_load16(const uint32_t* base, size_t i) {
    const uint32_t* w = base + i * (2 * F::WORDS);
    return Affine<F>{felt_load16<F>(w), felt_load16<F>(w + F::WORDS)};
}
template <class F>
__device__ __forceinline__ void aff_store16(uint32_t* base, size_t i, const Affine<F>& p) {
    uint32_t* w = base + i * (2 * F::WORDS);
    felt_store16<F>(w, p.x);
    felt_store16<F>(w + F::WORDS, p.y);
}
template <class F>
__device__ __forceinline__ XYZZ<F> xyzz_load16(const uint32_t* base, size_t i) {
    const uint32_t* w = base + i * (4 * F::WORDS);
    return XYZZ<F>{felt_load16<F>(w), felt_load16<F>(w + F::WORDS), felt_load16<F>(w + 2 * F::WORDS),
                   felt_load16<F>(w + 3 * F::WORDS)};
}
template <class F>
__device__ __forceinline__ void xyzz_store16(uint32_t* base, size_t i, const XYZZ<F>& p) {
    uint32_t* w = base + i * (4 * F::WORDS);
    felt_store16<F>(w, p.x);
    felt_store16<F>(w + F::WORDS, p.y);
    felt_store16<F>(w + 2 * F::WORDS, p.zz);
    felt_store16<F>(w + 3 * F::WORDS, p.zzz);
}

// ---- a G1 XYZZ entry in the LDS table of a one-wave block (g1_lincomb.hip, g1_ntt.hip, groth16_verify.hip) ----
// Word-interleaved across the lanes: word i of entry e of lane l at ((e 48 + i) 64 + l) -- whatever entries the lanes pick, a
// wave's access to word i is 64 distinct banks.
constexpr int XW = 4 * G1Field::WORDS;      // 32-bit words of a packed G1 XYZZ point: 48
struct ZkLdsTab {
    uint32_t* base;            // the wave's table + this lane
    __device__ __forceinline__ void put(int e, const XYZZ<G1Field>& p) {
        uint32_t w[XW];
        xyzz_store<G1Field>(w, p);
#pragma unroll
        for (int i = 0; i < XW; i++) base[(e * XW + i) * 64] = w[i];
    }
    __device__ __forceinline__ XYZZ<G1Field> get(int e) const {
        uint32_t w[XW];
#pragma unroll
        for (int i = 0; i < XW; i++) w[i] = base[(e * XW + i) * 64];
        return xyzz_load<G1Field>(w);
    }
};

// ---- host conversions between the C-ABI structs (u64 limbs, ext Montgomery) and Fp ----
template <class P>
inline Fp<P> host_load_ext(const uint64_t* l) {  // raw bits of the external form
    uint32_t w[P::W];
    for (int i = 0; i < P::W / 2; i++) { w[2 * i] = (uint32_t)l[i]; w[2 * i + 1] = (uint32_t)(l[i] >> 32); }
    return fp_unpack<P>(w);
}
template <class P>
inline void host_store_ext(uint64_t* l, const Fp<P>& a) {
    uint32_t w[P::W];
    fp_pack<P>(w, a);
    for (int i = 0; i < P::W / 2; i++) l[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

}  // namespace zk
