// g1_ntt.cuh -- one butterfly of a radix-2 transform over G1 POINTS, written once for the device kernels (g1_ntt.hip, one butterfly
// per lane) and for the host (its test hook, over Fq64Field with a plain loop around it).
//
// A butterfly takes (a, b) in XYZZ form and a twiddle w of 256 raw bits and leaves (a + w b, a - w b): ONE full-width scalar
// multiplication t = w b, then two complete additions.  The multiplication is the fixed schedule of g1_lincomb.cuh with 3-bit
// windows instead of 4-bit ones, because the operand is an XYZZ point and the table of its multiples sits in LDS: four entries
// (1 b .. 4 b) are 768 bytes per lane, 48 KiB per wave, three waves per CU; eight entries would leave one.
//   k + 0b100100...100 = sum n_w 8^w (86 digits cover 258 bits; k < 2^256 leaves no carry)   =>   k = sum (n_w - 4) 8^w
// so every digit is in [-4, 3].  Every lane of a wave runs the same sequence -- the table, then per window three doublings and ONE
// complete addition -- whatever its twiddle is: the digit only selects the operand.  No endomorphism: the points may be outside the
// prime-order subgroup.  All additions are ec.cuh's complete xyzz_add: a = t (a doubling), a = -t (a cancellation) and infinity
// on either side are ordinary inputs of a butterfly (an input that is one point everywhere meets both at the first level).
#pragma once
#include "ec.cuh"

namespace zk {

constexpr int G1NTT_TAB = 4;            // table entries per butterfly: e holds (e + 1) b
constexpr int G1NTT_WINDOWS = 86;       // 3-bit windows over 258 bits

// Tab: void put(int e, const XYZZ<F>&), XYZZ<F> get(int e) for e < G1NTT_TAB (LDS on the device, a local array on the host)
template <class F, class Tab>
ZK_HD XYZZ<F> g1_ntt_mul(const XYZZ<F>& P, const uint32_t k[8], Tab& tab) {
    // kk = (k + bias) << 30 in nine words: the top digit (bits 255 .. 257) ends at the top of kk[8]
    uint32_t kk[9], carry = 0;
#pragma unroll
    for (int i = 0; i < 9; i++) {
        uint32_t bias = 0;                                   // bit 3 w + 2 of every window
#pragma unroll
        for (int b = 0; b < 32; b++)
            if ((32 * i + b) % 3 == 2 && 32 * i + b < 3 * G1NTT_WINDOWS) bias |= 1u << b;
        const uint64_t t = (uint64_t)(i < 8 ? k[i] : 0u) + bias + carry;
        kk[i] = (uint32_t)t;
        carry = (uint32_t)(t >> 32);
    }
#pragma unroll
    for (int i = 8; i > 0; i--) kk[i] = (kk[i] << 30) | (kk[i - 1] >> 2);
    kk[0] <<= 30;
    XYZZ<F> e = P;
    tab.put(0, e);
#pragma unroll 1
    for (int i = 1; i < G1NTT_TAB; i++) {
        e = xyzz_add<F>(e, P);
        tab.put(i, e);
    }
    XYZZ<F> acc = xyzz_inf<F>();
#pragma unroll 1
    for (int w = G1NTT_WINDOWS - 1; w >= 0; w--) {
#pragma unroll 1
        for (int j = 0; j < 3; j++) acc = xyzz_dbl<F>(acc);
        const int d = (int)(kk[8] >> 29) - 4;
#pragma unroll
        for (int i = 8; i > 0; i--) kk[i] = (kk[i] << 3) | (kk[i - 1] >> 29);
        kk[0] <<= 3;
        const int m = d < 0 ? -d : d;
        XYZZ<F> t = tab.get(m ? m - 1 : 0);
        t.y = F::select(d < 0, F::neg(t.y), t.y);
        t.zz = F::select(m == 0, F::zero(), t.zz);          // a zero digit adds infinity
        acc = xyzz_add<F>(acc, t);
    }
    return acc;
}

// (a, b) <- (a + w b, a - w b)
template <class F, class Tab>
ZK_HD void g1_ntt_butterfly(XYZZ<F>& a, XYZZ<F>& b, const uint32_t w[8], Tab& tab) {
    const XYZZ<F> t = g1_ntt_mul<F>(b, w, tab);
    b = xyzz_add<F>(a, xyzz_neg<F>(t));
    a = xyzz_add<F>(a, t);
}

// The schedule both sides run: the input in bit-reversed order, then level s = 0 .. log_n - 1 with half = 2^s; butterfly j of a
// level (j < n / 2) pairs lo = (j / half) 2 half + j % half with lo + half under twiddle number (j % half) (n / (2 half)).
ZK_HD uint32_t g1_ntt_bitrev(uint32_t i, uint32_t log_n) {
    uint32_t r = 0;
    for (uint32_t b = 0; b < log_n; b++) r |= ((i >> b) & 1u) << (log_n - 1 - b);
    return r;
}
ZK_HD void g1_ntt_pair(uint32_t j, uint32_t s, uint32_t log_n, uint32_t* lo, uint32_t* tw) {
    const uint32_t half = 1u << s, in = j & (half - 1);
    *lo = ((j >> s) << (s + 1)) + in;
    *tw = in << (log_n - 1 - s);
}

}  // namespace zk
