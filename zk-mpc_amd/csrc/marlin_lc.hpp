// marlin_lc.hpp -- what Marlin's prover and verifier must derive alike on the host (over hostfr.hpp's Fr): the evaluation domains and the
// coefficients of AHPForR1CS::construct_linear_combinations (arkworks/marlin/src/ahp/mod.rs:112-290).  marlin_prove.hip builds its
// query set from them and marlin_verify.hip its pairing equations: one statement, so the two cannot drift.
#pragma once
#include "hostfr.hpp"

namespace zk {

struct Dom {
    size_t size; uint32_t log; HF gen;
    explicit Dom(size_t num_coeffs) {
        log = 0;
        while (((size_t)1 << log) < num_coeffs) log++;
        size = (size_t)1 << log;
        gen = HF::domain_root(log);
    }
    HF vanishing(const HF& t) const { return t.pow(size) - HF::one(); }
};

// ---- construct_linear_combinations: the coefficients that are not 1 ----------------------------------------------------------
// In: the challenges, the seven evaluations of the proof (d = a_denom, b_denom, c_denom at gamma; the others at their query points)
// and x = the formatted public input (1 | inputs, |X| values).
struct MarlinLcIn {
    HF alpha, eta[3], beta, gamma;
    HF z_b_beta, t_beta, g_1_beta, g_2_gamma, d[3];
    const HF* x;
};
// outer_sumcheck = mask_poly + z_a * z_a + outer_c_zb - ... in the reference's term order:
//   mask_poly, z_a z_a, outer_c_zb (One), w w, outer_c_x (One), h_1 h_1, outer_c_g1 (One)
// inner_sumcheck = val[0] a_val + val[1] b_val + val[2] c_val + inner_c (One) + h_2 h_2
// m_denom        = ba (One) - alpha m_row - beta m_col + m_row_col
struct MarlinLc {
    HF z_a, outer_c_zb, w, outer_c_x, h_1, outer_c_g1;
    HF val[3], inner_c, h_2;
    HF ba;
};
inline MarlinLc marlin_lc(const Dom& H, const Dom& K, const Dom& X, const MarlinLcIn& in) {
    const HF one = HF::one();
    const HF &alpha = in.alpha, &beta = in.beta, &gamma = in.gamma;
    const size_t n = H.size, ni = X.size;
    const HF v_h_alpha = H.vanishing(alpha), v_h_beta = H.vanishing(beta), v_x_beta = beta.pow(ni) - one;
    const HF r_alpha_at_beta = (alpha == beta) ? HF::from_u64(n) * alpha.pow(n - 1) : (v_h_alpha - v_h_beta) * (alpha - beta).inv();
    HF x_beta = HF::zero(), g = one;                                           // the public input's polynomial at beta
    if (v_x_beta.is_zero()) {
        for (size_t k = 0; k < ni; k++, g = g * X.gen) if (g == beta) x_beta = in.x[k];
    } else {
        const HF l0 = v_x_beta * HF::from_u64(ni).inv();
        for (size_t k = 0; k < ni; k++, g = g * X.gen) x_beta = x_beta + in.x[k] * (l0 * g * (beta - g).inv());
    }
    MarlinLc c;
    c.ba = beta * alpha;
    c.z_a = r_alpha_at_beta * (in.eta[0] + in.eta[2] * in.z_b_beta);
    c.outer_c_zb = r_alpha_at_beta * in.eta[1] * in.z_b_beta;
    c.w = (in.t_beta * v_x_beta).neg();
    c.outer_c_x = (in.t_beta * x_beta).neg();
    c.h_1 = v_h_beta.neg();
    c.outer_c_g1 = (beta * in.g_1_beta).neg();
    const HF vv = v_h_alpha * v_h_beta;
    const HF da = in.d[0], db = in.d[1], dc = in.d[2], b_expr = da * db * dc * (gamma * in.g_2_gamma + in.t_beta * HF::from_u64(K.size).inv());
    c.val[0] = in.eta[0] * db * dc * vv;
    c.val[1] = in.eta[1] * da * dc * vv;
    c.val[2] = in.eta[2] * db * da * vv;
    c.inner_c = b_expr.neg();
    c.h_2 = K.vanishing(gamma).neg();
    return c;
}

}  // namespace zk
