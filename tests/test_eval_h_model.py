"""CPU: the identity behind zk_pk::h_eval / l_eval_pad ("H over coset values"), in Fr with the oracle's field arithmetic.

With e = a o b on the coset, H_i = h_query[i] (i <= D-2), zinv = 1 / Z(g), M the coset-ifft matrix (M_ij = g^-i w^-ij / D) and N the
ifft matrix (N_ir = w^-ir / D), what create_proof adds into C for the quotient is

    sum_{i<=D-2} h_i H_i  =  sum_j e_j H'_j - sum_k z_k K_k,    H'_j = zinv sum_i M_ij H_i,  K_k = zinv sum_r C_rk V_r,  V_r = sum_i N_ir H_i

Both sides are linear in (e, z): it holds for every assignment, satisfying or not.  The scalars tau^i Z(tau) / delta stand in for the
points.  Checked from the definitions, and for the two forms zk_groth16_setup computes the tables by: H' as ONE inverse transform of
(zinv Z(tau) / delta) (tau/g)^i, and V_r = -(u_r / delta) (1 - tau^(D-1) w^r) with u the Lagrange coefficients at tau."""
import pytest

import zkref as O

P = O.R_MOD


def _system(nc, n_pub, n_free, seed):
    """rows <A_i, z> <B_i, z> = c0 o_i + c1 * 1 + c2 * p_1 (+ an earlier variable), solved in order for the new witness o_i: non-unit
    coefficients, C entries in column 0 (the constant) and column 1 (an instance column)."""
    rng = O.Prng(seed)
    z = [1] + [rng.fr() for _ in range(n_pub + n_free)]
    a_rows, b_rows, c_rows = [], [], []
    for i in range(nc):
        nv = len(z)
        a = [(rng.fr(), rng.fr() % nv) for _ in range(3)]
        b = [(rng.fr(), rng.fr() % nv) for _ in range(2)]
        c0, c1, c2, c3 = (2 + rng.fr() % 5), rng.fr(), rng.fr(), rng.fr()
        extra = rng.fr() % nv
        rest = (c1 + c2 * z[1] + c3 * z[extra]) % P
        o = (O.evaluate_constraint(a, z) * O.evaluate_constraint(b, z) - rest) * pow(c0, -1, P) % P
        a_rows.append(a); b_rows.append(b)
        c_rows.append([(c0, nv), (c1, 0), (c2, 1), (c3, extra)])
        z.append(o)
    ni = 1 + n_pub
    return O.R1CS(ni, len(z) - ni, a_rows, b_rows, c_rows), z


def _coset_product(r1cs, z, dom):
    nc, ni, D = r1cs.num_constraints, r1cs.num_instance, dom.size
    a = [O.evaluate_constraint(r1cs.a[i], z) for i in range(nc)] + list(z[:ni]) + [0] * (D - nc - ni)
    b = [O.evaluate_constraint(r1cs.b[i], z) for i in range(nc)] + [0] * (D - nc)
    a, b = dom.coset_fft(dom.ifft(a)), dom.coset_fft(dom.ifft(b))
    return [x * y % P for x, y in zip(a, b)]


@pytest.mark.parametrize("nc,n_pub,n_free,seed", [(5, 1, 2, 11), (11, 2, 3, 12)])       # D = 8 (7 of 8 rows), D = 16 (14 of 16)
def test_h_over_coset_values_equals_h_over_coefficients(nc, n_pub, n_free, seed):
    r1cs, z_sat = _system(nc, n_pub, n_free, seed)
    dom = O.Domain(nc + r1cs.num_instance)
    D, w, g = dom.size, dom.group_gen, dom.generator
    assert D == (8 if nc == 5 else 16) and nc + r1cs.num_instance < D
    assert any(c % P != 1 for row in r1cs.a + r1cs.b + r1cs.c for c, _ in row)
    assert all(any(k == 0 for _, k in row) and any(k == 1 for _, k in row) for row in r1cs.c)
    rng = O.Prng(seed + 100)
    tau, delta = rng.fr(), rng.fr()
    zt = dom.evaluate_vanishing_polynomial(tau)
    di = pow(delta, -1, P)
    H = [zt * di % P * pow(tau, i, P) % P for i in range(D - 1)]                    # h_query's scalars: D - 1 of them
    zinv = pow(dom.evaluate_vanishing_polynomial(g), -1, P)
    winv, ginv, dinv = dom.group_gen_inv, dom.generator_inv, dom.size_inv
    # the tables from the definitions (sums over i <= D-2)
    Hp = [zinv * sum(pow(ginv, i, P) * pow(winv, i * j, P) * dinv * H[i] for i in range(D - 1)) % P for j in range(D)]
    V = [sum(pow(winv, i * r, P) * dinv * H[i] for i in range(D - 1)) % P for r in range(D)]
    nvars1 = r1cs.num_instance + r1cs.num_witness
    K = [0] * nvars1
    for r in range(nc):
        for coeff, k in r1cs.c[r]:
            K[k] = (K[k] + zinv * coeff * V[r]) % P
    assert K[0] != 0 and K[1] != 0                                                   # the constant's term and an instance column's
    # ... and as the setup computes them
    q = tau * ginv % P
    assert Hp == dom.ifft([zinv * zt * di % P * pow(q, i, P) % P for i in range(D - 1)] + [0])
    u = dom.evaluate_all_lagrange_coefficients(tau)
    t_top = pow(tau, D - 1, P)
    assert V == [-(u[r] * di) * (1 - t_top * pow(w, r, P)) % P for r in range(D)]

    z_bad = list(z_sat)
    z_bad[-2] = (z_bad[-2] + 1 + rng.fr()) % P
    z_bad[2] = rng.fr()
    for z, satisfying in ((z_sat, True), (z_bad, False)):
        ok = all(O.evaluate_constraint(r1cs.a[i], z) * O.evaluate_constraint(r1cs.b[i], z) % P == O.evaluate_constraint(r1cs.c[i], z)
                 for i in range(nc))
        assert ok == satisfying
        h = O.witness_map(r1cs, z)
        assert len(h) == D
        lhs = sum(h[i] * H[i] for i in range(D - 1)) % P                              # the min(len) rule drops h[D-1]
        e = _coset_product(r1cs, z, dom)
        rhs = (sum(ej * hj for ej, hj in zip(e, Hp)) - sum(zk * kk for zk, kk in zip(z, K))) % P
        assert rhs == lhs
        if not satisfying:
            # coefficient D-1 is there to be dropped, and both sides drop it: with a D-th point tau^(D-1) Z(tau) / delta the sum differs
            assert h[D - 1] != 0
            assert rhs != (lhs + h[D - 1] * zt * di % P * t_top) % P
        # the L job: l_eval_pad over z[1..] plus the constant's point l_eval_0 = -K_0 (z_0 = 1)
        assert z[0] == 1
        assert sum(zk * kk for zk, kk in zip(z, K)) % P == (K[0] + sum(zk * kk for zk, kk in zip(z[1:], K[1:]))) % P
