"""Aggregated Groth16 verification through the HOST instantiation (zk_groth16_verify_aggregate_host): count proofs of one key as one
folded pairing product with 128-bit coefficients r_i,

    prod_i e(r_i A_i, B_i) . e(sum r_i C_i, -delta) . e(sum_j s_j gamma_abc[j], -gamma) . e(s_0 alpha, -beta) = 1.

Six proofs of the D = 8 golden key (pairing_cases.golden_verifier) over two assignments and six (r, s), from the oracle's
known-trapdoor prediction.  The folded value of a failing batch is held, coefficient by coefficient in the w-basis, to the oracle's
value computed another way: (prod_i V_i^{r_i})^3 with V_i the reference's own left side over right side of proof i."""
import ctypes as C
import functools

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import _lib, api
from helpers import ih, r1cs_from_json, trapdoor_from_json
from marlin_verify_cases import cofactor_torsion_point
from pairing_cases import flip_sign, golden_verifier

N_PROOFS = 6
ENDS = [1, 2, 2 ** 64 - 1, 2 ** 64, 2 ** 128 - 1]
SEED = bytes(range(32))
ZK_ERR_ARG = -2


@functools.lru_cache(maxsize=None)
def six():
    """[(A, B, C), ...], [inputs, ...]: proofs 0, 2, 4 over one assignment of the mul-chain system, 1, 3, 5 over another."""
    v = golden_verifier()
    r1cs, td = r1cs_from_json(v.j), trapdoor_from_json(v.j["trapdoor"])
    pks = O.ProvingKeyScalars(r1cs, td)
    zs = [[ih(x) for x in v.j["z"]], O.mul_chain_r1cs(5, 11, 13)[1]]
    assert len(zs[1]) == len(zs[0]) and zs[1][1] != zs[0][1]
    rng = O.Prng(0xA66)
    proofs, inputs = [], []
    for k in range(N_PROOFS):
        z = zs[k % 2]
        proofs.append(O.predict_proof(r1cs, pks, z, rng.fr(), rng.fr()))
        inputs.append(z[1:v.j["num_instance"]])
    for p, x in zip(proofs[:2], inputs[:2]):
        assert O.verify_proof(v.opk, p, x)
    return proofs, inputs


def seeded_coeffs(n=N_PROOFS):
    return [int(lo) | (int(hi) << 64) for lo, hi in api.verify_aggregate_coeffs_from_seed(SEED, n)]


def run(proofs, inputs, coeffs):
    v = golden_verifier()
    data = [p if isinstance(p, bytes) else O.proof_serialize(*p) for p in proofs]
    inp = np.stack([cv.fr_to_mont(x) for x in inputs])
    return api.groth16_verify_aggregate_host(inputs_mont=inp, proofs=data, coeffs=coeffs, **v.vk)


# ---- the oracle's value of the fold, another way ----
@functools.lru_cache(maxsize=None)
def ml_alpha_beta():
    v = golden_verifier()
    return tuple(O.miller_loop(O.g1_neg(v.opk.alpha_g1), v.opk.beta_g2))


@functools.lru_cache(maxsize=None)
def ml_inputs(inputs):
    v = golden_verifier()
    pi = v.opk.gamma_abc_g1[0]
    for x, g in zip(inputs, v.opk.gamma_abc_g1[1:]):
        pi = O.g1_add(pi, O.g1_mul(g, x))
    return tuple(O.miller_loop(pi, O.g2_neg(v.opk.gamma_g2)))


@functools.lru_cache(maxsize=None)
def oracle_v(A, B, C, inputs):
    """V = (ML(A, B) ML(PI, -gamma) ML(C, -delta) ML(-alpha, beta))^((q^12 - 1) / r): one for a valid proof"""
    v = golden_verifier()
    f = O.fq12_mul(O.miller_loop(A, B), list(ml_inputs(inputs)))
    f = O.fq12_mul(f, O.miller_loop(C, O.g2_neg(v.opk.delta_g2)))
    return tuple(O.fq12_pow(O.fq12_mul(f, list(ml_alpha_beta())), O.FINAL_EXP))


def oracle_folded(proofs, inputs, coeffs):
    acc = O.FQ12_ONE
    for (A, B, Cc), x, r in zip(proofs, inputs, coeffs):
        acc = O.fq12_mul(acc, O.fq12_pow(list(oracle_v(A, B, Cc, tuple(x))), r))
    return O.fq12_pow(acc, api.gt_exponent_multiple())


def test_all_valid_batches_fold_to_one():
    proofs, inputs = six()
    for coeffs in (seeded_coeffs(), ENDS + [seeded_coeffs()[0]], [2 ** 128 - 1] * N_PROOFS):
        ok, folded = run(proofs, inputs, coeffs)
        assert ok is True and api.gt_is_one(folded), coeffs
    ok, folded = run(proofs[:1], inputs[:1], [2 ** 64])       # a batch of one
    assert ok is True and api.gt_is_one(folded)


def test_swapped_c_fails_with_the_oracles_folded_value():
    proofs, inputs = six()
    spoiled = list(proofs)
    spoiled[0] = (proofs[0][0], proofs[0][1], proofs[1][2])
    coeffs = seeded_coeffs()
    ok, folded = run(spoiled, inputs, coeffs)
    assert ok is False and not api.gt_is_one(folded)
    want = oracle_folded(spoiled, inputs, coeffs)
    assert want != O.FQ12_ONE
    assert api.gt_to_w_basis(folded) == want
    # the valid proofs contribute one whatever their coefficients are: the oracle's V_i says so itself
    assert all(oracle_v(*p, tuple(x)) == tuple(O.FQ12_ONE) for p, x in zip(proofs[1:3], inputs[1:3]))


def test_coefficients_are_applied_per_proof():
    """C_0 + D and C_1 - D for a subgroup point D cancel under equal coefficients (why the coefficients must be unpredictable) and
    under no others; a zero coefficient drops its proof."""
    proofs, inputs = six()
    D = O.g1_mul(O.G1_GEN, 0x5EED)
    p0 = (proofs[0][0], proofs[0][1], O.g1_add(proofs[0][2], D))
    p1 = (proofs[1][0], proofs[1][1], O.g1_add(proofs[1][2], O.g1_neg(D)))
    ok, folded = run([p0, p1], inputs[:2], [1, 1])
    assert ok is True and api.gt_is_one(folded)
    ok, folded = run([p0, p1], inputs[:2], [1, 2])
    assert ok is False and not api.gt_is_one(folded)
    ok, folded = run([p0, proofs[1]], inputs[:2], [0, 5])
    assert ok is True and api.gt_is_one(folded)
    ok, _ = run([p0, proofs[1]], inputs[:2], [1, 5])
    assert ok is False


def test_wrong_input_and_flipped_sign_fail():
    proofs, inputs = six()
    coeffs = seeded_coeffs()
    wrong = list(inputs)
    wrong[2] = [(x + 1) % O.R_MOD for x in inputs[2]]
    ok, folded = run(proofs, wrong, coeffs)
    assert ok is False and not api.gt_is_one(folded)
    data = [O.proof_serialize(*p) for p in proofs]
    data[3] = flip_sign(data[3], 0)
    ok, folded = run(data, inputs, coeffs)
    assert ok is False and not api.gt_is_one(folded)


def test_non_curve_bytes_are_a_verdict_with_an_all_zero_folded_value():
    proofs, inputs = six()
    data = [O.proof_serialize(*p) for p in proofs]
    x = 5
    while pow((x ** 3 + 1) % O.Q_MOD, (O.Q_MOD - 1) // 2, O.Q_MOD) == 1:
        x += 1
    data[4] = x.to_bytes(48, "little") + data[4][48:]
    ok, folded = run(data, inputs, seeded_coeffs())
    assert ok is False and not folded.any()


def test_cofactor_torsion_is_rejected_where_the_pairing_cannot_see_it():
    v = golden_verifier()
    proofs, inputs = six()
    T = cofactor_torsion_point()
    A, B, Cc = proofs[1]
    for moved in ((O.g1_add(A, T), B, Cc), (A, B, O.g1_add(Cc, T))):
        assert api.groth16_verify_host(inputs_mont=cv.fr_to_mont(inputs[1]), proof=O.proof_serialize(*moved), **v.vk) is True
        batch = [proofs[0], moved, proofs[2]]
        ok, folded = run(batch, inputs[:3], seeded_coeffs(3))
        assert ok is False and not folded.any()


def test_coefficients_from_a_seed():
    a = api.verify_aggregate_coeffs_from_seed(SEED, 64)
    assert a.shape == (64, 2) and a.dtype == np.uint64
    assert (a == api.verify_aggregate_coeffs_from_seed(SEED, 64)).all()
    assert (a[:7] == api.verify_aggregate_coeffs_from_seed(SEED, 7)).all()
    assert (a[:, 0] | a[:, 1]).all()
    b = api.verify_aggregate_coeffs_from_seed(bytes(31) + b"\x01", 64)
    assert not (a == b).all(axis=1).any()
    assert len({(int(lo), int(hi)) for lo, hi in a}) == 64
    assert api.verify_aggregate_coeffs_from_seed(SEED, 0).shape == (0, 2)


def test_err_arg_cases():
    v = golden_verifier()
    proofs, inputs = six()
    lib = _lib.load()
    vk, _abc = api._vk_host(**v.vk)
    data = np.frombuffer(b"".join(O.proof_serialize(*p) for p in proofs[:2]), dtype=np.uint8)
    inp = np.stack([cv.fr_to_mont(x) for x in inputs[:2]])
    co = np.array([[1, 0], [2, 0]], dtype=np.uint64)
    ok, folded = C.c_int(7), np.zeros(72, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(vk_=vk, count=2, inp_=inp, ninp=1, data_=data, co_=co, ok_=ok, folded_=folded):
        return lib.zk_groth16_verify_aggregate_host(C.byref(vk_) if vk_ is not None else None, count, p(inp_), ninp, p(data_), p(co_),
                                                    C.byref(ok_) if ok_ is not None else None, p(folded_))

    assert call() == _lib.ZK_OK and ok.value == 1
    assert call(folded_=None) == _lib.ZK_OK                     # folded is optional
    for bad in (dict(vk_=None), dict(count=0), dict(inp_=None), dict(data_=None), dict(co_=None), dict(ok_=None),
                dict(ninp=2), dict(ninp=0), dict(count=2 ** 22 - 2)):
        assert call(**bad) == ZK_ERR_ARG, bad
    assert call(count=1) == _lib.ZK_OK                          # (the lane limit is count + 3 <= 2^22, not a small count)
    not_below_r = inp.copy()
    not_below_r[1, 0] = 2 ** 64 - 1
    assert call(inp_=not_below_r) == ZK_ERR_ARG
    out = np.zeros((2, 2), dtype=np.uint64)
    assert lib.zk_verify_aggregate_coeffs_from_seed(None, 2, p(out)) == ZK_ERR_ARG
    assert lib.zk_verify_aggregate_coeffs_from_seed(SEED, 2, None) == ZK_ERR_ARG
    with pytest.raises(ValueError):
        api.verify_aggregate_coeffs_from_seed(b"short", 2)
    with pytest.raises(api.ZkError):                             # through the Python form: a wrong input count
        api.groth16_verify_aggregate_host(inputs_mont=np.zeros((2, 2, 4), np.uint64), proofs=bytes(data), coeffs=[1, 1], **v.vk)
