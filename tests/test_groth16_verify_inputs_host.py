"""Groth16 verification through the HOST forms (zk_groth16_verify_host[_checked], zk_groth16_verify_aggregate_host) on keys with
0, 1, 2, 3, 8 and 33 public inputs, with proofs forged from the trapdoor for input vectors placed where the prepared-input sum and
the folded sum degenerate (groth16_verify_cases.py): inputs of 0, 1 and r - 1, a term equal or opposite to the running sum, a
prepared input at infinity, a coefficient sum s_j = 0.  The key is the oracle's (points from O.g1_mul / O.g2_mul); the oracle's own
verifier referees a fixed sample, its pairings being slow in Python."""
import ctypes as C
import functools

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import _lib, api
import groth16_verify_cases as G

ZK_ERR_ARG = -2
SENSITIVITY_NINPS = (1, 2, 3, 8)
# what the oracle's verifier referees: (ninp, vector name, the input to change or None), at most 8
ORACLE_SAMPLE = ((0, "random", None), (1, "cancel@last", None), (3, "dbl@0", None), (3, "cancel@last", None), (3, "cancel@0", 2),
                 (8, "mixed", None), (33, "dbl@last", None), (2, "tops", 0))


def verify(k, x, data, check):
    return api.groth16_verify_host(inputs_mont=G.inputs_mont([x])[0], proof=data, check_subgroup=check, **k.vk)


def aggregate(k, xs, datas, coeffs):
    return api.groth16_verify_aggregate_host(inputs_mont=G.inputs_mont(xs), proofs=list(datas), coeffs=coeffs, **k.vk)


@functools.lru_cache(maxsize=None)
def named(ninp):
    """{name: (x, abc, proof bytes)} of every named vector at this input count"""
    k = G.host_key(ninp + 1)
    rng = O.Prng(0x16A0 + ninp)
    out = {}
    for name in G.vector_names(ninp):
        x = G.vector(name, k.pks, rng)
        abc, _ = G.forge(k.pks, k.td, x, rng)
        out[name] = (x, abc, G.proof_bytes(k.td, abc))
    return out


@pytest.mark.parametrize("ninp", G.NINPS)
def test_every_named_vector_accepts_and_one_changed_input_rejects(ninp):
    k = G.host_key(ninp + 1)
    assert len(G.vector_names(ninp)) == (1 if ninp == 0 else 7 if ninp == 1 else 9)
    # every input position through the unchecked form (the checked one runs the same loop behind its subgroup test); beyond 8
    # inputs the first, the middle and the last position through the other two
    some = range(ninp) if ninp <= 8 else (0, ninp // 2, ninp - 1)
    for name, (x, _, data) in named(ninp).items():
        for check in (False, True):
            assert verify(k, x, data, check) is True, (name, check)
            for j in (some if check else range(ninp)):
                assert verify(k, G.spoil(x, j), data, check) is False, (name, check, j)
        ok, folded = aggregate(k, [x], [data], [G.FOLD_COEFFS[0]])
        assert ok is True and api.gt_is_one(folded), name
        for j in some:
            ok, folded = aggregate(k, [G.spoil(x, j)], [data], [G.FOLD_COEFFS[0]])
            assert ok is False and folded.any() and not api.gt_is_one(folded), (name, j)


def test_no_public_input_rejects_another_proofs_c():
    k = G.host_key(1)
    rng = O.Prng(0x0C0C)
    abc, pi = G.forge(k.pks, k.td, [], rng)
    other, _ = G.forge(k.pks, k.td, [], rng)
    assert pi == k.pks.gamma_abc[0] and other[2] != abc[2]
    good, bad = G.proof_bytes(k.td, abc), G.proof_bytes(k.td, (abc[0], abc[1], other[2]))
    for check in (False, True):
        assert verify(k, [], good, check) is True and verify(k, [], bad, check) is False
    assert aggregate(k, [[], []], [good, G.proof_bytes(k.td, other)], list(G.FOLD_COEFFS))[0] is True
    ok, folded = aggregate(k, [[], []], [good, bad], list(G.FOLD_COEFFS))
    assert ok is False and not api.gt_is_one(folded)


@pytest.mark.parametrize("swap", [False, True], ids=["plus_one", "rows_swapped"])
@pytest.mark.parametrize("ninp", SENSITIVITY_NINPS)
def test_sensitivity_batches(ninp, swap):
    k = G.host_key(ninp + 1)
    rng = O.Prng(0x5E45 + 2 * ninp + swap)
    true, given, spoiled = G.sensitivity(k.pks, rng, swap)
    count = len(true)
    datas = [G.proof_bytes(k.td, G.forge(k.pks, k.td, x, rng)[0]) for x in true]
    want = G.model_verdicts(count, spoiled)
    assert sum(want) == (count - 2 if swap else count // 2)
    for check in (False, True):
        assert [int(verify(k, given[i], datas[i], check)) for i in range(count)] == want
        assert all(verify(k, true[i], datas[i], check) for i in range(count))
    coeffs = [int(lo) | (int(hi) << 64) for lo, hi in api.verify_aggregate_coeffs_from_seed(bytes(range(32)), count)]
    ok, folded = aggregate(k, true, datas, coeffs)
    assert ok is True and api.gt_is_one(folded)
    ok, folded = aggregate(k, given, datas, coeffs)
    assert ok is False and folded.any() and not api.gt_is_one(folded)


@pytest.mark.parametrize("name", G.fold_case_names(3))
def test_folded_only_cases(name):
    k = G.host_key(4)
    rng = O.Prng(0xF01D + sum(name.encode()))
    coeffs, xs = G.fold_case(name, k.pks, rng)
    datas = [G.proof_bytes(k.td, G.forge(k.pks, k.td, x, rng)[0]) for x in xs]
    ok, folded = aggregate(k, xs, datas, coeffs)
    assert ok is True and api.gt_is_one(folded)
    for i in range(len(xs)):
        for j in range(3):
            moved = [list(x) for x in xs]
            moved[i] = G.spoil(xs[i], j)
            ok, folded = aggregate(k, moved, datas, coeffs)
            assert ok is False and folded.any() and not api.gt_is_one(folded), (i, j)


def test_the_oracle_as_referee():
    assert len(ORACLE_SAMPLE) <= 8
    assert {"cancel@last", "dbl@0"} <= {name for _, name, _ in ORACLE_SAMPLE} and any(j is not None for _, _, j in ORACLE_SAMPLE)
    for ninp, name, change in ORACLE_SAMPLE:
        k = G.host_key(ninp + 1)
        x, abc, data = named(ninp)[name]
        given = x if change is None else G.spoil(x, change)
        want = O.verify_proof(k.opk, G.proof_points(k.td, abc), given)
        assert want is (change is None), (ninp, name)
        for check in (False, True):
            assert verify(k, given, data, check) is want, (ninp, name, check)


def test_folded_value_against_the_oracles_product():
    """Three proofs of the three-input key, the second with a changed input: the folded GT value, coefficient by coefficient in the
    w-basis, is (prod_i V_i^{r_i})^3 with V_i the oracle's own left side over right side of proof i."""
    k = G.host_key(4)
    rng = O.Prng(0x0FA1)
    xs = [G.vector(name, k.pks, rng) for name in ("random", "mixed", "dbl@0")]
    abcs = [G.forge(k.pks, k.td, x, rng)[0] for x in xs]
    given = [xs[0], G.spoil(xs[1], 1), xs[2]]
    coeffs = [G.FOLD_COEFFS[0], 2 ** 64 + 5, G.FOLD_COEFFS[1]]
    ok, folded = aggregate(k, given, [G.proof_bytes(k.td, abc) for abc in abcs], coeffs)
    assert ok is False
    ml_ab = O.miller_loop(O.g1_neg(k.opk.alpha_g1), k.opk.beta_g2)
    acc = O.FQ12_ONE
    for x, abc, r in zip(given, abcs, coeffs):
        A, B, Cc = G.proof_points(k.td, abc)
        pi = k.opk.gamma_abc_g1[0]
        for xj, g in zip(x, k.opk.gamma_abc_g1[1:]):
            pi = O.g1_add(pi, O.g1_mul(g, xj))
        f = O.fq12_mul(O.miller_loop(A, B), O.miller_loop(pi, O.g2_neg(k.opk.gamma_g2)))
        f = O.fq12_mul(O.fq12_mul(f, O.miller_loop(Cc, O.g2_neg(k.opk.delta_g2))), ml_ab)
        v = O.fq12_pow(f, O.FINAL_EXP)
        assert (v == O.FQ12_ONE) == (x is not given[1])
        acc = O.fq12_mul(acc, O.fq12_pow(v, r))
    want = O.fq12_pow(acc, api.gt_exponent_multiple())
    assert want != O.FQ12_ONE and api.gt_to_w_basis(folded) == want


def test_refusals():
    k = G.host_key(4)
    x, _, data = named(3)["random"]
    lib = _lib.load()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    buf = np.frombuffer(data, dtype=np.uint8)
    inp = G.inputs_mont([x])
    co = np.array([[1, 0]], dtype=np.uint64)
    ok = C.c_int(7)
    singles = (lib.zk_groth16_verify_host, lib.zk_groth16_verify_host_checked)

    def single(fn, vk, inp_, ninp):
        return fn(C.byref(vk), p(inp_), ninp, p(buf), C.byref(ok))

    def folded(vk, inp_, ninp):
        return lib.zk_groth16_verify_aggregate_host(C.byref(vk), 1, p(inp_), ninp, p(buf), p(co), C.byref(ok), None)

    vk, _abc = api._vk_host(**k.vk)
    for fn in singles:
        assert single(fn, vk, inp, 3) == _lib.ZK_OK and ok.value == 1
    assert folded(vk, inp, 3) == _lib.ZK_OK and ok.value == 1
    # gamma_abc_len is not ninp + 1, in both directions; no inputs where there are some
    for ninp in (2, 4):
        assert [single(fn, vk, inp, ninp) for fn in singles] == [ZK_ERR_ARG] * 2 and folded(vk, inp, ninp) == ZK_ERR_ARG
    for length in (3, 5):
        short, _abc2 = api._vk_host(**dict(k.vk, gamma_abc_g1=np.concatenate([k.vk["gamma_abc_g1"]] * 2)[:length]))
        assert [single(fn, short, inp, 3) for fn in singles] == [ZK_ERR_ARG] * 2 and folded(short, inp, 3) == ZK_ERR_ARG
    assert [single(fn, vk, None, 3) for fn in singles] == [ZK_ERR_ARG] * 2 and folded(vk, None, 3) == ZK_ERR_ARG
    # an input whose words are r, at every position
    for j in range(3):
        at_r = inp.copy()
        at_r[0, j] = cv.fr_raw([O.R_MOD])[0]
        assert [single(fn, vk, at_r, 3) for fn in singles] == [ZK_ERR_ARG] * 2 and folded(vk, at_r, 3) == ZK_ERR_ARG
        with pytest.raises(api.ZkError):
            api.groth16_verify_host(inputs_mont=at_r[0], proof=data, **k.vk)
        with pytest.raises(api.ZkError):
            api.groth16_verify_aggregate_host(inputs_mont=at_r, proofs=data, coeffs=[1], **k.vk)
    below = inp.copy()
    below[0, 1] = cv.fr_raw([O.R_MOD - 1])[0]          # (the words r - 1 are a field element: a verdict)
    assert single(singles[0], vk, below, 3) == _lib.ZK_OK and ok.value == 0
    # no public input: inputs = NULL is legal
    k0 = G.host_key(1)
    _, _, data0 = named(0)["random"]
    buf = np.frombuffer(data0, dtype=np.uint8)
    vk0, _abc0 = api._vk_host(**k0.vk)
    for fn in singles:
        ok.value = 7
        assert single(fn, vk0, None, 0) == _lib.ZK_OK and ok.value == 1
    ok.value = 7
    assert folded(vk0, None, 0) == _lib.ZK_OK and ok.value == 1
    assert single(singles[0], vk0, inp, 1) == ZK_ERR_ARG
