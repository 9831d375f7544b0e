"""CPU: the transform over G1 points through its host twin (zk_diag_g1_ntt_host: the butterfly of csrc/g1_ntt.cuh instantiated over the
host field, a plain loop around it) against the discrete-log identity: the input is k_i G with known k_i, the expected output
(DFT of k over Fr) G with the scalar transform from the oracle's Domain and the points from the oracle's G1 arithmetic."""
import ctypes as C

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import _lib, api
import g1_ntt_cases as NC

ZK_ERR_ARG = -2


def test_the_c_oracles_points_are_the_python_oracles():
    for k in (1, 2, O.R_MOD - 1, NC.scalars("random", 3)[5]):
        assert cv.g1_array_to_affine(NC.points_of([k]))[0] == O.g1_mul(O.G1_GEN, k)
    assert cv.g1_array_to_affine(NC.points_of([0]))[0] is None


@pytest.mark.parametrize("inverse_root", [False, True])
@pytest.mark.parametrize("log_n", [1, 3, 6])
@pytest.mark.parametrize("case", NC.CASES)
def test_host_transform_is_the_scalar_transform_in_the_exponent(case, log_n, inverse_root):
    k = NC.scalars(case, log_n, inverse_root)
    want = NC.transformed(k, inverse_root)
    if case == "zeros":
        assert k[-1] == 0 and k.count(0) >= 1
    if case == "equal":
        assert all(w == 0 for w in want[1:]) and want[0] != 0
    if case == "zero_output":
        assert want[len(k) // 2] == 0 and want[-1] == 0 and sum(w == 0 for w in want) == len({len(k) // 2, len(k) - 1})
    got = api.g1_ntt_host(NC.points_of(k), inverse_root)
    assert np.array_equal(got, NC.points_of(want))


def test_two_vectors_in_one_call_are_two_transforms():
    a, b = NC.scalars("random", 3), NC.scalars("zeros", 3)
    got = api.g1_ntt_host(np.stack([NC.points_of(a), NC.points_of(b)]), True)
    assert got.shape == (2, 8, 12)
    assert np.array_equal(got[0], NC.points_of(NC.transformed(a, True))) and np.array_equal(got[1], NC.points_of(NC.transformed(b, True)))


def test_a_point_outside_the_subgroup_goes_through_the_plain_chain():
    """no endomorphism: with T of order dividing the cofactor, (P + T, P) transforms to (2 P + T, T) by the group law alone"""
    import marlin_verify_cases as MC
    T = MC.cofactor_torsion_point()
    P = O.g1_mul(O.G1_GEN, 77)
    got = cv.g1_array_to_affine(api.g1_ntt_host(cv.g1_affine_to_array([O.g1_add(P, T), P])))
    assert got == [O.g1_add(O.g1_add(P, P), T), T]


def test_the_hook_refuses_what_it_cannot_take():
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pts = NC.points_of(NC.scalars("random", 1))
    out = np.zeros_like(pts)
    assert lib.zk_diag_g1_ntt_host(p(pts), 1, 1, 0, p(out)) == 0
    assert lib.zk_diag_g1_ntt_host(None, 1, 1, 0, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_ntt_host(p(pts), 1, 1, 0, None) == ZK_ERR_ARG
    assert lib.zk_diag_g1_ntt_host(p(pts), 13, 1, 0, p(out)) == ZK_ERR_ARG
    bad = pts.copy()
    bad[1, :6] = np.uint64(0xffffffffffffffff)                       # a coordinate not below q
    assert lib.zk_diag_g1_ntt_host(p(bad), 1, 1, 0, p(out)) == ZK_ERR_ARG
