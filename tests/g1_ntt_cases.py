"""Shared by tests/test_g1_ntt_host.py and tests/test_gpu_g1_ntt.py: the inputs of the transform over G1 points (csrc/g1_ntt.hip) as
scalars k_i, so that the expected output is known by the discrete-log identity

    sum_i w^(ij) (k_i G)  =  (sum_i w^(ij) k_i) G

with the scalar transform from the oracle's Domain.  Every case is a list of n scalars; a zero scalar is a point at infinity."""
import functools

import numpy as np

import zkref as O
import zkref_c as OC
import zk_mpc_amd.convert as cv

R = O.R_MOD
CASES = ("random", "zeros", "equal", "unit", "zero_output")


@functools.lru_cache(maxsize=None)
def scalars(case: str, log_n: int, inverse_root: bool = False) -> tuple:
    n = 1 << log_n
    rng = O.Prng(0x617 + 31 * log_n + sum(case.encode()))
    if case == "random":
        k = [rng.fr() for _ in range(n)]
    elif case == "zeros":                            # infinity among the inputs, the last slot included (h_query's D-th point)
        k = [0 if (i % 3 == 1 or i == n - 1) else rng.fr() for i in range(n)]
    elif case == "equal":                            # a + w b with a = b and w = 1, a - w b = O: a doubling and a cancellation at level 0
        k = [rng.fr()] * n
    elif case == "unit":
        k = [1] + [0] * (n - 1)
    elif case == "zero_output":                      # the inverse transform of a vector with zeros: outputs n / 2 and n - 1 are infinity
        y = [rng.fr() for _ in range(n)]
        y[n // 2] = 0
        y[n - 1] = 0
        dom = O.Domain(n)
        k = dom._transform(y, dom.group_gen if inverse_root else dom.group_gen_inv)
        k = [x * dom.size_inv % R for x in k]
        assert not all(x == 0 for x in k)
    else:
        raise KeyError(case)
    return tuple(k)


def transformed(k, inverse_root: bool) -> list:
    dom = O.Domain(len(k))
    assert dom.size == len(k)
    return dom._transform(list(k), dom.group_gen_inv if inverse_root else dom.group_gen)


_GEN = cv.g1_affine_to_array([O.G1_GEN])[0]


@functools.lru_cache(maxsize=None)
def _point(k: int):
    return None if k % R == 0 else cv.g1_projective_to_affine(OC.g1_mul(_GEN, cv.fr_to_mont([k])[0]))


def points_of(k) -> np.ndarray:
    """k_i G as an (n, 12) ABI array, from the C oracle's scalar multiplication"""
    return cv.g1_affine_to_array([_point(x) for x in k])
