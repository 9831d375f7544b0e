"""Shared builders of the Groth16 verification tests over keys with 0 .. 33 public inputs (test_groth16_verify_inputs_host.py,
test_gpu_groth16_verify_inputs.py): pure Python plus the oracle.

Proofs are FORGED from the trapdoor.  The oracle gives the discrete log of every key element (O.ProvingKeyScalars: gamma_abc =
g_0 .. g_ninp), so for ANY input vector x a proof that verifies can be written down, no satisfied circuit needed:

    pi = g_0 + sum_j x_j g_{j+1}                 (mod r)
    a, b random;  c = (a b - alpha beta - pi gamma) / delta
    proof = (a G1', b G2', c G1'),   G1' = g1_k G1,  G2' = g2_k G2

"Accept" then holds only if the verifier computed exactly the prepared input pi G1', and the x_j can be placed where its sums
degenerate.  acc_t = g_0 + sum_{j<t} x_j g_{j+1} is the running sum in front of term t; the named vectors are

    random, zeros, ones, tops (all r - 1), mixed (0, 1, r - 1, random in turn)
    dbl@t      x_t = acc_t / g_{t+1}: term t equals the running sum (the doubling branch of the addition)
    cancel@t   x_t = -acc_t / g_{t+1}: the sum is at infinity after term t and goes on from there; for t = last it is pi = 0

and for the folded check with coefficients r_i (s_0 = sum r_i, s_{j+1} = sum_i r_i x_ij; the sum is sum_j s_j g_j from infinity)

    s_zero@j   two proofs, s_{j+1} = 0
    s_equal    s_1 g_1 = s_0 g_0 (the second term doubles the first),  s_cancel: s_1 g_1 = -s_0 g_0
    sum_inf    one proof, coefficient 1, a cancel@last vector: the whole sum is at infinity

Every builder asserts the property it claims in integers."""
import functools
from types import SimpleNamespace

import numpy as np

import zkref as O
import zk_mpc_amd.convert as cv

R = O.R_MOD
NINPS = (0, 1, 2, 3, 8, 33)
FOLD_COEFFS = (0x9E3779B97F4A7C15F39CC0605CEDC835, 0xC2B2AE3D27D4EB4F165667B19E3779F9)      # two fixed 128-bit coefficients


def inv(v):
    return pow(v % R, -1, R)


def nonzero(rng):
    while True:
        v = rng.fr()
        if v:
            return v


@functools.lru_cache(maxsize=None)
def system(ni, nc=5, seed=0x6716):
    """A small random constraint system with ni instance variables (ni - 1 public inputs) and its trapdoor: non-unit coefficients,
    every instance column in A.  -> r1cs, td, pks (the key's discrete logs; every gamma_abc scalar non-zero)."""
    rng = O.Prng(seed + 1000 * ni + nc)
    nw = 3
    nv = ni + nw
    coef = lambda: 2 + rng.fr() % (R - 2)
    a = [[] for _ in range(nc)]
    for j in range(ni):
        a[j % nc].append((coef(), j))
    for i in range(nc):
        a[i].append((coef(), ni + rng.u64() % nw))
    b = []
    for i in range(nc):
        first = rng.u64() % nv
        b.append([(coef(), first)] + ([(coef(), (first + 1) % nv)] if rng.u64() & 1 else []))
    c = [[(coef(), ni + i % nw)] for i in range(nc)]
    r1cs = O.R1CS(ni, nw, a, b, c)
    assert all(any(col == j for row in a for _, col in row) for j in range(ni))
    assert all(k not in (0, 1) for m in (a, b, c) for row in m for k, _ in row)
    td = O.Trapdoor(*[nonzero(rng) for _ in range(7)])
    pks = O.ProvingKeyScalars(r1cs, td)
    assert len(pks.gamma_abc) == ni and all(pks.gamma_abc)
    return SimpleNamespace(r1cs=r1cs, td=td, pks=pks, ninp=ni - 1)


@functools.lru_cache(maxsize=None)
def host_key(ni):
    """system(ni) with the oracle's verifying-key points (O.g1_mul / O.g2_mul on the discrete logs) and the same as ABI arrays."""
    s = system(ni)
    td = s.td
    g1, g2 = O.g1_mul(O.G1_GEN, td.g1_k), O.g2_mul(O.G2_GEN, td.g2_k)
    opk = SimpleNamespace(alpha_g1=O.g1_mul(g1, td.alpha), beta_g1=O.g1_mul(g1, td.beta), delta_g1=O.g1_mul(g1, td.delta),
                          beta_g2=O.g2_mul(g2, td.beta), gamma_g2=O.g2_mul(g2, td.gamma), delta_g2=O.g2_mul(g2, td.delta),
                          gamma_abc_g1=[O.g1_mul(g1, k) for k in s.pks.gamma_abc])
    vk = dict(alpha_g1=cv.g1_affine_to_array([opk.alpha_g1])[0], beta_g2=cv.g2_affine_to_array([opk.beta_g2])[0],
              gamma_g2=cv.g2_affine_to_array([opk.gamma_g2])[0], delta_g2=cv.g2_affine_to_array([opk.delta_g2])[0],
              gamma_abc_g1=cv.g1_affine_to_array(opk.gamma_abc_g1))
    return SimpleNamespace(r1cs=s.r1cs, td=td, pks=s.pks, ninp=s.ninp, g1=g1, g2=g2, opk=opk, vk=vk)


# ---- the prepared input and the forged proof ---------------------------------------------------------------------------------------
def acc(pks, x, t):
    """g_0 + sum_{j<t} x_j g_{j+1}: the running sum in front of term t"""
    g = pks.gamma_abc
    return (g[0] + sum(x[j] * g[j + 1] for j in range(t))) % R


def prepared(pks, x):
    assert len(x) == len(pks.gamma_abc) - 1
    return acc(pks, x, len(x))


def forge(pks, td, x, rng):
    """-> (a, b, c) the discrete logs of a proof that verifies for the inputs x, and pi"""
    pi = prepared(pks, x)
    a, b = nonzero(rng), nonzero(rng)
    c = (a * b - td.alpha * td.beta - pi * td.gamma) * inv(td.delta) % R
    assert (a * b - td.alpha * td.beta - pi * td.gamma - c * td.delta) % R == 0
    return (a, b, c), pi


@functools.lru_cache(maxsize=None)
def _points(g1_k, g2_k, abc):
    g1, g2 = O.g1_mul(O.G1_GEN, g1_k), O.g2_mul(O.G2_GEN, g2_k)
    return O.g1_mul(g1, abc[0]), O.g2_mul(g2, abc[1]), O.g1_mul(g1, abc[2])


def proof_points(td, abc):
    """the oracle's (A, B, C) of the discrete logs abc"""
    return _points(td.g1_k, td.g2_k, tuple(abc))


def proof_bytes(td, abc):
    return O.proof_serialize(*proof_points(td, abc))


def inputs_mont(xs):
    """count input vectors -> (count, ninp, 4) Montgomery"""
    n = len(xs[0])
    assert all(len(x) == n for x in xs)
    flat = [v for x in xs for v in x]
    return (cv.fr_to_mont(flat) if flat else np.zeros((0, 4), np.uint64)).reshape(len(xs), n, 4)


def spoil(x, j):
    """x with input j changed by +1"""
    y = list(x)
    y[j] = (y[j] + 1) % R
    return y


# ---- the input vectors by name ---------------------------------------------------------------------------------------------------
def vector_names(ninp):
    if ninp == 0:
        return ["random"]
    names = ["random", "zeros", "ones", "tops", "mixed", "dbl@0", "cancel@last"]
    if ninp > 1:
        names += ["dbl@last", "cancel@0"]
    return names


def vector(name, pks, rng):
    g = pks.gamma_abc
    n = len(g) - 1
    x = [rng.fr() for _ in range(n)]
    if name == "random":
        return x
    if name in ("zeros", "ones", "tops"):
        return [{"zeros": 0, "ones": 1, "tops": R - 1}[name]] * n
    if name == "mixed":
        return [(0, 1, R - 1, x[j])[j % 4] for j in range(n)]
    kind, at = name.split("@")
    t = n - 1 if at == "last" else int(at)
    assert kind in ("dbl", "cancel") and 0 <= t < n
    before = acc(pks, x, t)
    assert before != 0
    sign = 1 if kind == "dbl" else R - 1
    x[t] = sign * before * inv(g[t + 1]) % R
    if kind == "dbl":
        assert x[t] * g[t + 1] % R == before and acc(pks, x, t + 1) == 2 * before % R
    else:
        assert (x[t] * g[t + 1] + before) % R == 0 and acc(pks, x, t + 1) == 0
        assert t < n - 1 or prepared(pks, x) == 0
        assert t == n - 1 or prepared(pks, x) == sum(x[j] * g[j + 1] for j in range(t + 1, n)) % R
    return x


# ---- the folded check ------------------------------------------------------------------------------------------------------------
def coeff_sums(coeffs, xs):
    """s_0 = sum r_i, s_{j+1} = sum_i r_i x_ij (mod r)"""
    n = len(xs[0])
    return [sum(coeffs) % R] + [sum(r * x[j] for r, x in zip(coeffs, xs)) % R for j in range(n)]


def fold_case_names(ninp):
    return ["s_zero@%d" % j for j in range(ninp)] + ["s_equal", "s_cancel", "sum_inf"]


def fold_case(name, pks, rng):
    """-> (coeffs, xs): the 128-bit coefficients and one input vector per proof of the named case"""
    g = pks.gamma_abc
    n = len(g) - 1
    assert n >= 1
    if name == "sum_inf":
        coeffs, xs = [1], [vector("cancel@last", pks, rng)]
        s = coeff_sums(coeffs, xs)
        assert sum(sj * gj for sj, gj in zip(s, g)) % R == 0
        return coeffs, xs
    coeffs = list(FOLD_COEFFS)
    r1, r2 = coeffs
    xs = [[nonzero(rng) for _ in range(n)] for _ in range(2)]
    if name.startswith("s_zero@"):
        j = int(name[7:])
        xs[1][j] = (R - r1) * xs[0][j] * inv(r2) % R
        s = coeff_sums(coeffs, xs)
        assert s[j + 1] == 0 and all(s[k] for k in range(n + 1) if k != j + 1)
    else:
        sign = {"s_equal": 1, "s_cancel": R - 1}[name]
        want = sign * (r1 + r2) * g[0] * inv(g[1]) % R
        xs[1][0] = (want - r1 * xs[0][0]) * inv(r2) % R
        s = coeff_sums(coeffs, xs)
        assert s[0] and s[1] * g[1] % R == sign * s[0] * g[0] % R
    return coeffs, xs


# ---- batches ---------------------------------------------------------------------------------------------------------------------
def model_verdicts(count, spoiled):
    """The verdicts of a batch from its construction: zero where an entry was spoiled."""
    assert all(0 <= k < count for k in spoiled)
    return [0 if k in spoiled else 1 for k in range(count)]


def sensitivity(pks, rng, swap=False):
    """2 ninp + 2 pairwise distinct input vectors -> (true, given, spoiled): in every odd k input (k // 2) % ninp is changed by +1,
    so that every input position is hit; or (swap) the rows of proofs 0 and 1 change places."""
    n = len(pks.gamma_abc) - 1
    assert n >= 1
    count = 2 * n + 2
    true = [[rng.fr() for _ in range(n)] for _ in range(count)]
    assert len({tuple(x) for x in true}) == count
    given = [list(x) for x in true]
    if swap:
        given[0], given[1] = list(true[1]), list(true[0])
        return true, given, {0, 1}
    hit = set()
    for k in range(1, count, 2):
        j = (k // 2) % n
        given[k] = spoil(true[k], j)
        hit.add(j)
    assert hit == set(range(n))
    return true, given, set(range(1, count, 2))
