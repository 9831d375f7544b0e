"""Points of the two curves with the oracle's verdict on subgroup membership, for the subgroup tests (host and device).

The expected flag of every case is the reference's own test, `r P == O` (short_weierstrass_jacobian.rs:146-149), through the
oracle's plain double-and-add: `O.ec_mul_raw(P, R_MOD, ops) is None`.  A point is None (infinity) or an affine pair; G2 coordinates
are pairs (c0, c1).  Nothing here reads the library.
"""
import functools
import random

import numpy as np

import zkref as O
from marlin_verify_cases import cofactor_torsion_point

Q = O.Q_MOD
R = O.R_MOD


def oracle_in_subgroup(P, ops):
    return O.ec_mul_raw(P, R, ops) is None


def fq2_sqrt(a):
    """A square root of a = (a0, a1) in Fq2 = Fq[u]/(u^2 + 5) by the norm method, or None."""
    a0, a1 = a
    if a1 == 0:
        s = O.fq_sqrt(a0)
        if s is not None:
            return (s, 0)
        s = O.fq_sqrt(a0 * pow(Q - 5, -1, Q) % Q)
        return None if s is None else (0, s)
    s = O.fq_sqrt((a0 * a0 + 5 * a1 * a1) % Q)
    if s is None:
        return None
    inv2 = pow(2, -1, Q)
    for sign in (1, -1):
        x0 = O.fq_sqrt((a0 + sign * s) * inv2 % Q)
        if x0 is not None and x0 != 0:
            y = (x0, a1 * pow(2 * x0, -1, Q) % Q)
            if O.fq2_sqr(y) == (a0 % Q, a1 % Q):
                return y
    return None


@functools.lru_cache(maxsize=None)
def g2_coeff_b():
    """b' read off the generator: y^2 - x^3"""
    x, y = O.G2_GEN
    return O.fq2_sub(O.fq2_sqr(y), O.fq2_mul(O.fq2_sqr(x), x))


@functools.lru_cache(maxsize=None)
def g2_outside_point():
    """A point of the twist outside the prime-order subgroup: the first x = (0x5eed + k, 1) with x^3 + b' a square."""
    b = g2_coeff_b()
    k = 0
    while True:
        x = (0x5eed + k, 1)
        y = fq2_sqrt(O.fq2_add(O.fq2_mul(O.fq2_sqr(x), x), b))
        if y is not None:
            P = (x, y)
            assert O.ec_is_on_curve(P, O.Fq2Ops)
            if not oracle_in_subgroup(P, O.Fq2Ops):
                return P
        k += 1


@functools.lru_cache(maxsize=None)
def g2_cofactor_torsion_point():
    """T2 = r P for a twist point P outside the subgroup: on the twist, of order dividing the cofactor, not infinity."""
    T = O.ec_mul_raw(g2_outside_point(), R, O.Fq2Ops)
    assert T is not None
    return T


G1_ORDER2 = (Q - 1, 0)      # (-1)^3 + 1 = 0
G1_ORDER3 = (0, 1)          # 3-torsion: x = 0


@functools.lru_cache(maxsize=None)
def g1_cases():
    """[(point, in_subgroup)]"""
    F = O.FqOps
    T = cofactor_torsion_point()
    rng = random.Random(0x5b6)
    S = [O.ec_mul_raw(O.G1_GEN, k, F) for k in (1, 2, 3, R - 1, rng.randrange(R), rng.randrange(R))]
    pts = list(S) + [None, T, O.ec_add(T, T, F)]
    pts += [O.ec_add(s, T, F) for s in S[:3]]
    assert O.ec_is_on_curve(G1_ORDER2, F) and O.ec_is_on_curve(G1_ORDER3, F)
    pts += [G1_ORDER2, G1_ORDER3, O.ec_add(S[1], G1_ORDER2, F), O.ec_add(S[4], G1_ORDER3, F), O.ec_add(G1_ORDER2, G1_ORDER3, F)]
    for P in pts:
        assert O.ec_is_on_curve(P, F)
    return [(P, oracle_in_subgroup(P, F)) for P in pts]


@functools.lru_cache(maxsize=None)
def g2_cases():
    F = O.Fq2Ops
    T = g2_cofactor_torsion_point()
    rng = random.Random(0x5b7)
    S = [O.ec_mul_raw(O.G2_GEN, k, F) for k in (1, 2, 3, R - 1, rng.randrange(R), rng.randrange(R))]
    pts = list(S) + [None, T, O.ec_add(T, T, F), g2_outside_point()]
    pts += [O.ec_add(s, T, F) for s in S[:3]]
    for P in pts:
        assert O.ec_is_on_curve(P, F)
    return [(P, oracle_in_subgroup(P, F)) for P in pts]


def cases(group):
    out = g1_cases() if group == 1 else g2_cases()
    flags = [f for _, f in out]
    assert any(flags) and not all(flags)
    return out


def table(group, n, seed=0x7ab1e):
    """n cases: the list repeated to length n and shuffled by a fixed seed.  -> ([points], [flags])"""
    cs = cases(group)
    rep = [cs[i % len(cs)] for i in range(n)]
    random.Random(seed + n).shuffle(rep)
    return [p for p, _ in rep], [f for _, f in rep]


# ---- the ABI's forms ----------------------------------------------------------------------------------------------------------------
def _mont_words(v):
    m = O.fq_to_mont(v)
    return [(m >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]


def abi_array(group, pts):
    """(n, 12) / (n, 24) uint64: x | y in the reference's Montgomery words, infinity all zero"""
    w = 12 if group == 1 else 24
    out = np.zeros((len(pts), w), dtype=np.uint64)
    for i, P in enumerate(pts):
        if P is None:
            continue
        coords = [P[0], P[1]] if group == 1 else [P[0][0], P[0][1], P[1][0], P[1][1]]
        out[i] = [l for c in coords for l in _mont_words(c)]
    return out


def serialize(group, pts, compressed):
    if group == 1:
        f = O.g1_serialize if compressed else O.g1_serialize_uncompressed
    else:
        f = O.g2_serialize if compressed else O.g2_serialize_uncompressed
    return b"".join(f(P) for P in pts)
