"""Shared builders of the tests of Groth16 verification over several keys in one call (test_groth16_verify_keys_host.py,
test_gpu_groth16_verify_keys.py), on top of groth16_verify_cases.py: pure Python plus the oracle.

Four keys with 0, 1, 3 and 3 public inputs.  G.system(ni, nc) seeds its trapdoor from (ni, nc), so the two three-input keys, made
with different nc, have DIFFERENT trapdoors at the same input count: a proof of one is no proof of the other.  A batch is a key
index per proof (key_of, any order), an input vector per proof and a proof forged from its key's trapdoor (G.forge); `spoiled`
proofs are given inputs changed by +1, so they fail and the folded product is not one.

Every single-key reference is computed on the sub-batch of one key: its proofs, inputs and coefficients in the caller's order."""
import functools
from types import SimpleNamespace

import numpy as np

import zkref as O
import zk_mpc_amd.convert as cv
import groth16_verify_cases as G

R = O.R_MOD
KEY_SHAPES = ((1, 5), (2, 5), (4, 5), (4, 6))      # (ni, nc): 0, 1, 3, 3 public inputs
NINPS = tuple(ni - 1 for ni, _ in KEY_SHAPES)
# grouped run lengths per key: boundaries at lanes 63, 64 and 128; one proof each; a listed key without a proof and a segment of 65
RUNS = {"63_1_64_2": (63, 1, 64, 2), "1_1_1_1": (1, 1, 1, 1), "65_0_64_1": (65, 0, 64, 1)}
ORDERS = ("grouped", "interleaved", "reversed")


@functools.lru_cache(maxsize=None)
def host_key(ni, nc):
    """G.host_key for system(ni, nc): the oracle's verifying-key points of that trapdoor, and the same as ABI arrays"""
    s = G.system(ni, nc)
    td = s.td
    g1, g2 = O.g1_mul(O.G1_GEN, td.g1_k), O.g2_mul(O.G2_GEN, td.g2_k)
    opk = SimpleNamespace(alpha_g1=O.g1_mul(g1, td.alpha), beta_g1=O.g1_mul(g1, td.beta), delta_g1=O.g1_mul(g1, td.delta),
                          beta_g2=O.g2_mul(g2, td.beta), gamma_g2=O.g2_mul(g2, td.gamma), delta_g2=O.g2_mul(g2, td.delta),
                          gamma_abc_g1=[O.g1_mul(g1, k) for k in s.pks.gamma_abc])
    vk = dict(alpha_g1=cv.g1_affine_to_array([opk.alpha_g1])[0], beta_g2=cv.g2_affine_to_array([opk.beta_g2])[0],
              gamma_g2=cv.g2_affine_to_array([opk.gamma_g2])[0], delta_g2=cv.g2_affine_to_array([opk.delta_g2])[0],
              gamma_abc_g1=cv.g1_affine_to_array(opk.gamma_abc_g1))
    return SimpleNamespace(r1cs=s.r1cs, td=td, pks=s.pks, ninp=s.ninp, g1=g1, g2=g2, opk=opk, vk=vk)


def four_keys():
    keys = [host_key(ni, nc) for ni, nc in KEY_SHAPES]
    tds = [(k.td.alpha, k.td.beta, k.td.gamma, k.td.delta) for k in keys]
    assert len(set(tds)) == 4 and len({k.td.delta for k in keys}) == 4 and tuple(k.ninp for k in keys) == NINPS
    return keys


def key_order(runs, order):
    """key_of for the multiset `runs` (proofs per key): grouped by key, dealt round-robin (i mod 4 while every key has proofs left),
    or the grouped order reversed"""
    grouped = [k for k, n in enumerate(runs) for _ in range(n)]
    if order == "grouped":
        return grouped
    if order == "reversed":
        return grouped[::-1]
    assert order == "interleaved"
    left, out = list(runs), []
    while any(left):
        for k in range(len(left)):
            if left[k]:
                left[k] -= 1
                out.append(k)
    assert sorted(out) == grouped
    return out


def forge_batch(keys, key_of, rng):
    """-> (xs, abcs): an input vector and the discrete logs of a valid proof for every entry of key_of"""
    xs, abcs = [], []
    for k in key_of:
        x = [rng.fr() for _ in range(keys[k].ninp)]
        xs.append(x)
        abcs.append(G.forge(keys[k].pks, keys[k].td, x, rng)[0])
    return xs, abcs


def spoil_some(keys, key_of, xs, per_key=1, min_keys=2):
    """xs with the first input of `per_key` proofs of every key that has inputs changed by +1 -> (given, the spoiled proofs)"""
    given, hit, seen = [list(x) for x in xs], set(), {}
    for i, k in enumerate(key_of):
        if keys[k].ninp and seen.get(k, 0) < per_key:
            given[i] = G.spoil(xs[i], 0)
            hit.add(i)
            seen[k] = seen.get(k, 0) + 1
    assert len(seen) >= min_keys, "the batch must fail in at least %d keys" % min_keys
    return given, hit


def flat_inputs(xs):
    """the input vectors concatenated in proof order as (n, 4) Montgomery"""
    flat = [v for x in xs for v in x]
    return cv.fr_to_mont(flat).reshape(-1, 4) if flat else np.zeros((0, 4), np.uint64)


def sub_batch(key_of, k):
    """the proofs of key k in the caller's order"""
    return [i for i, kk in enumerate(key_of) if kk == k]


def coeff_rows(coeffs, rows):
    return np.ascontiguousarray(np.asarray(coeffs, dtype=np.uint64).reshape(-1, 2)[rows])


def product_of_single_key(single, gt_mul, keys, key_of, xs, data, coeffs):
    """The definition of `folded`: the product over the used keys of single(k, inputs (n, ninp, 4), proofs (n, 192), coeffs (n, 2)) ->
    (ok, folded) on each key's sub-batch.  -> (all ok, the product)"""
    ok_all, prod = True, None
    for k in range(len(keys)):
        rows = sub_batch(key_of, k)
        if not rows:
            continue
        ok, f = single(k, G.inputs_mont([xs[i] for i in rows]), np.ascontiguousarray(data[rows]), coeff_rows(coeffs, rows))
        ok_all = ok_all and ok
        prod = f if prod is None else gt_mul(prod, f)
    return ok_all, prod


def forge_with_c(pks, td, x, c, rng):
    """-> (a, b, c): a proof that verifies for the inputs x with the GIVEN discrete log c of its C (a random, b solved for)"""
    pi = G.prepared(pks, x)
    rhs = (td.alpha * td.beta + pi * td.gamma + c * td.delta) % R
    assert rhs != 0
    a = G.nonzero(rng)
    b = rhs * G.inv(a) % R
    assert b != 0 and (a * b - td.alpha * td.beta - pi * td.gamma - c * td.delta) % R == 0
    return (a, b, c % R)
