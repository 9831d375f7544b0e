"""Shared inputs and oracle values of the pairing tests (test_pairing_host.py, test_gpu_pairing.py): computed once per session."""
import functools
from types import SimpleNamespace

import numpy as np

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import api
from helpers import g1_from_json, g2_from_json, golden, ih, r1cs_from_json, trapdoor_from_json


def g1_arr(points):
    return cv.g1_affine_to_array(points)


def g2_arr(points):
    return cv.g2_affine_to_array(points)


@functools.lru_cache(maxsize=None)
def pairing_cases():
    """Four seeded (a, b) with P = a G1, Q = b G2."""
    rng = O.Prng(0x9A1E)
    ab = [(rng.fr(), rng.fr()) for _ in range(4)]
    return [(a, b, O.g1_mul(O.G1_GEN, a), O.g2_mul(O.G2_GEN, b)) for a, b in ab]


@functools.lru_cache(maxsize=None)
def oracle_gt(idx):
    """The oracle's fq12_pow(miller_loop(P, Q), FINAL_EXP) raised to ZK_GT_EXPONENT_MULTIPLE, as 12 coefficients of w^k."""
    _, _, P, Q = pairing_cases()[idx]
    return tuple(O.fq12_pow(O.fq12_pow(O.miller_loop(P, Q), O.FINAL_EXP), api.gt_exponent_multiple()))


@functools.lru_cache(maxsize=None)
def golden_verifier():
    """The D = 8 key and proof of tests/golden/groth16.json with the oracle's view of both."""
    j = golden("groth16.json")["mul_chain_5"]
    pkj = j["pk"]
    opk = SimpleNamespace(alpha_g1=g1_from_json(pkj["alpha_g1"]), beta_g2=g2_from_json(pkj["beta_g2"]), gamma_g2=g2_from_json(pkj["gamma_g2"]),
                          delta_g2=g2_from_json(pkj["delta_g2"]), gamma_abc_g1=[g1_from_json(p) for p in pkj["gamma_abc_g1"]])
    r1cs, td = r1cs_from_json(j), trapdoor_from_json(j["trapdoor"])
    z = [ih(v) for v in j["z"]]
    A, B, C = O.predict_proof(r1cs, O.ProvingKeyScalars(r1cs, td), z, ih(j["r"]), ih(j["s"]))
    assert O.proof_serialize(A, B, C) == bytes.fromhex(j["proof"])
    vk = dict(alpha_g1=g1_arr([opk.alpha_g1])[0], beta_g2=g2_arr([opk.beta_g2])[0], gamma_g2=g2_arr([opk.gamma_g2])[0],
              delta_g2=g2_arr([opk.delta_g2])[0], gamma_abc_g1=g1_arr(opk.gamma_abc_g1))
    return SimpleNamespace(j=j, opk=opk, vk=vk, proof=(A, B, C), inputs=z[1:j["num_instance"]])


def flip_sign(proof: bytes, which: int) -> bytes:
    """The sign flag (bit 7 of the last byte) of A (0), B (1) or C (2) flipped."""
    b = bytearray(proof)
    b[(47, 143, 191)[which]] ^= 0x80
    return bytes(b)


def fq12_cases(n=130, seed=0xF912):
    """n pairs (a, b) of Fq12 elements as (n, 72) uint64 arrays plus their w-basis coefficients: elements of coefficients 0, 1 and
    q - 1 first, seeded random ones after."""
    rng = O.Prng(seed)
    q = O.Q_MOD
    special = [[0] * 12, [1] + [0] * 11, [q - 1] * 12, [1] * 12, [0, 1] + [0] * 10, [q - 1] + [0] * 11, [0] * 11 + [q - 1],
               [(q - 1) if k % 2 else 0 for k in range(12)], [1 if k % 3 else q - 1 for k in range(12)]]
    rnd = lambda: [rng.u64() * rng.u64() * rng.u64() * rng.u64() * rng.u64() * rng.u64() % q for _ in range(12)]
    a = [special[i % len(special)] if i < 2 * len(special) else rnd() for i in range(n)]
    b = [special[(i // len(special) + i) % len(special)] if i < 2 * len(special) else rnd() for i in range(n)]
    return a, b, np.stack([api.gt_from_w_basis(x) for x in a]), np.stack([api.gt_from_w_basis(x) for x in b])
