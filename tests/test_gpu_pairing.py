"""The pairing kernels (csrc/pairing.hip) and zk_groth16_verify_batch (csrc/groth16_verify_keys.hip) on the device, exact against the host instantiation of the same
templates (which tests/test_pairing_host.py holds to the oracle) and, at a few points, against the oracle itself."""
import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from zk_mpc_amd import api
from zk_mpc_amd._lib import ZkError
from helpers import mont1
from pairing_cases import flip_sign, fq12_cases, g1_arr, g2_arr, oracle_gt, pairing_cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tower_cases():
    a, b, A, B = fq12_cases(130)
    # the cyclotomic squaring is only a squaring on the cyclotomic subgroup: pairing values in the first cases of that op
    _, _, P, Q = pairing_cases()[0]
    g = api.pairing_products_host(g1_arr([P, O.G1_GEN, P]), g2_arr([Q, Q, O.G2_GEN]))
    return a, b, A, B, g


@pytest.mark.parametrize("op", range(8), ids=["mul", "sqr", "sparse", "inverse", "frob1", "frob2", "frob3", "cyclotomic_sqr"])
def test_tower_ops_on_the_device(ctx, tower_cases, op):
    """130 cases (two waves and a tail): coefficients 0, 1, q - 1 and seeded random elements."""
    a, b, A, B, g = tower_cases
    if op == 7:
        A = A.copy()
        A[:3], A[64], A[129] = g, g[0], g[1]
    got = ctx.diag_fq12(op, A, B)
    assert np.array_equal(got, api.diag_fq12_host(op, A, B))
    w = lambda rows: [api.gt_to_w_basis(r) for r in rows]
    if op == 0:
        assert w(got) == [O.fq12_mul(x, y) for x, y in zip(a, b)]
    if op == 1:
        assert w(got) == [O.fq12_mul(x, x) for x in a]
    if op == 7:
        for k in (0, 1, 2, 64, 129):
            x = api.gt_to_w_basis(A[k])
            assert api.gt_to_w_basis(got[k]) == O.fq12_mul(x, x)


@pytest.fixture(scope="module")
def points():
    """130 x 3 seeded pairs, with P or Q at infinity at lanes 0, 63 and 64; the first pairs are pairing_cases()."""
    rng = O.Prng(0xBEEF)
    n = 130 * 3
    g1s = [O.g1_mul(O.G1_GEN, rng.fr()) for _ in range(8)]
    g2s = [O.g2_mul(O.G2_GEN, rng.fr()) for _ in range(8)]
    P = [g1s[i % 8] if i % 5 else O.g1_add(g1s[i % 8], g1s[(i // 8) % 8]) for i in range(n)]
    Q = [g2s[(i * 3) % 8] if i % 7 else O.g2_add(g2s[i % 8], g2s[(i // 8 + 1) % 8]) for i in range(n)]
    for k, (_, _, p, q) in enumerate(pairing_cases()):
        P[1 + k], Q[1 + k] = p, q
    P[0] = None
    Q[63] = None
    P[64], Q[64] = None, None
    return g1_arr(P), g2_arr(Q)


@pytest.fixture(scope="module")
def host_single(points):
    p, q = points
    return api.pairing_products_host(p[:130], q[:130])


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_pairing_products_single(ctx, points, host_single, count):
    p, q = points
    got = ctx.pairing_products(p[:count], q[:count])
    assert np.array_equal(got, host_single[:count])
    assert api.gt_is_one(got[0])
    if count > 64:
        assert api.gt_is_one(got[63]) and api.gt_is_one(got[64])
    if count == 130:
        for k in (0, 1):
            assert tuple(api.gt_to_w_basis(got[1 + k])) == oracle_gt(k)


def test_pairing_products_of_three(ctx, points):
    p, q = points
    got = ctx.pairing_products(p[:195], q[:195], pairs=3)
    assert got.shape == (65, 72)
    assert np.array_equal(got, api.pairing_products_host(p[:195], q[:195], pairs=3))
    with pytest.raises(ValueError):
        ctx.pairing_products(p[:4], q[:4], pairs=3)
    assert ctx.lib.zk_pairing_products(ctx.h, None, None, 1, 1, None) == -2


@pytest.fixture(scope="module")
def d8_batch(ctx):
    """A D = 8 mul-chain key and 130 proofs of it from zk_groth16_prove_batch."""
    rng = O.Prng(0x7E57)
    n, count = 5, 130
    dr = ctx.r1cs_mul_chain(n)
    pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])
    m = n + 3
    host = np.concatenate([ctx.download(ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr())), (m, 4)) for _ in range(count)])
    rl, sl = [mont1(rng.fr()) for _ in range(count)], [mont1(rng.fr()) for _ in range(count)]
    proofs = ctx.create_proofs_batch(pk, dr, host, rl, sl)
    inputs = host.reshape(count, m, 4)[:, 1:2, :].copy()
    return pk, proofs, inputs


def test_groth16_verify_batch(ctx, d8_batch):
    pk, proofs, inputs = d8_batch
    count = len(proofs)
    assert ctx.groth16_verify_batch(pk, inputs, proofs).tolist() == [1] * count
    spoiled, inp = list(proofs), inputs.copy()
    inp[0, 0] = mont1((cv.fr_from_mont(inp[0])[0] + 1) % O.R_MOD)                      # a wrong input
    spoiled[63] = proofs[63][:144] + proofs[62][144:]                                    # C swapped
    spoiled[64] = flip_sign(proofs[64], 0)                                               # the sign bit of A
    x = 5
    while pow((x ** 3 + 1) % O.Q_MOD, (O.Q_MOD - 1) // 2, O.Q_MOD) == 1:
        x += 1
    spoiled[129] = x.to_bytes(48, "little") + proofs[129][48:]                           # bytes that are not on the curve
    want = [0 if k in (0, 63, 64, 129) else 1 for k in range(count)]
    got = ctx.groth16_verify_batch(pk, inp, spoiled)
    assert got.tolist() == want
    # one proof through the device path and through the host arithmetic
    assert ctx.groth16_verify(pk, inputs[5], proofs[5]) and pk.verify_host(inputs[5], proofs[5])
    assert not ctx.groth16_verify(pk, inputs[6], proofs[5]) and not pk.verify_host(inputs[6], proofs[5])
    # a key that went through its serialised form gives the same verdicts
    assert len(S.verifying_key_bytes(ctx, pk)) > 0
    pk2, _, _ = S.proving_key_from_bytes(ctx, S.proving_key_bytes(ctx, pk, compressed=False), compressed=False)
    assert ctx.groth16_verify_batch(pk2, inp, spoiled).tolist() == want
    # a wrong input count, no proofs
    with pytest.raises(ZkError):
        ctx.groth16_verify_batch(pk, np.zeros((count, 2, 4), np.uint64), proofs)
    ok = np.zeros(1, np.int32)
    assert ctx.lib.zk_groth16_verify_batch(ctx.h, pk.h, 0, inputs.ctypes.data, 1, proofs[0], ok.ctypes.data) == -2
    assert ctx.lib.zk_groth16_verify_batch(ctx.h, pk.h, 1, inputs.ctypes.data, 1, None, ok.ctypes.data) == -2
    # a key from zk_pk_upload has no verifying-key parts
    up = ctx.pk_upload(pk.vk_g1(0), pk.vk_g1(1), pk.vk_g1(2), pk.vk_g2(0), pk.vk_g2(1), pk.download("a_query"), pk.download("b_g1_query"),
                       pk.download("b_g2_query"), pk.download("h_query"), pk.download("l_query"))
    with pytest.raises(ZkError):
        ctx.groth16_verify_batch(up, inputs, proofs)
    up.free()
    pk2.free()


def test_kzg_opening_check_as_a_pairing_product(ctx):
    """KZG10::check (kzg10/mod.rs:320-343): e(C - v g, h) e(-w, beta h - z h) = 1, on the commitment and proof of the device."""
    rng = O.Prng(0x4B5A)
    deg = 15
    pp = O.KzgParams(deg, rng.fr(), g_k=rng.fr(), gg_k=rng.fr(), h_k=rng.fr())
    pg = ctx.bases_upload(cv.g1_affine_to_array(pp.powers_of_g), 1)
    coeffs = [rng.fr() for _ in range(deg + 1)]
    dc = ctx.upload(cv.fr_to_mont(coeffs))
    z = rng.fr()
    v = O.poly_evaluate(coeffs, z)
    comm = cv.g1_projective_to_affine(ctx.kzg_commit_dev(pg, dc.ptr, deg + 1))
    w = cv.g1_projective_to_affine(ctx.kzg_open_dev(pg, dc.ptr, deg + 1, mont1(z))[0])
    rhs = O.g2_add(pp.beta_h, O.g2_neg(O.g2_mul(pp.h, z)))
    for value, want in ((v, True), ((v + 1) % O.R_MOD, False)):
        inner = O.g1_add(comm, O.g1_neg(O.g1_mul(pp.g, value)))
        gt = ctx.pairing_products(g1_arr([inner, O.g1_neg(w)]), g2_arr([pp.h, rhs]), pairs=2)[0]
        assert api.gt_is_one(gt) == want
        assert O.kzg_check(pp, comm, z, value, w) == want
    pg.free()
    dc.free()
