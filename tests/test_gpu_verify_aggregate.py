"""Aggregated Groth16 verification on the device (csrc/groth16_verify_keys.hip, csrc/groth16_verify.hip, csrc/pairing.hip): the two fold kernels alone against host arithmetic, word
for word; the long pairing product against the host's product of the same pairs; the aggregate against its host instantiation
(which tests/test_verify_aggregate_host.py holds to the oracle)."""
import functools

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import api
from zk_mpc_amd._lib import ZkError
from helpers import mont1
from marlin_verify_cases import lincomb
from pairing_cases import flip_sign, fq12_cases, g1_arr, g2_arr, pairing_cases

pytestmark = pytest.mark.gpu


# ---- k_fq12_fold ------------------------------------------------------------------------------------------------------------------
def fold_sizes():
    span = api._lib.load().zk_diag_fq12_fold_span()
    # 64 span + 1: the second level plus one (16 385 values of 576 bytes with a span of 256: 9.4 MB)
    return sorted({1, 2, 63, 64, 65, 130, span, span + 1, 64 * span + 1})


@functools.lru_cache(maxsize=None)
def fold_reference(skip_zero):
    """The values and the host's running product (zk_gt_mul in a loop) at every size of fold_sizes().  The values are fq12_cases(130),
    a then b, special elements first, repeated to the longest size.  fq12_cases starts with the zero element, so every product
    of the sequence as it stands is zero: the second sequence (skip_zero) leaves the zero elements out, and its products are not."""
    _, _, A, B = fq12_cases(130)
    pool = np.concatenate([A, B])
    if skip_zero:
        pool = pool[pool.any(axis=1)]
    sizes = fold_sizes()
    vals = pool[np.arange(sizes[-1]) % len(pool)]
    want, acc = {}, vals[0]
    for i in range(sizes[-1]):
        if i:
            acc = api.gt_mul(acc, vals[i])
        if i + 1 in sizes:
            want[i + 1] = acc
    return vals, want


@pytest.mark.parametrize("skip_zero", [False, True], ids=["as_listed", "without_zero"])
def test_fq12_fold_against_the_host_product(ctx, skip_zero):
    vals, want = fold_reference(skip_zero)
    for n in fold_sizes():
        got = ctx.diag_fq12_fold(vals[:n])
        assert np.array_equal(got, want[n]), n
        assert got.any() == skip_zero, n
    assert ctx.lib.zk_diag_fq12_fold_dev(ctx.h, None, 1, None) == -2
    assert ctx.lib.zk_diag_fq12_fold_dev(ctx.h, vals.ctypes.data, 0, vals.ctypes.data) == -2


# ---- k_g1_scale_fold --------------------------------------------------------------------------------------------------------------
SCALE_SIZES = [1, 63, 64, 65, 130, 4097]


@functools.lru_cache(maxsize=None)
def scale_cases():
    """4097 lanes over a table of 12 points: infinity at lanes 0, 63, 64; a point and its negative in one wave with one
    coefficient (lanes 5, 9: they cancel); one point twice with one coefficient (lanes 16, 17: the tree's first step doubles);
    coefficients 0, 1, 2^32 (the word seam), 2^128 - 1 at lanes 1 .. 4 and 65 .. 68, seeded 128-bit ones elsewhere.
    -> table (13, 12) with row 12 infinity, index (n,), coeffs (n, 2) uint64, the host's scaled points (n, 12)."""
    rng = O.Prng(0xA66E)
    n = SCALE_SIZES[-1]
    base = [O.g1_mul(O.G1_GEN, rng.fr()) for _ in range(10)]
    table = base + [O.g1_neg(base[3]), O.G1_GEN, None]
    idx = np.array([(i * 7 + i // 64) % 10 for i in range(n)], dtype=np.uint32)
    co = [rng.u64() | (rng.u64() << 64) for _ in range(n)]
    for k in (0, 63, 64):
        idx[k] = 12
    ends = [0, 1, 2 ** 32, 2 ** 128 - 1]
    for k, c in enumerate(ends):
        co[1 + k], co[65 + k] = c, c
        idx[65 + k] = 11
    idx[5], idx[9], co[9] = 3, 10, co[5]
    idx[16], idx[17], co[17] = 7, 7, co[16]
    coeffs = np.array([[c & (2 ** 64 - 1), c >> 64] for c in co], dtype=np.uint64)
    tab = g1_arr(table)
    rc, scaled = lincomb(tab, idx, scalars8(coeffs), np.arange(n + 1, dtype=np.uint32))
    assert rc == 0
    # spot checks of the reference itself against the oracle's group law
    for k in (0, 1, 2, 3, 4, 5, 68, 129):
        assert cv.g1_array_to_affine(scaled[k:k + 1])[0] == (O.g1_mul(table[idx[k]], co[k]) if table[idx[k]] is not None else None), k
    return tab, idx, coeffs, scaled


def scalars8(coeffs):
    """(n, 2) uint64 -> (n, 8) uint32 raw scalars, the high four words zero"""
    k = np.zeros((len(coeffs), 8), dtype=np.uint32)
    k[:, :4] = np.ascontiguousarray(coeffs).view(np.uint32).reshape(-1, 4)
    return k


def host_sum(points):
    """The sum of (n, 12) affine points through zk_diag_g1_lincomb_host: segments of 64 with the scalar one, level after level."""
    pts = np.ascontiguousarray(points)
    while True:
        n = len(pts)
        one = np.zeros((n, 8), dtype=np.uint32)
        one[:, 0] = 1
        off = np.array(list(range(0, n, 64)) + [n], dtype=np.uint32)
        rc, pts = lincomb(pts, np.arange(n, dtype=np.uint32), one, off)
        assert rc == 0
        if len(pts) == 1:
            return pts[0]


def projective_to_affine_words(p18):
    """The hook's sum: Z is one (x | y are the affine words) or zero (infinity: all-zero affine words)."""
    return p18[:12] if p18[12:].any() else np.zeros(12, dtype=np.uint64)


@pytest.mark.parametrize("n", SCALE_SIZES)
def test_g1_scale_sum_against_the_host_lincomb(ctx, n):
    tab, idx, coeffs, scaled = scale_cases()
    got, total = ctx.diag_g1_scale_sum(tab[idx[:n]], coeffs[:n])
    assert np.array_equal(got, scaled[:n])
    assert np.array_equal(projective_to_affine_words(total), host_sum(scaled[:n]))
    if n == 130:
        assert not got[0].any() and not got[63].any() and not got[64].any() and not got[1].any() and not got[65].any()
        assert np.array_equal(got[66], tab[11]) and got[5].any()
        # the cancelling pair and the doubling pair as sums of two
        _, pair = ctx.diag_g1_scale_sum(np.stack([tab[3], tab[10]]), np.stack([coeffs[5], coeffs[5]]), scaled=False)
        assert not pair[12:].any()
        _, pair = ctx.diag_g1_scale_sum(np.stack([tab[7], tab[7]]), np.stack([coeffs[16], coeffs[16]]), scaled=False)
        assert np.array_equal(projective_to_affine_words(pair), host_sum(np.stack([scaled[16], scaled[16]])))
        # the plain sum (no coefficients) of the same lanes
        _, plain = ctx.diag_g1_scale_sum(tab[idx[:n]], None, scaled=False)
        assert np.array_equal(projective_to_affine_words(plain), host_sum(tab[idx[:n]]))


# ---- zk_pairing_product_long ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points():
    """The recipe of test_gpu_pairing.py: 195 seeded pairs, P or Q at infinity at lanes 0, 63 and 64; the first are pairing_cases()."""
    rng = O.Prng(0xBEEF)
    n = 195
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


@pytest.mark.parametrize("n", [1, 64, 65, 195])
def test_pairing_product_long(ctx, n):
    p, q = points()
    got = ctx.pairing_product_long(p[:n], q[:n])
    assert np.array_equal(got, api.pairing_products_host(p[:n], q[:n], pairs=n)[0])
    assert api.gt_is_one(got) == (n == 1)
    if n == 1:
        assert ctx.lib.zk_pairing_product_long(ctx.h, p.ctypes.data, q.ctypes.data, 0, got.ctypes.data) == -2
        assert ctx.lib.zk_pairing_product_long(ctx.h, None, q.ctypes.data, 1, got.ctypes.data) == -2


# ---- the aggregate ------------------------------------------------------------------------------------------------------------------
SEED = bytes(range(7, 39))


@pytest.fixture(scope="module")
def d8_batch(ctx):
    """The batch of test_gpu_pairing.py: a D = 8 mul-chain key and 130 proofs of it from zk_groth16_prove_batch; and its spoiled set
    (a wrong input at 0, C swapped at 63, A's sign at 64, bytes off the curve at 129)."""
    rng = O.Prng(0x7E57)
    n, count = 5, 130
    dr = ctx.r1cs_mul_chain(n)
    pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])
    m = n + 3
    host = np.concatenate([ctx.download(ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr())), (m, 4)) for _ in range(count)])
    rl, sl = [mont1(rng.fr()) for _ in range(count)], [mont1(rng.fr()) for _ in range(count)]
    proofs = ctx.create_proofs_batch(pk, dr, host, rl, sl)
    inputs = host.reshape(count, m, 4)[:, 1:2, :].copy()
    spoiled, inp = list(proofs), inputs.copy()
    inp[0, 0] = mont1((cv.fr_from_mont(inp[0])[0] + 1) % O.R_MOD)
    spoiled[63] = proofs[63][:144] + proofs[62][144:]
    spoiled[64] = flip_sign(proofs[64], 0)
    x = 5
    while pow((x ** 3 + 1) % O.Q_MOD, (O.Q_MOD - 1) // 2, O.Q_MOD) == 1:
        x += 1
    spoiled[129] = x.to_bytes(48, "little") + proofs[129][48:]
    return pk, proofs, inputs, spoiled, inp


@pytest.mark.parametrize("count", [1, 61, 62, 130])      # Miller lanes 4, 64, 65, 133
def test_aggregate_against_the_host_aggregate(ctx, d8_batch, count):
    pk, proofs, inputs, spoiled, inp = d8_batch
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, count)
    ok, folded = ctx.groth16_verify_aggregate(pk, inputs[:count], proofs[:count], coeffs=coeffs)
    h_ok, h_folded = pk.verify_aggregate_host(inputs[:count], proofs[:count], coeffs)
    assert ok is True and h_ok is True and api.gt_is_one(folded) and np.array_equal(folded, h_folded)
    ok, folded = ctx.groth16_verify_aggregate(pk, inp[:count], spoiled[:count], coeffs=coeffs)
    h_ok, h_folded = pk.verify_aggregate_host(inp[:count], spoiled[:count], coeffs)
    assert ok is False and h_ok is False and np.array_equal(folded, h_folded)
    assert folded.any() == (count < 130)              # bytes off the curve at 129: rejected before the pairing
    assert not api.gt_is_one(folded)


def test_seeded_aggregate_and_the_verdicts_of_each(ctx, d8_batch):
    pk, proofs, inputs, spoiled, inp = d8_batch
    count = len(proofs)
    ok, each = ctx.groth16_verify_aggregate(pk, inputs, proofs, seed=SEED, each=True)
    assert ok is True and each.tolist() == [1] * count
    assert ctx.groth16_verify_aggregate(pk, inputs, proofs, seed=SEED) is True
    assert ctx.groth16_verify_aggregate(pk, inputs, proofs) is True                 # a seed from the operating system
    ok, each = ctx.groth16_verify_aggregate(pk, inp, spoiled, seed=SEED, each=True)
    assert ok is False and each.tolist() == ctx.groth16_verify_batch(pk, inp, spoiled, check_subgroup=True).tolist()
    assert each.tolist() == [0 if k in (0, 63, 64, 129) else 1 for k in range(count)]
    # the seeded entry is the _coeffs entry fed with coeffs_from_seed
    for n in (62, 129):
        seeded = ctx.groth16_verify_aggregate(pk, inp[:n], spoiled[:n], seed=SEED)
        by_coeffs, _ = ctx.groth16_verify_aggregate(pk, inp[:n], spoiled[:n], coeffs=api.verify_aggregate_coeffs_from_seed(SEED, n))
        assert seeded is False and by_coeffs is False
    # small coefficients given as integers
    assert ctx.groth16_verify_aggregate(pk, inputs[1:3], proofs[1:3], coeffs=[1, 1])[0] is True


def test_aggregate_refuses(ctx, d8_batch):
    pk, proofs, inputs, _, _ = d8_batch
    with pytest.raises(ZkError):                       # a wrong input count
        ctx.groth16_verify_aggregate(pk, np.zeros((130, 2, 4), np.uint64), proofs, seed=SEED)
    ok, data, folded = np.zeros(1, np.int32), np.frombuffer(proofs[0], dtype=np.uint8), np.zeros(72, np.uint64)
    co = np.array([[1, 0]], dtype=np.uint64)
    f = ctx.lib.zk_groth16_verify_aggregate_coeffs
    assert f(ctx.h, pk.h, 1, inputs.ctypes.data, 1, data.ctypes.data, co.ctypes.data, ok.ctypes.data_as(api.C.POINTER(api.C.c_int)), folded.ctypes.data) == 0
    assert ok[0] == 1
    for count, pr, c in ((0, data.ctypes.data, co.ctypes.data), (1, None, co.ctypes.data), (1, data.ctypes.data, None),
                         (2 ** 22 - 2, data.ctypes.data, co.ctypes.data)):
        assert f(ctx.h, pk.h, count, inputs.ctypes.data, 1, pr, c, ok.ctypes.data_as(api.C.POINTER(api.C.c_int)), None) == -2
    g = ctx.lib.zk_groth16_verify_aggregate
    assert g(ctx.h, pk.h, 1, inputs.ctypes.data, 1, data.ctypes.data, None, ok.ctypes.data_as(api.C.POINTER(api.C.c_int)), None) == -2
    # a key from zk_pk_upload has no verifying-key parts
    up = ctx.pk_upload(pk.vk_g1(0), pk.vk_g1(1), pk.vk_g1(2), pk.vk_g2(0), pk.vk_g2(1), pk.download("a_query"), pk.download("b_g1_query"),
                       pk.download("b_g2_query"), pk.download("h_query"), pk.download("l_query"))
    with pytest.raises(ZkError):
        ctx.groth16_verify_aggregate(up, inputs, proofs, seed=SEED)
    up.free()


def test_aggregate_timer_names(ctx, d8_batch):
    """With profiling, one aggregate call over one proof leaves exactly these timers, each counted once: the phases by device events,
    the laps by the host's clock (tools/bench_verify_aggregate.py reads them by name)."""
    pk, proofs, inputs, _, _ = d8_batch
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, 1)
    ctx.set_profiling(True)
    try:
        ctx.timers()
        ok, _ = ctx.groth16_verify_aggregate(pk, inputs[:1], proofs[:1], coeffs=coeffs)
        got = ctx.timers()
    finally:
        ctx.set_profiling(False)
    print(sorted(got.items()))
    assert ok is True
    names = ("k_decompress", "k_subgroup", "k_scale", "k_miller", "k_fold", "host_sums", "wait_scale", "wait_miller", "host_finish")
    assert {k: c for k, (_, c) in got.items()} == {"verify_aggregate." + w: 1 for w in names}
