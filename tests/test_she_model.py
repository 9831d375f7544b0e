"""The references of she_cases.py, held against the oracle, against each other and against closed forms; and would the exact
SHE tests (test_gpu_she_exact.py) notice a wrong kernel?  No broken library is built or run: three single-line defects are planted
in the references and the operand families the device tests use have to show them.  Runs without a GPU."""
import random

import numpy as np
import pytest

import she_cases as SC
import zkref as O
import zk_mpc_amd.convert as cv


@pytest.mark.parametrize("n", [4, 8, 64, 256])
def test_products_equal_the_oracle(n):
    for name in ("random", "all_q-1"):
        a, b = SC.family(name, n, 1), SC.family(name, n, 2)
        want = O.encodedtext_mul(a, b)
        assert SC.kron_mul(a, b) == want, name
        assert SC.ntt_mul(a, b) == want, name
        assert SC.ring_mul(a, b) == want, name


@pytest.mark.parametrize("n", [1024, 2048, 4096])
def test_kronecker_equals_transform(n):
    for name in ("random", "all_q-1"):
        a, b = SC.family(name, n, 1), SC.family(name, n, 2)
        assert SC.kron_mul(a, b) == SC.ntt_mul(a, b), name


def test_ring_mul_off_the_transform_path():
    for n in (1, 2, 3, 100):
        a, b = SC.family("random", n, 1), SC.family("random", n, 2)
        assert SC.ring_mul(a, b) == O.encodedtext_mul(a, b)


@pytest.mark.parametrize("log_n", range(2, 15))
def test_closed_forms(log_n):
    """all (q - 1) squared is 2k + 2 - N; X^k a is the signed rotation.  Through the reference the device is compared with at
    that size, so above 4096 this is the only check of ntt_mul that no transform takes part in."""
    n = 1 << log_n
    top = SC.family("all_q-1", n)
    assert SC.ring_mul(top, top) == SC.all_top_squared(n)
    a = SC.family("random", n, 2)
    for d in SC.DELTAS if n <= 1024 else ("delta_1", "delta_last"):
        assert SC.ring_mul(SC.family(d, n), a) == SC.delta_times(SC.delta_index(d, n), a), d


def test_residue_top_is_the_largest_word_pattern():
    w = SC.words([SC.RESIDUE_TOP])
    assert SC.stored_ints(w) == [SC.Q - 1]
    assert SC.all_below_q(w) and not SC.all_below_q(w + np.uint64(1))          # 1 added to every word: above q
    assert cv.fq753_from_mont(w) == [SC.RESIDUE_TOP]


@pytest.mark.parametrize("n", [1, 2, 8, 32])
def test_encode_decode_equal_the_oracle(n):
    rng = random.Random(n)
    for vals in (SC.uniform_r(rng, n), [SC.R - 1] * n):
        assert SC.encode_fast(vals) == O.plaintexts_encode(vals)
    for coeffs in (SC.uniform_q(rng, n), [SC.LIFT_ENDS[(i + n) % len(SC.LIFT_ENDS)] for i in range(n)], SC.encode_fast(SC.uniform_r(rng, n))):
        assert SC.decode_fast(coeffs) == O.encodedtext_decode(coeffs)


def test_centred_lift_ends():
    assert [SC.centred_lift(c) for c in (0, SC.Q // 2, SC.Q // 2 + 1, SC.Q - 1)] == \
        [0, (SC.Q // 2) % SC.R, (SC.Q // 2 + 1 - SC.Q) % SC.R, SC.R - 1]


@pytest.mark.parametrize("n", [1024, 16384])
def test_encode_decode_round_trip(n):
    v = SC.uniform_r(random.Random(n), n)
    enc = SC.encode_fast(v)
    assert max(enc) < SC.R
    assert SC.decode_fast(enc) == v


def _ciphertext_inputs(n, seed):
    rng = random.Random(seed)
    sk = [rng.randrange(11) for _ in range(n)]
    pk_a, pk_b = SC.uniform_q(rng, n), SC.uniform_q(rng, n)
    return rng, sk, pk_a, pk_b


@pytest.mark.parametrize("n", [3, 8, 64])
def test_ciphertext_references_equal_the_oracle(n):
    """Both forms: the restatement over ring_mul, and the one that shares forward transforms (the same at N = 3)."""
    rng, sk, pk_a, pk_b = _ciphertext_inputs(n, 40 + n)
    e, r = [SC.uniform_q(rng, n) for _ in range(2)], [SC.uniform_q(rng, 3 * n) for _ in range(2)]
    for mul in (None, SC.ring_mul):
        cts = [SC.ct_encrypt(e[i], pk_a, pk_b, r[i], mul=mul) for i in range(2)]
        assert cts == [O.ciphertext_encrypt_from(e[i], pk_a, pk_b, r[i]) for i in range(2)]
        prod = SC.ct_mul(cts[0], cts[1], mul=mul)
        assert prod == O.ciphertext_mul(cts[0], cts[1])
        for ct in (cts[0], prod):
            assert SC.ct_decrypt(ct, sk, mul=mul) == O.ciphertext_decrypt(ct, sk)


def test_ciphertext_references_agree_at_a_tile():
    """At N = 1024 ring_mul is Kronecker substitution: the transform-sharing form against a product with no root of unity."""
    n = 1024
    rng, sk, pk_a, pk_b = _ciphertext_inputs(n, 41)
    e, r = SC.uniform_q(rng, n), SC.uniform_q(rng, 3 * n)
    ct = SC.ct_encrypt(e, pk_a, pk_b, r)
    assert ct == SC.ct_encrypt(e, pk_a, pk_b, r, mul=SC.ring_mul)
    top = ([SC.Q - 1] * n,) * 3
    for x, y in ((ct, top), (top, top)):
        prod = SC.ct_mul(x, y)
        assert prod == SC.ct_mul(x, y, mul=SC.ring_mul)
    assert SC.ct_decrypt(prod, sk) == SC.ct_decrypt(prod, sk, mul=SC.ring_mul)


# ---- would the device tests notice? -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [8, 2048, 8192])
def test_twiddle_defect_shows_in_every_product_case(n):
    """One wrong twiddle index at the top level of the forward transform changes the product of every pair that
    test_gpu_she_exact.py multiplies at this size.  The transform of a delta at an even index does not change (its odd half is
    zero, and a wrong factor of zero shows nothing), which is why the deltas run against a dense operand: that one's transform
    is wrong, and so is the product."""
    for case in SC.product_cases(n):
        a, b = SC.case_operands(case, n)
        assert SC.ntt_mul(a, b, "twiddle") != SC.ntt_mul(a, b), case
    # the blindness the note above speaks of, for one operand alone
    d = SC.family("delta_0", n)
    assert SC.forward(d, defect="twiddle") == SC.forward(d)


@pytest.mark.parametrize("n", [8, 2048])
def test_dropped_negation_shows_in_every_ciphertext_case(n):
    """c2 = x1 y1 without its sign: seen wherever x1 y1 is not zero, so by random ciphertexts and by all-(q - 1) ones alike; a
    ciphertext with c1 = 0 would be blind, and none of the device cases has one."""
    rng = random.Random(n)
    rand = [tuple(SC.uniform_q(rng, n) for _ in range(3)) for _ in range(2)]
    top = ([SC.Q - 1] * n,) * 3
    for x, y in ((rand[0], rand[1]), (top, top)):
        good, bad = SC.ct_mul(x, y), SC.ct_mul(x, y, defect="c2_sign")
        assert good[:2] == bad[:2] and good[2] != bad[2]
    zero_c1 = (rand[0][0], [0] * n, rand[0][2])
    assert SC.ct_mul(zero_c1, rand[1]) == SC.ct_mul(zero_c1, rand[1], defect="c2_sign")


def test_wrong_row_shows_with_distinct_rows_only():
    """A row index taken modulo the wrong length: seen when every row holds another polynomial (the batch cases) and in the
    grid-stride layout (row r holds polynomial r mod 3 and 1025 rows: the last row would read polynomial 0, not 1); NOT seen
    when all rows are equal, which is why the all-(q - 1) ciphertexts never run without random ones at the same shape."""
    n, batch = 8, 3
    rng = random.Random(5)
    a, b = [SC.uniform_q(rng, n) for _ in range(batch)], [SC.uniform_q(rng, n) for _ in range(batch)]
    good = SC.batch_mul(a, b)
    assert good == [O.encodedtext_mul(x, y) for x, y in zip(a, b)]
    assert SC.batch_mul(a, b, "row") != good
    rows = 1025
    ga, gb = [a[i % 3] for i in range(rows)], [b[i % 3] for i in range(rows)]
    want = [good[i % 3] for i in range(rows)]
    m = rows - 1
    assert [good[(i % m) % 3] for i in range(rows)] != want                      # what batch_mul(ga, gb, "row") gives, by rows
    assert SC.batch_mul(ga[:4] + ga[-1:], gb[:4] + gb[-1:], "row")[-1] != want[-1]
    top = [[SC.Q - 1] * n] * batch
    assert SC.batch_mul(top, top, "row") == SC.batch_mul(top, top)
