"""GPU: aggregated Marlin verification on the device.  The kernel of its long sum alone (csrc/g1_term_fold.hip through
zk_diag_g1_term_sum_dev) in both modes -- FULL against the host instantiation of the same per-term source word for word and the oracle's
sums, GLV against zk_diag_g1_glv_sum_host word for word and the oracle -- and the entry points zk_marlin_verify_aggregate_coeffs /
zk_marlin_verify_aggregate against the host form (zk_marlin_verify_aggregate_host): the verdict, `folded` word for word, what is
rejected before the pairing and at it, the coefficient of every equation, cofactor torsion, the seeded form's per-proof verdicts, and
what the call refuses.  The cases are tests/marlin_aggregate_cases.py as the host form's tests use them."""
import ctypes as C
import functools

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from zk_mpc_amd import _lib, api
import marlin_aggregate_cases as AC
import marlin_verify_cases as MC

pytestmark = pytest.mark.gpu

ZK_ERR_ARG = -2
R = O.R_MOD
FULL_SCALARS = [0, 1, R - 1, R, (1 << 256) - 1, int("7" * 64, 16), int("8" * 64, 16)]


# ---- the kernel of the long sum, FULL mode: 256 raw bits per term ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def full_cases():
    """4097 terms over eight points: (points (n, 12), words (n, 8), the host's per-term points from zk_diag_g1_lincomb_host on one-term
    segments, {size: the oracle's sum of the first `size` terms}).  Lanes 0 .. 6: the seam scalars; 7: infinity as a term; 8, 9: one
    point twice with one scalar (equal points at an even lane and its neighbour: the tree's first step doubles); 10, 11: (P, k) beside
    (P, r - k), which cancel; then random scalars, every third one 256 raw bits, not reduced."""
    rng = O.Prng(0x7e2f)
    n = AC.SIZES[-1]
    base = [O.g1_mul(O.G1_GEN, rng.fr()) for _ in range(8)]
    idx = [(3 * i + i // 64) % 8 for i in range(n)]
    ks = [rng.fr() if i % 3 else (rng.u64() << 192) | (rng.u64() << 128) | (rng.u64() << 64) | rng.u64() for i in range(n)]
    ks[:len(FULL_SCALARS)] = FULL_SCALARS
    k = rng.fr()
    idx[8], idx[9], ks[8], ks[9] = 5, 5, k, k
    idx[10], idx[11], ks[10], ks[11] = 6, 6, k, R - k
    pts = cv.g1_affine_to_array(base)[idx]
    inf = cv.g1_affine_to_array([None])[0]
    pts[7] = inf
    words = np.array([MC.scalar_words(v) for v in ks], dtype=np.uint32)
    rc, host = MC.lincomb(np.concatenate([cv.g1_affine_to_array(base), inf[None]]), np.array([8 if i == 7 else j for i, j in enumerate(idx)], dtype=np.uint32),
                          words, np.arange(n + 1, dtype=np.uint32))
    assert rc == 0
    sums = {}
    for size in AC.SIZES:
        per = [0] * 8
        for i in range(size):
            if i != 7:
                per[idx[i]] = (per[idx[i]] + ks[i]) % R
        acc = None
        for p, s in zip(base, per):
            acc = O.g1_add(acc, O.g1_mul(p, s))
        sums[size] = acc
    return pts, words, host, sums


@pytest.mark.parametrize("n", AC.SIZES)
def test_full_hook_per_term_equals_the_host_and_the_sum_the_oracle(ctx, n):
    pts, words, host, sums = full_cases()
    scaled, s = DM.diag_g1_term_sum(ctx, pts[:n], words[:n], DM.TERM_FULL)
    bad = [i for i in range(n) if not np.array_equal(scaled[i], host[i])]
    assert not bad, bad[:8]
    assert AC.projective_point(s) == sums[n]
    if n >= 12:
        got = cv.g1_array_to_affine(scaled[:12])
        assert got[0] is None and got[3] is None and got[7] is None                      # 0 P, r P, k O
        assert got[8] == got[9] and got[8] is not None and got[10] == O.g1_neg(got[11])
    if n == 1:
        assert sums[n] is None                                                          # a batch whose sum is infinity
    _, s2 = DM.diag_g1_term_sum(ctx, pts[:n], words[:n], DM.TERM_FULL, scaled=False)      # without the affine store: the same sum
    assert np.array_equal(s, s2)


def test_full_hook_equal_and_opposite_neighbours_alone(ctx):
    pts, words, host, _ = full_cases()
    _, pair = DM.diag_g1_term_sum(ctx, pts[8:10], words[8:10], DM.TERM_FULL, scaled=False)
    want = cv.g1_array_to_affine(host[8:9])[0]
    assert AC.projective_point(pair) == O.g1_add(want, want)
    _, pair = DM.diag_g1_term_sum(ctx, pts[10:12], words[10:12], DM.TERM_FULL, scaled=False)
    assert AC.projective_point(pair) is None


# ---- GLV mode: k1 | k2, 128 raw bits each ----------------------------------------------------------------------------------------------
def test_glv_hook_against_the_oracle_on_the_seams(ctx):
    pts, halves, want, total = AC.glv_cases()
    scaled, s = DM.diag_g1_term_sum(ctx, pts, halves, DM.TERM_GLV)
    got = cv.g1_array_to_affine(scaled)
    bad = [(i, halves[i].tolist()) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad[:4]
    assert AC.projective_point(s) == total and total is not None
    _, pair = DM.diag_g1_term_sum(ctx, pts[-4:-2], halves[-4:-2], DM.TERM_GLV, scaled=False)      # a doubling, a cancellation
    assert AC.projective_point(pair) == O.g1_add(want[-4], want[-3])
    _, pair = DM.diag_g1_term_sum(ctx, pts[-2:], halves[-2:], DM.TERM_GLV, scaled=False)
    assert AC.projective_point(pair) is None


@pytest.mark.parametrize("n", AC.SIZES)
def test_glv_hook_random_halves_equal_the_host_hook_and_the_oracle(ctx, n):
    pts, halves, host, sums = AC.glv_random()
    scaled, s = DM.diag_g1_term_sum(ctx, pts[:n], halves[:n], DM.TERM_GLV)
    bad = [i for i in range(n) if not np.array_equal(scaled[i], host[i])]
    assert not bad, bad[:8]
    assert AC.projective_point(s) == sums[n]


def test_hook_refuses(ctx):
    pts, words, _, _ = full_cases()
    lib = ctx.lib
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(18, np.uint64)
    pt, wd = np.ascontiguousarray(pts[:2]), np.ascontiguousarray(words[:2])
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(pt), p(wd), 2, 0, None, p(out)) == 0
    assert lib.zk_diag_g1_term_sum_dev(None, p(pt), p(wd), 2, 0, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, None, p(wd), 2, 0, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(pt), None, 2, 0, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(pt), p(wd), 0, 0, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(pt), p(wd), 2, 0, None, None) == ZK_ERR_ARG
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(pt), p(wd), 2 ** 22 + 1, 0, None, p(out)) == ZK_ERR_ARG
    for mode in (-1, 2, 7):                                                             # a mode that is not built
        assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(pt), p(wd), 2, mode, None, p(out)) == ZK_ERR_ARG
    big = pt.copy()
    big[1, 3] = 2 ** 64 - 1
    big[1, 5] = 2 ** 64 - 1                                                             # x not below q
    assert lib.zk_diag_g1_term_sum_dev(ctx.h, p(big), p(wd), 2, 0, None, p(out)) == ZK_ERR_ARG


# ---- the entry points against the host form --------------------------------------------------------------------------------------------
def agg_dev(ctx, items, coeffs, si=0, folded=True):
    inputs, proofs = AC.batch(items)
    return DM.verify_aggregate_coeffs(ctx, AC.vk(si), inputs, proofs, coeffs, folded=folded)


@pytest.mark.parametrize("count", [1, 4, 33])
def test_valid_batches_fold_to_one_with_the_host_forms_value(ctx, count):
    """68 lanes (count 4) are the first two blocks of the long sum, 66 witnesses (count 33) the first two of the second."""
    inputs, proofs = AC.cycled(count)
    coeffs = AC.seeded_coeffs(count)
    ok, folded = DM.verify_aggregate_coeffs(ctx, AC.vk(), inputs, proofs, coeffs)
    ok_h, folded_h = DM.verify_aggregate_host(AC.vk(), inputs, proofs, coeffs)
    assert ok is True and ok_h is True and api.gt_is_one(folded)
    assert np.array_equal(folded, folded_h)
    ok, none = DM.verify_aggregate_coeffs(ctx, AC.vk(), inputs, proofs, coeffs, folded=False)      # folded = NULL
    assert ok is True and none is None


def test_the_second_systems_key_and_proof(ctx):
    ok, folded = agg_dev(ctx, AC.good(1), AC.seeded_coeffs(1), si=1)
    assert ok is True and api.gt_is_one(folded)


@pytest.mark.parametrize("si", [0, 1])
def test_every_rejected_variant_inside_a_batch_of_three(ctx, si):
    g = AC.good(si)
    rejected = [v for v in AC.system(si)["variants"] if v["verdict"] == 0]
    assert {v["name"] for v in rejected} == AC.BEFORE_PAIRING | AC.AT_THE_PAIRING
    coeffs = AC.seeded_coeffs(3)
    for v in rejected:
        items = [g[0], MC.variant_args(v)[:2], g[-1]]
        ok, folded = agg_dev(ctx, items, coeffs, si)
        assert ok is False, v["name"]
        if v["name"] in AC.BEFORE_PAIRING:
            assert not folded.any(), v["name"]
        else:
            ok_h, folded_h = AC.agg_host(items, coeffs, si)
            assert ok_h is False and folded_h.any() and not api.gt_is_one(folded_h)
            assert np.array_equal(folded, folded_h), v["name"]
    ok, folded = agg_dev(ctx, [g[0], g[-1], g[0]], coeffs, si)      # the same batch without the variant
    assert ok is True and api.gt_is_one(folded)


def test_coefficients_are_applied_per_equation(ctx):
    """wit_gamma_other_point spoils the proof's equation at gamma alone: the batch passes exactly when the coefficient of equation
    2 k + 1 is zero; and the two coefficients of the failing proof swapped give another folded value (each the host form's)."""
    g = AC.good()
    items = [g[0], AC.variant("wit_gamma_other_point"), g[1]]
    co = AC.seeded_coeffs(3)
    ok, folded = agg_dev(ctx, items, co[:3] + [0] + co[4:])
    assert ok is True and api.gt_is_one(folded)
    for other in (1, 2 ** 64, co[3]):
        ok, folded = agg_dev(ctx, items, co[:3] + [other] + co[4:])
        assert ok is False and folded.any() and not api.gt_is_one(folded), other
    ok, _ = agg_dev(ctx, items, co[:2] + [0] + co[3:])              # zero on the equation at beta does not help
    assert ok is False
    ok, _ = agg_dev(ctx, items, co[:2] + [0, 0] + co[4:])           # both zero: the proof is dropped
    assert ok is True
    swapped = co[:2] + [co[3], co[2]] + co[4:]
    ok_a, folded_a = agg_dev(ctx, items, co)
    ok_b, folded_b = agg_dev(ctx, items, swapped)
    assert ok_a is False and ok_b is False and not np.array_equal(folded_a, folded_b)
    assert np.array_equal(folded_a, AC.agg_host(items, co)[1]) and np.array_equal(folded_b, AC.agg_host(items, swapped)[1])


def _key_with(i, val, si=0):
    k = AC.system(si)["key"]
    parts = [bytes.fromhex(k["ivk_bytes"]), MC._g1(k["g"]), MC._g1(k["gamma_g"]), MC._g2(k["h"]), MC._g2(k["beta_h"]), MC._g1(k["shift_h"]), MC._g1(k["shift_k"])]
    parts[i] = val(parts[i]) if callable(val) else val
    return DM.VerifierKey.from_parts(*parts)


def test_cofactor_torsion_is_rejected_where_the_pairing_cannot_see_it(ctx):
    g = AC.good()
    moved = MC.witness_plus_torsion(AC.system())
    ok, folded = agg_dev(ctx, [g[0], moved, g[1]], AC.seeded_coeffs(3))
    assert ok is False and not folded.any()
    ok, folded = agg_dev(ctx, [moved], [0, 0])                      # and whatever the coefficients: the points are tested first
    assert ok is False and not folded.any()
    # a key point outside the prime-order subgroup is what is wrong with the CALL
    T = cv.g1_affine_to_array([MC.cofactor_torsion_point()])[0]
    inputs, proofs = AC.batch(g[:2])
    for i in (1, 2, 5, 6):
        with pytest.raises(_lib.ZkError, match="error -2"):
            DM.verify_aggregate_coeffs(ctx, _key_with(i, T), inputs, proofs, AC.seeded_coeffs(2))


def test_seeded_form_and_its_per_proof_verdicts(ctx):
    g = AC.good()
    inputs, proofs = AC.cycled(5)
    ok, each = DM.verify_aggregate(ctx, AC.vk(), inputs, proofs, AC.SEED)
    assert ok is True and each.tolist() == [1] * 5
    ok, none = DM.verify_aggregate(ctx, AC.vk(), inputs, proofs, AC.SEED, each=False)
    assert ok is True and none is None
    # the seeded form IS the coefficient form under zk_verify_aggregate_coeffs_from_seed(seed, 2 count)
    items = [g[0], AC.variant("eval_z_b_plus_1"), g[1], g[2], MC.witness_plus_torsion(AC.system())]
    inputs, proofs = AC.batch(items)
    ok, each = DM.verify_aggregate(ctx, AC.vk(), inputs, proofs, AC.SEED)
    want = DM.verify_batch(ctx, AC.vk(), inputs, proofs)
    assert ok is False and each.tolist() == want.tolist() == [1, 0, 1, 1, 0]
    items = items[:4]                                               # without the torsion: rejected at the pairing, under the seed's coefficients
    inputs, proofs = AC.batch(items)
    ok, each = DM.verify_aggregate(ctx, AC.vk(), inputs, proofs, AC.SEED)
    assert ok is False and each.tolist() == [1, 0, 1, 1]
    assert agg_dev(ctx, items, AC.seeded_coeffs(4))[0] is False


def test_timer_names(ctx):
    """With profiling, one accepted batch leaves exactly these timers, each counted once (tools/bench_marlin_verify_aggregate.py reads
    them by name): the laps by the host's clock, the k_ phases by device events."""
    inputs, proofs = AC.cycled(2)
    ctx.set_profiling(True)
    try:
        ctx.timers()
        ok, _ = DM.verify_aggregate_coeffs(ctx, AC.vk(), inputs, proofs, AC.seeded_coeffs(2))
        got = ctx.timers()
    finally:
        ctx.set_profiling(False)
    print(sorted(got.items()))
    assert ok is True
    names = ("parse", "decompress", "build", "device", "host_pairing", "k_decompress", "k_subgroup", "k_scale_fold", "k_term_fold")
    assert {k: c for k, (_, c) in got.items()} == {"marlin_verify_agg." + w: 1 for w in names}


def test_err_arg_cases(ctx):
    """Every case the host form's test lists, plus a null context and a null seed; ok_all stays untouched and the context usable."""
    lib = ctx.lib
    inputs, proofs = AC.batch(AC.good()[:2])
    count, inp, p_inp, p_buf, p_off, keep = DM._batch_args(inputs, proofs)
    co = api._coeff_array(AC.seeded_coeffs(2), 4)
    ok, folded = C.c_int(7), np.zeros(72, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(ctx_=ctx.h, vk_=AC.vk(), count_=2, inp_=p_inp, ninp=1, buf_=p_buf, off_=p_off, co_=p(co), ok_=ok):
        return lib.zk_marlin_verify_aggregate_coeffs(ctx_, C.byref(vk_.struct) if vk_ is not None else None, count_, inp_, ninp, buf_, off_, co_,
                                                     C.byref(ok_) if ok_ is not None else None, p(folded))
    assert call() == 0 and ok.value == 1
    ok.value = 7
    for bad in (dict(ctx_=None), dict(vk_=None), dict(count_=0), dict(inp_=None), dict(buf_=None), dict(off_=None), dict(co_=None), dict(ok_=None),
                dict(count_=2 ** 18 + 1)):
        assert call(**bad) == ZK_ERR_ARG, bad
    down = np.array([951, 0, 951], dtype=np.uint64)                  # decreasing offsets
    assert call(off_=p(down)) == ZK_ERR_ARG
    not_below_r = inp.copy()
    not_below_r[1, 0] = 2 ** 64 - 1
    assert call(inp_=p(not_below_r)) == ZK_ERR_ARG
    # the key: what zk_marlin_verify_host refuses, and a point outside the prime-order subgroup (on the curve, canonical, not infinity)
    assert call(vk_=_key_with(0, lambda b: b[:-1])) == ZK_ERR_ARG
    assert call(vk_=_key_with(5, np.zeros(12, np.uint64))) == ZK_ERR_ARG
    T = cv.g1_affine_to_array([MC.cofactor_torsion_point()])[0]
    for i in (1, 2, 5, 6):
        assert call(vk_=_key_with(i, T)) == ZK_ERR_ARG, i
    tx, ty = MC.cofactor_torsion_point()

    def b_row_col_moved(ivk):
        ivk = bytearray(ivk)
        ivk[24 + 195 * 7:24 + 195 * 7 + 96] = tx.to_bytes(48, "little") + ty.to_bytes(48, "little")      # the index commitment b_row_col
        return bytes(ivk)
    assert call(vk_=_key_with(0, b_row_col_moved)) == ZK_ERR_ARG
    assert ok.value == 7                                             # untouched by the refused calls

    # the seeded form: the same, and a null seed
    each = np.full(2, 7, dtype=np.int32)

    def seeded(ctx_=ctx.h, count_=2, seed_=AC.SEED, off_=p_off, ok_=ok):
        return lib.zk_marlin_verify_aggregate(ctx_, C.byref(AC.vk().struct), count_, p_inp, 1, p_buf, off_, seed_, C.byref(ok_) if ok_ is not None else None,
                                              p(each))
    for bad in (dict(ctx_=None), dict(seed_=None), dict(count_=0), dict(count_=2 ** 18 + 1), dict(off_=None), dict(ok_=None)):
        assert seeded(**bad) == ZK_ERR_ARG, bad
    assert ok.value == 7 and each.tolist() == [7, 7]
    assert seeded() == 0 and ok.value == 1 and each.tolist() == [1, 1]
    with pytest.raises(ValueError):                                  # through the Python form: one coefficient per PROOF is too few
        DM.verify_aggregate_coeffs(ctx, AC.vk(), inputs, proofs, [1, 1])
    assert call() == 0 and ok.value == 1                             # the context is as usable as before
