"""Aggregated Marlin verification through the HOST instantiation (zk_marlin_verify_aggregate_host): count proofs of one key as one
folded KZG check with a 128-bit coefficient rho per opening equation (two per proof, at beta and gamma),

    e( sum rho_{k,q} L_{k,q}, h ) . e( sum rho_{k,q} W_{k,q}, -beta_h ) = 1,

and the per-term multiplication of its long sum (csrc/g1_lincomb.cuh: lincomb_term_glv, instantiated for the host by
zk_diag_g1_glv_sum_host) against the oracle's group law.  The folded value of a failing batch is held, coefficient by coefficient in
the w-basis, to the oracle's value computed another way: (prod V_{k,q}^{rho_{k,q}})^ZK_GT_EXPONENT_MULTIPLE with V_{k,q} built from
the arguments with which the oracle's own verifier calls kzg_check."""
import ctypes as C

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from zk_mpc_amd import _lib, api
import marlin_aggregate_cases as AC
import marlin_verify_cases as MC

ZK_ERR_ARG = -2


# ---- the GLV term ------------------------------------------------------------------------------------------------------------------
def test_glv_hook_against_the_oracle_on_the_seams():
    pts, halves, want, total = AC.glv_cases()
    scaled, s = DM.diag_g1_glv_sum(pts, halves)
    got = cv.g1_array_to_affine(scaled)
    bad = [(i, halves[i].tolist()) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, bad
    assert AC.projective_point(s) == total and total is not None
    assert sum(w is None for w in want) >= 3 and len(want) > 100
    # the two pairs that meet in the tree, as sums of two: a doubling, a cancellation
    _, pair = DM.diag_g1_glv_sum(pts[-4:-2], halves[-4:-2], scaled=False)
    assert AC.projective_point(pair) == O.g1_add(want[-4], want[-3])
    _, pair = DM.diag_g1_glv_sum(pts[-2:], halves[-2:], scaled=False)
    assert AC.projective_point(pair) is None


def test_glv_hook_sums_of_random_halves_against_the_oracle():
    pts, halves, _, sums = AC.glv_random()
    for n in AC.SIZES:
        _, s = DM.diag_g1_glv_sum(pts[:n], halves[:n], scaled=False)
        assert AC.projective_point(s) == sums[n], n


def test_glv_hook_refuses():
    pts, halves, _, _ = AC.glv_cases()
    lib = _lib.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    out = np.zeros(18, np.uint64)
    assert lib.zk_diag_g1_glv_sum_host(p(pts), p(halves), 2, None, p(out)) == 0
    assert lib.zk_diag_g1_glv_sum_host(None, p(halves), 2, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_glv_sum_host(p(pts), None, 2, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_glv_sum_host(p(pts), p(halves), 0, None, p(out)) == ZK_ERR_ARG
    assert lib.zk_diag_g1_glv_sum_host(p(pts), p(halves), 2, None, None) == ZK_ERR_ARG
    assert lib.zk_diag_g1_glv_sum_host(p(pts), p(halves), 2 ** 22 + 1, None, p(out)) == ZK_ERR_ARG
    big = pts[:2].copy()
    big[1, 3] = 2 ** 64 - 1
    big[1, 5] = 2 ** 64 - 1                                         # x not below q
    assert lib.zk_diag_g1_glv_sum_host(p(big), p(halves), 2, None, p(out)) == ZK_ERR_ARG


# ---- accepting ---------------------------------------------------------------------------------------------------------------------
def test_golden_proofs_are_accepted_one_by_one_and_rederived():
    doc = AC.golden()
    for inputs, proof in AC.good():
        assert DM.verify_host(AC.vk(), inputs, proof)
    keys = MC.oracle_keys(AC.system())
    assert MC.oracle_verdict(keys, doc["proofs"][2]) == 1           # one entry live: the fixture cannot rot


def test_all_valid_batches_fold_to_one():
    g = AC.good()
    for coeffs in (AC.seeded_coeffs(4), [AC.M128] * 8, [1, 2, 2 ** 64 - 1, 2 ** 64, AC.M128, 1 << 127, 3, 5]):
        ok, folded = AC.agg_host(g, coeffs)
        assert ok is True and api.gt_is_one(folded), coeffs
    for k in range(4):                                              # batches of one
        ok, folded = AC.agg_host(g[k:k + 1], AC.seeded_coeffs(4)[2 * k:2 * k + 2])
        assert ok is True and api.gt_is_one(folded), k
    ok, folded = AC.agg_host(AC.good(1), AC.seeded_coeffs(1), si=1)      # the second system's key and proof
    assert ok is True and api.gt_is_one(folded)


def test_folded_is_optional():
    inputs, proofs = AC.batch(AC.good()[:2])
    count, inp, p_inp, p_buf, p_off, _keep = DM._batch_args(inputs, proofs)
    co = api._coeff_array(AC.seeded_coeffs(2), 4)
    ok = C.c_int(7)
    rc = _lib.load().zk_marlin_verify_aggregate_host(C.byref(AC.vk().struct), count, p_inp, inp.shape[1], p_buf, p_off, co.ctypes.data_as(C.c_void_p),
                                                     C.byref(ok), None)
    assert rc == 0 and ok.value == 1


# ---- rejecting ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", [0, 1])
def test_every_rejected_variant_inside_a_batch_of_three(si):
    g = AC.good(si)
    rejected = [v for v in AC.system(si)["variants"] if v["verdict"] == 0]
    assert {v["name"] for v in rejected} == AC.BEFORE_PAIRING | AC.AT_THE_PAIRING
    coeffs = AC.seeded_coeffs(3)
    got = {}
    for v in rejected:
        ok, folded = AC.agg_host([g[0], MC.variant_args(v)[:2], g[-1]], coeffs, si)
        got[v["name"]] = (ok, bool(folded.any()), api.gt_is_one(folded))
    want = {n: (False, False, False) for n in AC.BEFORE_PAIRING}
    want.update({n: (False, True, False) for n in AC.AT_THE_PAIRING})
    assert got == want
    ok, folded = AC.agg_host([g[0], g[-1], g[0]], coeffs, si)      # the same batch without the variant
    assert ok is True and api.gt_is_one(folded)


def test_coefficients_are_applied_per_equation():
    """wit_gamma_other_point spoils the proof's equation at gamma alone: coefficient 0 THERE (equation 2 k + 1) and the batch is
    accepted, any other value and it is not; 0 on the equation at beta does not help."""
    g = AC.good()
    items = [g[0], AC.variant("wit_gamma_other_point"), g[1]]
    co = AC.seeded_coeffs(3)
    ok, folded = AC.agg_host(items, co[:3] + [0] + co[4:])
    assert ok is True and api.gt_is_one(folded)
    for other in (1, 2 ** 64, co[3]):
        ok, folded = AC.agg_host(items, co[:3] + [other] + co[4:])
        assert ok is False and folded.any() and not api.gt_is_one(folded), other
    ok, _ = AC.agg_host(items, co[:2] + [0] + co[3:])
    assert ok is False
    ok, _ = AC.agg_host(items, co[:2] + [0, 0] + co[4:])            # both zero: the proof is dropped
    assert ok is True


def oracle_v(si, inputs_hex, proof):
    """[V_beta, V_gamma] of one proof: the oracle's verify run with kzg_check patched to record its arguments, and from them
    V = (ML(C - v g - rv gamma_g, h) ML(-w, beta_h - z h))^((q^12 - 1) / r) -- one exactly where kzg_check says True."""
    import marlin_full_ref as MF
    keys = MC.oracle_keys(AC.system(si))
    calls, verdicts = [], []
    real = MF.O.kzg_check

    def record(pp, comm, z, value, w, random_v=None):
        calls.append((comm, z, value, w, random_v))
        verdicts.append(real(pp, comm, z, value, w, random_v))
        return True                                                  # (verify stops at the first failing equation otherwise)
    MF.O.kzg_check = record
    try:
        assert MF.verify(keys, [int(x, 16) for x in inputs_hex], MF.proof_deserialize(proof))
    finally:
        MF.O.kzg_check = real
    assert len(calls) == 2
    verdict = all(verdicts)
    pp, vs = keys.pp, []
    for comm, z, value, w, rv in calls:
        inner = O.g1_add(comm, O.g1_neg(O.g1_mul(pp.g, value)))
        if rv is not None:
            inner = O.g1_add(inner, O.g1_neg(O.g1_mul(pp.gamma_g, rv)))
        f = O.fq12_mul(O.miller_loop(inner, pp.h), O.miller_loop(O.g1_neg(w), O.g2_add(pp.beta_h, O.g2_neg(O.g2_mul(pp.h, z)))))
        vs.append(O.fq12_pow(f, O.FINAL_EXP))
    assert bool(verdict) == all(v == O.FQ12_ONE for v in vs)
    return vs


def test_failing_batch_has_the_oracles_folded_value():
    doc, sysm = AC.golden(), AC.system()
    by_name = {v["name"]: v for v in sysm["variants"]}
    entries = [doc["proofs"][1], by_name["eval_z_b_plus_1"], doc["proofs"][2]]
    items = [(cv.fr_to_mont([int(x, 16) for x in e["inputs"]]), bytes.fromhex(e["proof"])) for e in entries]
    coeffs = AC.seeded_coeffs(3)
    ok, folded = AC.agg_host(items, coeffs)
    assert ok is False and not api.gt_is_one(folded)
    acc = O.FQ12_ONE
    ones = []
    for k, e in enumerate(entries):
        for q, v in enumerate(oracle_v(0, e["inputs"], bytes.fromhex(e["proof"]))):
            ones.append(v == O.FQ12_ONE)
            acc = O.fq12_mul(acc, O.fq12_pow(v, coeffs[2 * k + q]))
    want = O.fq12_pow(acc, api.gt_exponent_multiple())
    assert ones[:2] == [True, True] and ones[4:] == [True, True] and not all(ones[2:4])
    assert want != O.FQ12_ONE
    assert api.gt_to_w_basis(folded) == want


def test_cofactor_torsion_is_rejected_where_the_pairing_cannot_see_it():
    g = AC.good()
    moved = MC.witness_plus_torsion(AC.system())
    ok, folded = AC.agg_host([g[0], moved, g[1]], AC.seeded_coeffs(3))
    assert ok is False and not folded.any()
    ok, folded = AC.agg_host([moved], [0, 0])                       # and whatever the coefficients: the points are tested first
    assert ok is False and not folded.any()


# ---- the call ----------------------------------------------------------------------------------------------------------------------
def test_err_arg_cases():
    sysm = AC.system()
    lib = _lib.load()
    inputs, proofs = AC.batch(AC.good()[:2])
    count, inp, p_inp, p_buf, p_off, keep = DM._batch_args(inputs, proofs)
    co = api._coeff_array(AC.seeded_coeffs(2), 4)
    ok, folded = C.c_int(7), np.zeros(72, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def call(vk_=AC.vk(), count_=2, inp_=p_inp, ninp=1, buf_=p_buf, off_=p_off, co_=p(co), ok_=ok):
        return lib.zk_marlin_verify_aggregate_host(C.byref(vk_.struct) if vk_ is not None else None, count_, inp_, ninp, buf_, off_, co_,
                                                   C.byref(ok_) if ok_ is not None else None, p(folded))
    assert call() == 0 and ok.value == 1
    ok.value = 7
    for bad in (dict(vk_=None), dict(count_=0), dict(inp_=None), dict(buf_=None), dict(off_=None), dict(co_=None), dict(ok_=None),
                dict(count_=2 ** 18 + 1)):
        assert call(**bad) == ZK_ERR_ARG, bad
    down = np.array([951, 0, 951], dtype=np.uint64)                  # decreasing offsets
    assert call(off_=p(down)) == ZK_ERR_ARG
    not_below_r = inp.copy()
    not_below_r[1, 0] = 2 ** 64 - 1
    assert call(inp_=p(not_below_r)) == ZK_ERR_ARG
    # the key: what zk_marlin_verify_host refuses, and a point outside the prime-order subgroup (on the curve, canonical, not infinity)
    k = sysm["key"]
    parts = [bytes.fromhex(k["ivk_bytes"]), MC._g1(k["g"]), MC._g1(k["gamma_g"]), MC._g2(k["h"]), MC._g2(k["beta_h"]), MC._g1(k["shift_h"]), MC._g1(k["shift_k"])]

    def with_part(i, val):
        q = list(parts)
        q[i] = val
        return DM.VerifierKey.from_parts(*q)
    assert call(vk_=with_part(0, parts[0][:-1])) == ZK_ERR_ARG
    assert call(vk_=with_part(5, np.zeros(12, np.uint64))) == ZK_ERR_ARG
    T = cv.g1_affine_to_array([MC.cofactor_torsion_point()])[0]
    for i in (1, 2, 5, 6):
        assert call(vk_=with_part(i, T)) == ZK_ERR_ARG, i
        assert DM.verify_host(with_part(i, T), *AC.good()[0]) in (True, False)      # (zk_marlin_verify_host takes such a key: a verdict)
    tx, ty = MC.cofactor_torsion_point()
    ivk = bytearray(parts[0])
    ivk[24 + 195 * 7:24 + 195 * 7 + 96] = tx.to_bytes(48, "little") + ty.to_bytes(48, "little")      # the index commitment b_row_col
    assert call(vk_=with_part(0, bytes(ivk))) == ZK_ERR_ARG
    assert ok.value == 7                                             # untouched by the refused calls
    with pytest.raises(ValueError):                                  # through the Python form: one coefficient per PROOF is too few
        DM.verify_aggregate_host(AC.vk(), inputs, proofs, [1, 1])
    with pytest.raises(_lib.ZkError):
        DM.verify_aggregate_host(with_part(6, T), inputs, proofs, [1, 1, 1, 1])
