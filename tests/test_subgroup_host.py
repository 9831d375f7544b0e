"""Subgroup membership through the HOST instantiation of csrc/subgroup.cuh (zk_g1_in_subgroup_host, zk_g2_in_subgroup_host,
zk_groth16_verify_host_checked): the same template the kernel runs, over 64-bit limbs.  The expected verdict everywhere is the
reference's own test r P == O through the oracle's plain double-and-add (subgroup_cases.py)."""
import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import api
from marlin_verify_cases import cofactor_torsion_point
from pairing_cases import golden_verifier
import subgroup_cases as sc


@pytest.mark.parametrize("group", [1, 2])
def test_host_form_equals_the_oracle_on_every_case(group):
    cs = sc.cases(group)
    got = api.in_subgroup_host(sc.abi_array(group, [p for p, _ in cs]), group)
    assert [int(g) for g in got] == [int(f) for _, f in cs]


@pytest.mark.parametrize("group", [1, 2])
def test_case_arrays_are_the_abi_form_the_package_writes(group):
    pts = [p for p, _ in sc.cases(group)]
    want = cv.g1_affine_to_array(pts) if group == 1 else cv.g2_affine_to_array(pts)
    assert np.array_equal(sc.abi_array(group, pts), want)


@pytest.mark.parametrize("group", [1, 2])
def test_a_word_not_below_q_is_an_argument_error(group):
    arr = sc.abi_array(group, [p for p, _ in sc.cases(group)][:3])
    q_words = [(O.Q_MOD >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]
    for coord in range(arr.shape[1] // 6):
        bad = arr.copy()
        bad[1, 6 * coord:6 * coord + 6] = q_words
        with pytest.raises(api.ZkError):
            api.in_subgroup_host(bad, group)
    assert len(api.in_subgroup_host(arr, group)) == 3


def test_checked_host_verify_rejects_what_the_pairing_cannot_see():
    """A proof whose A (or C) is moved by a point of the cofactor torsion still satisfies the pairing equation -- e(T, Q) = 1 -- so
    zk_groth16_verify_host answers 1; the reference fails it at Proof::deserialize, and so does the checked form."""
    v = golden_verifier()
    A, B, C = v.proof
    inp = cv.fr_to_mont(v.inputs)
    good = O.proof_serialize(A, B, C)
    assert api.groth16_verify_host(inputs_mont=inp, proof=good, **v.vk) is True
    assert api.groth16_verify_host(inputs_mont=inp, proof=good, check_subgroup=True, **v.vk) is True
    T = cofactor_torsion_point()
    for moved in ((O.g1_add(A, T), B, C), (A, B, O.g1_add(C, T))):
        data = O.proof_serialize(*moved)
        assert api.groth16_verify_host(inputs_mont=inp, proof=data, **v.vk) is True
        assert api.groth16_verify_host(inputs_mont=inp, proof=data, check_subgroup=True, **v.vk) is False
    # B moved by a torsion point of the twist: only the checked verdict is pinned (the Miller loop's value on a G2 argument outside
    # the subgroup is nothing the reference defines)
    data = O.proof_serialize(A, O.g2_add(B, sc.g2_cofactor_torsion_point()), C)
    assert api.groth16_verify_host(inputs_mont=inp, proof=data, check_subgroup=True, **v.vk) is False
    # a tampered proof stays rejected in both forms
    wrong = cv.fr_to_mont([(x + 1) % O.R_MOD for x in v.inputs])
    assert api.groth16_verify_host(inputs_mont=wrong, proof=good, **v.vk) is False
    assert api.groth16_verify_host(inputs_mont=wrong, proof=good, check_subgroup=True, **v.vk) is False
