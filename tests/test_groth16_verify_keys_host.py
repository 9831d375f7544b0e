"""CPU: zk_groth16_verify_aggregate_keys_host, the folded Groth16 check of one batch over several keys on the host
(csrc/groth16_verify_keys.hip), held to its definition: the product, by zk_gt_mul, of zk_groth16_verify_aggregate_host on every
key's sub-batch with that sub-batch's coefficients.  Four keys with 0, 1, 3 and 3 public inputs and distinct trapdoors
(groth16_keys_cases.py), valid and spoiled batches in three orders, one key alone against the single-key call word for word, a key
listed twice, the refusals.  Proof points come from the oracle in Python, so the batches are small."""
import ctypes as C
import functools

import numpy as np
import pytest

import zkref as O
from zk_mpc_amd import _lib, api
import groth16_verify_cases as G
import groth16_keys_cases as K

ZK_ERR_ARG = -2
RUNS = (2, 1, 2, 2)


@functools.lru_cache(maxsize=None)
def batch(order):
    keys = K.four_keys()
    key_of = K.key_order(RUNS, order)
    rng = O.Prng(0x4B59 + len(order))
    xs, abcs = K.forge_batch(keys, key_of, rng)
    data = np.frombuffer(b"".join(G.proof_bytes(keys[k].td, abc) for k, abc in zip(key_of, abcs)), dtype=np.uint8).reshape(-1, 192)
    coeffs = api.verify_aggregate_coeffs_from_seed(bytes(range(32)), len(key_of))
    return keys, key_of, xs, data, coeffs


def several(keys, key_of, xs, data, coeffs):
    return api.groth16_verify_aggregate_keys_host([k.vk for k in keys], key_of, K.flat_inputs(xs), data.tobytes(), coeffs)


def single_host(keys):
    return lambda k, inp, proofs, co: api.groth16_verify_aggregate_host(inputs_mont=inp, proofs=proofs.tobytes(), coeffs=co, **keys[k].vk)


@pytest.mark.parametrize("order", K.ORDERS)
def test_the_value_is_the_product_of_the_single_key_values(order):
    keys, key_of, xs, data, coeffs = batch(order)
    ok, folded = several(keys, key_of, xs, data, coeffs)
    assert ok is True and api.gt_is_one(folded)
    given, hit = K.spoil_some(keys, key_of, xs)
    assert len(hit) == 3                                            # one proof of every key that has inputs
    ok, folded = several(keys, key_of, given, data, coeffs)
    w_ok, want = K.product_of_single_key(single_host(keys), api.gt_mul, keys, key_of, given, data, coeffs)
    assert ok is False and w_ok is False and not api.gt_is_one(want)
    assert api.gt_eq(folded, want) and np.array_equal(folded, want)
    # inputs as one array per proof: the same call
    ok2, folded2 = api.groth16_verify_aggregate_keys_host([k.vk for k in keys], key_of, [G.inputs_mont([x])[0] for x in given], list(data), coeffs)
    assert ok2 is False and np.array_equal(folded2, folded)


def test_the_callers_order_does_not_matter_to_the_value():
    """the same multiset of (key, inputs, proof, coefficient) in another order: the same product"""
    keys, key_of, xs, data, coeffs = batch("grouped")
    given, _ = K.spoil_some(keys, key_of, xs)
    _, folded = several(keys, key_of, given, data, coeffs)
    order = [5, 0, 3, 6, 1, 4, 2]
    _, moved = several(keys, [key_of[i] for i in order], [given[i] for i in order], data[order], coeffs[order])
    assert np.array_equal(folded, moved) and not api.gt_is_one(folded)


def test_one_used_key_is_the_single_key_call_word_for_word():
    keys, key_of, xs, data, coeffs = batch("grouped")
    rows = K.sub_batch(key_of, 2)
    for given in ([xs[i] for i in rows], [G.spoil(xs[rows[0]], 2)] + [xs[i] for i in rows[1:]]):
        want = api.groth16_verify_aggregate_host(inputs_mont=G.inputs_mont(given), proofs=data[rows].tobytes(), coeffs=coeffs[rows], **keys[2].vk)
        for vks, ko in (([keys[2].vk], [0] * len(rows)), ([k.vk for k in keys], [2] * len(rows))):      # alone; beside three unused keys
            got = api.groth16_verify_aggregate_keys_host(vks, ko, K.flat_inputs(given), data[rows].tobytes(), coeffs[rows])
            assert got[0] is want[0] and np.array_equal(got[1], want[1]) and got[1].any()


def test_a_key_listed_twice_is_two_keys():
    keys, key_of, xs, data, coeffs = batch("grouped")
    rows = K.sub_batch(key_of, 3)                                  # two proofs of the last key, one through each entry
    given = [G.spoil(xs[rows[0]], 1), xs[rows[1]]]
    ok, folded = api.groth16_verify_aggregate_keys_host([keys[3].vk, keys[3].vk], [0, 1], K.flat_inputs(given), data[rows].tobytes(), coeffs[rows])
    _, want = api.groth16_verify_aggregate_host(inputs_mont=G.inputs_mont(given), proofs=data[rows].tobytes(), coeffs=coeffs[rows], **keys[3].vk)
    assert ok is False and np.array_equal(folded, want) and not api.gt_is_one(folded)


def test_a_proof_under_another_keys_index_fails():
    keys, key_of, xs, data, coeffs = batch("grouped")
    a, b = K.sub_batch(key_of, 2)[0], K.sub_batch(key_of, 3)[0]    # the two three-input keys
    rows = [a, b]
    args = (K.flat_inputs([xs[a], xs[b]]), data[rows].tobytes(), coeffs[rows])
    assert api.groth16_verify_aggregate_keys_host([k.vk for k in keys], [2, 3], *args)[0] is True
    ok, folded = api.groth16_verify_aggregate_keys_host([k.vk for k in keys], [3, 2], *args)
    assert ok is False and folded.any() and not api.gt_is_one(folded)


def test_a_point_outside_the_subgroup_is_an_early_rejection():
    from marlin_verify_cases import cofactor_torsion_point
    keys, key_of, xs, data, coeffs = batch("grouped")
    moved = data.copy()
    c = O.g1_add(O.g1_deserialize(data[3, 144:192].tobytes()), cofactor_torsion_point())
    moved[3, 144:192] = np.frombuffer(O.g1_serialize(c), dtype=np.uint8)
    ok, folded = several(keys, key_of, xs, moved, coeffs)
    assert ok is False and not folded.any()


def test_refusals_leave_the_outputs_untouched():
    keys, key_of, xs, data, coeffs = batch("grouped")
    lib = _lib.load()
    views = [api._vk_host(**k.vk) for k in keys]
    arr = (_lib.VkHost * 4)(*[v[0] for v in views])
    ko = np.array(key_of, dtype=np.uint32)
    inp = K.flat_inputs(xs)
    buf = np.frombuffer(data.tobytes(), dtype=np.uint8)
    count, n_in = len(key_of), inp.shape[0]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    good = dict(vks=arr, n_keys=4, count=count, key_of=p(ko), inputs=p(inp), inputs_len=n_in, proofs=p(buf), coeffs=p(coeffs))

    def call(**change):
        a = dict(good, **change)
        ok, folded = C.c_int(7), np.full(72, 9, dtype=np.uint64)
        rc = lib.zk_groth16_verify_aggregate_keys_host(a["vks"], a["n_keys"], a["count"], a["key_of"], a["inputs"], a["inputs_len"], a["proofs"],
                                                       a["coeffs"], C.byref(ok), p(folded))
        if rc != 0:
            assert ok.value == 7 and (folded == 9).all(), change
        return rc

    assert call() == 0
    for name in ("vks", "key_of", "inputs", "proofs", "coeffs"):
        assert call(**{name: None}) == ZK_ERR_ARG, name
    assert call(count=0) == ZK_ERR_ARG and call(n_keys=0) == ZK_ERR_ARG
    assert call(n_keys=3) == ZK_ERR_ARG                             # key_of holds a 3
    bad_ko = ko.copy()
    bad_ko[2] = 4
    assert call(key_of=p(bad_ko)) == ZK_ERR_ARG
    assert call(inputs_len=n_in - 1) == ZK_ERR_ARG and call(inputs_len=n_in + 1) == ZK_ERR_ARG
    swapped = ko.copy()
    swapped[0] = 1                                                  # a 0-input proof under a 1-input key: the total changes
    assert call(key_of=p(swapped)) == ZK_ERR_ARG
    big = inp.copy()
    big[n_in - 1] = np.array([2 ** 64 - 1] * 4, dtype=np.uint64)
    assert call(inputs=p(big)) == ZK_ERR_ARG
    assert lib.zk_groth16_verify_aggregate_keys_host(good["vks"], 4, count, good["key_of"], good["inputs"], n_in, good["proofs"], good["coeffs"],
                                                     None, None) == ZK_ERR_ARG
