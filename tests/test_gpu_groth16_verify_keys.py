"""Groth16 verification of one batch over SEVERAL keys on the device (csrc/groth16_verify_keys.hip): zk_groth16_vkeys_verify_batch,
zk_groth16_vkeys_verify_aggregate_coeffs and the seeded zk_groth16_vkeys_verify_aggregate.

`folded` is held to its definition word for word: in a batch with spoiled inputs in two keys or more (so that the value is NOT one) it
equals the host form's value, the product of the single-key device values and the product of the single-key host values -- under
both settings of ZK_VFY_KEYS_MUL.  The shapes are the smallest at which the keyed sum can go wrong: grouped run lengths (63, 1, 64, 2)
with boundaries at lanes 63, 64 and 128, one proof per key, a listed key without a proof beside a segment of 65, each grouped,
interleaved and reversed; 70 keys of one proof and one of three (more keys than lanes in a wave); a key with 130 public inputs (the
cut of a key's terms into segments of 64 on the device multiplication path).  Then proofs under the wrong key, a C moved by cofactor
torsion, segment sums at infinity and the doubling branch of the tree, a key listed twice, one key alone, the refusals.  The
single-key entry points are the same code on a one-slot plan, so "one key alone" compares two routes into one implementation; what
holds it to an independent value is the second level of the keyed sum at 4 097 proofs of one key, against the host form on 8 proofs.

Keys and proofs: groth16_keys_cases.py; the points come from the fixed-base calls on the device."""
import contextlib
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest

import zkref as O
from zk_mpc_amd import api
from zk_mpc_amd._lib import ZkError
from marlin_verify_cases import cofactor_torsion_point
import groth16_verify_cases as G
import groth16_keys_cases as K
from test_gpu_groth16_verify_inputs import SEED, device_proofs
from test_gpu_groth16_vkey import BASE, gmul

pytestmark = pytest.mark.gpu

R = O.R_MOD
ZK_ERR_ARG = -2
MUL_MODES = ("host", "dev")
_DEV = {}


@contextlib.contextmanager
def keys_mul(mode):
    old = os.environ.get("ZK_VFY_KEYS_MUL")
    os.environ["ZK_VFY_KEYS_MUL"] = mode
    try:
        yield
    finally:
        if old is None:
            del os.environ["ZK_VFY_KEYS_MUL"]
        else:
            os.environ["ZK_VFY_KEYS_MUL"] = old


def four(ctx):
    """the four keys and their resident verifying keys"""
    if "four" not in _DEV:
        keys = K.four_keys()
        _DEV["four"] = (keys, [ctx.vkey_upload(**k.vk) for k in keys])
    return _DEV["four"]


def device_batch(ctx, keys, key_of, abcs):
    """(count, 192) proof bytes in the caller's order; one fixed-base pass per trapdoor"""
    data = np.zeros((len(key_of), 192), dtype=np.uint8)
    by_td = {}
    for i, k in enumerate(key_of):
        by_td.setdefault((keys[k].td.g1_k, keys[k].td.g2_k), (keys[k].td, []))[1].append(i)
    for td, rows in by_td.values():
        data[rows] = device_proofs(ctx, td, [abcs[i] for i in rows])
    return data


def grouped_batch(ctx, name):
    """the valid batch of K.RUNS[name] in grouped order, built once: the other orders move the same proofs"""
    if name not in _DEV:
        keys, _ = four(ctx)
        key_of = K.key_order(K.RUNS[name], "grouped")
        xs, abcs = K.forge_batch(keys, key_of, O.Prng(0x6B65 + sum(name.encode())))
        _DEV[name] = (key_of, xs, device_batch(ctx, keys, key_of, abcs))
    return _DEV[name]


def single_dev(ctx, vkeys):
    return lambda k, inp, proofs, co: ctx.groth16_verify_aggregate(vkeys[k], inp, proofs.tobytes(), coeffs=co)


def single_host(keys):
    return lambda k, inp, proofs, co: api.groth16_verify_aggregate_host(inputs_mont=inp, proofs=proofs.tobytes(), coeffs=co, **keys[k].vk)


def per_key_verdicts(ctx, keys, vkeys, key_of, xs, data, check):
    """zk_groth16_vkey_verify_batch on every key's sub-batch, scattered back into the caller's order"""
    out = np.full(len(key_of), -1, dtype=np.int32)
    for k in range(len(keys)):
        rows = K.sub_batch(key_of, k)
        if rows:
            out[rows] = ctx.groth16_verify_batch(vkeys[k], G.inputs_mont([xs[i] for i in rows]), data[rows].tobytes(), check_subgroup=check)
    return out.tolist()


def check_batch(ctx, keys, vkeys, key_of, xs, data, host=True, min_keys=2, checks=(False, True)):
    """Every form on one VALID batch and on the same batch with inputs spoiled in at least min_keys keys; -> the spoiled batch's folded
    value"""
    count, blob = len(key_of), data.tobytes()
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, count)
    ones = [1] * count
    for mode in MUL_MODES:
        with keys_mul(mode):
            ok, folded = ctx.verify_keys_aggregate(vkeys, key_of, K.flat_inputs(xs), blob, coeffs=coeffs)
        assert ok is True and api.gt_is_one(folded), mode
    assert ctx.verify_keys_batch(vkeys, key_of, K.flat_inputs(xs), blob).tolist() == ones
    assert ctx.verify_keys_aggregate(vkeys, key_of, K.flat_inputs(xs), blob, seed=SEED, each=True)[1].tolist() == ones

    given, hit = K.spoil_some(keys, key_of, xs, min_keys=min_keys)
    inp, want = K.flat_inputs(given), G.model_verdicts(count, hit)
    h_ok, p_host = K.product_of_single_key(single_host(keys), api.gt_mul, keys, key_of, given, data, coeffs)
    d_ok, p_dev = K.product_of_single_key(single_dev(ctx, vkeys), api.gt_mul, keys, key_of, given, data, coeffs)
    assert h_ok is False and d_ok is False and not api.gt_is_one(p_host) and p_host.any()      # never 1 = 1
    assert api.gt_eq(p_dev, p_host)
    for mode in MUL_MODES:
        with keys_mul(mode):
            ok, folded = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, coeffs=coeffs)
        assert ok is False, mode
        assert api.gt_eq(folded, p_host) and api.gt_eq(folded, p_dev) and np.array_equal(folded, p_host), mode
    if host:
        f_ok, f_host = api.groth16_verify_aggregate_keys_host([k.vk for k in keys], key_of, inp, blob, coeffs)
        assert f_ok is False and api.gt_eq(folded, f_host) and np.array_equal(folded, f_host)
    # verdicts in the caller's order: the construction's, the single-key batch form's, the seeded form's
    for check in checks:
        got = ctx.verify_keys_batch(vkeys, key_of, inp, blob, check_subgroup=check).tolist()
        assert got == want and got == per_key_verdicts(ctx, keys, vkeys, key_of, given, data, check), check
    ok, each = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, seed=SEED, each=True)
    assert ok is False and each.tolist() == want
    assert ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, seed=SEED) is False
    return folded


# ---- 1, 2: the exact value on every shape and order ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(K.RUNS))
def test_the_value_and_the_verdicts_on_every_shape_in_every_order(ctx, name):
    keys, vkeys = four(ctx)
    g_key_of, g_xs, g_data = grouped_batch(ctx, name)
    folded = {}
    for order in K.ORDERS:
        key_of = K.key_order(K.RUNS[name], order)
        # the SAME proofs moved: entry i of this order is the next unused grouped proof of its key
        nxt = {k: iter(K.sub_batch(g_key_of, k)) for k in set(g_key_of)}
        rows = [next(nxt[k]) for k in key_of]
        assert sorted(rows) == list(range(len(g_key_of)))
        folded[order] = check_batch(ctx, keys, vkeys, key_of, [g_xs[i] for i in rows], g_data[rows])
    assert len(folded) == 3 and all(f.any() for f in folded.values())


def test_the_callers_order_does_not_matter_to_the_value(ctx):
    """the same (key, inputs, proof, coefficient) tuples in another order: the same product"""
    keys, vkeys = four(ctx)
    key_of, xs, data = grouped_batch(ctx, "63_1_64_2")
    given, _ = K.spoil_some(keys, key_of, xs)
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, len(key_of))
    _, folded = ctx.verify_keys_aggregate(vkeys, key_of, K.flat_inputs(given), data.tobytes(), coeffs=coeffs)
    order = list(np.random.RandomState(7).permutation(len(key_of)))
    _, moved = ctx.verify_keys_aggregate(vkeys, [key_of[i] for i in order], K.flat_inputs([given[i] for i in order]), data[order].tobytes(),
                                         coeffs=coeffs[order])
    assert np.array_equal(folded, moved) and not api.gt_is_one(folded) and folded.any()


def synthetic_key(ctx, ninp, rng):
    """a key with BASE's alpha .. delta and gamma_abc[j] = k_j G: the host view, the trapdoor and gamma_abc's logs as G.forge reads them"""
    ks = [G.nonzero(rng) for _ in range(ninp + 1)]
    vk = dict(BASE.vk, gamma_abc_g1=gmul(ctx, ks))
    return SimpleNamespace(vk=vk, td=BASE.td, ninp=ninp, pks=SimpleNamespace(gamma_abc=[k * G.inv(BASE.td.g1_k) % R for k in ks]))


def test_more_keys_than_lanes_in_a_wave(ctx):
    """70 synthetic keys with one proof each and one with three, dealt in reverse: 71 segments, 71 x 3 tail lanes"""
    rng = O.Prng(0x71E5)
    keys = [synthetic_key(ctx, j % 3, rng) for j in range(70)] + [synthetic_key(ctx, 2, rng)]
    vkeys = [ctx.vkey_upload(**k.vk) for k in keys]
    key_of = K.key_order([1] * 70 + [3], "reversed")
    xs, abcs = K.forge_batch(keys, key_of, rng)
    check_batch(ctx, keys, vkeys, key_of, xs, device_batch(ctx, keys, key_of, abcs), checks=(True,))      # (71 single-key calls per form)
    for v in vkeys:
        v.free()


def test_a_key_whose_terms_are_cut_into_segments(ctx):
    """a key with 130 public inputs (132 multiplications: segments of 64, 64, 3 and alpha) beside a key without inputs"""
    four_keys, _ = four(ctx)
    rng = O.Prng(0x1300)
    keys = [four_keys[0], synthetic_key(ctx, 130, rng)]
    vkeys = [ctx.vkey_upload(**k.vk) for k in keys]
    key_of = [1, 0, 1, 0, 1]
    xs, abcs = K.forge_batch(keys, key_of, rng)
    check_batch(ctx, keys, vkeys, key_of, xs, device_batch(ctx, keys, key_of, abcs), min_keys=1)      # (one key with inputs)
    for v in vkeys:
        v.free()


# ---- 3: soundness across keys ---------------------------------------------------------------------------------------------------------
def test_a_proof_under_another_keys_index_fails_everywhere(ctx):
    keys, vkeys = four(ctx)
    rng = O.Prng(0x5A9)
    xs, abcs = K.forge_batch(keys, [2, 3], rng)
    data = device_batch(ctx, keys, [2, 3], abcs)
    inp, blob = K.flat_inputs(xs), data.tobytes()
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, 2)
    for key_of, want in (([2, 3], [1, 1]), ([3, 2], [0, 0])):
        for mode in MUL_MODES:
            with keys_mul(mode):
                ok, folded = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, coeffs=coeffs)
            assert ok is (want == [1, 1]) and api.gt_is_one(folded) == ok and folded.any()
        assert ctx.verify_keys_batch(vkeys, key_of, inp, blob).tolist() == want
        assert ctx.verify_keys_batch(vkeys, key_of, inp, blob, check_subgroup=True).tolist() == want
        ok, each = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, seed=SEED, each=True)
        assert ok is (want == [1, 1]) and each.tolist() == want


def test_a_c_moved_by_cofactor_torsion(ctx):
    """the pairing does not see the torsion part: only the subgroup test rejects the proof -- always in the folded forms"""
    keys, vkeys = four(ctx)
    rng = O.Prng(0x7025)
    key_of = [1, 2, 3, 2]
    xs, abcs = K.forge_batch(keys, key_of, rng)
    data = device_batch(ctx, keys, key_of, abcs)
    c = O.g1_add(O.g1_deserialize(data[3, 144:192].tobytes()), cofactor_torsion_point())
    data[3, 144:192] = np.frombuffer(O.g1_serialize(c), dtype=np.uint8)
    inp, blob = K.flat_inputs(xs), data.tobytes()
    ok, folded = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, coeffs=api.verify_aggregate_coeffs_from_seed(SEED, 4))
    assert ok is False and not folded.any()                         # an early rejection: all-zero words
    ok, each = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, seed=SEED, each=True)
    assert ok is False and each.tolist() == [1, 1, 1, 0]
    assert ctx.verify_keys_batch(vkeys, key_of, inp, blob, check_subgroup=True).tolist() == [1, 1, 1, 0]
    assert ctx.verify_keys_batch(vkeys, key_of, inp, blob).tolist() == [1, 1, 1, 1]


# ---- 4: degenerate segment sums ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["opposite", "equal"])
def test_a_segment_whose_two_terms_cancel_or_double(ctx, kind):
    """two proofs of one key under EQUAL coefficients with C and -C (the segment's sum is at infinity) or with the same C (the tree's
    first addition doubles); both proofs verify, by construction in integers, and a spoiled neighbour keeps the value off one"""
    keys, vkeys = four(ctx)
    rng = O.Prng(0xDE6 + len(kind))
    key_of = [1, 2, 2, 3]
    xs, abcs = K.forge_batch(keys, key_of, rng)
    c1 = abcs[1][2]
    abcs[2] = K.forge_with_c(keys[2].pks, keys[2].td, xs[2], (R - c1) if kind == "opposite" else c1, rng)
    assert (abcs[1][2] + abcs[2][2]) % R == 0 if kind == "opposite" else abcs[1][2] == abcs[2][2]
    data = device_batch(ctx, keys, key_of, abcs)
    assert (data[1, 144:192] == data[2, 144:192]).all() == (kind == "equal")
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, 4)
    coeffs[2] = coeffs[1]
    assert ctx.verify_keys_batch(vkeys, key_of, K.flat_inputs(xs), data.tobytes()).tolist() == [1, 1, 1, 1]
    for given, clean in ((xs, True), ([G.spoil(xs[0], 0)] + xs[1:], False), (xs[:1] + [G.spoil(xs[1], 1)] + xs[2:], False)):
        inp = K.flat_inputs(given)
        want = K.product_of_single_key(single_host(keys), api.gt_mul, keys, key_of, given, data, coeffs)
        for mode in MUL_MODES:
            with keys_mul(mode):
                ok, folded = ctx.verify_keys_aggregate(vkeys, key_of, inp, data.tobytes(), coeffs=coeffs)
            assert ok is clean and want[0] is clean and api.gt_is_one(folded) == clean
            assert np.array_equal(folded, want[1]) and folded.any()


# ---- 5: agreement with the single-key forms, refusals --------------------------------------------------------------------------------
def test_a_handle_listed_twice_is_two_keys(ctx):
    keys, vkeys = four(ctx)
    rng = O.Prng(0x2222)
    xs, abcs = K.forge_batch(keys, [3] * 4, rng)
    data = device_batch(ctx, keys, [3] * 4, abcs)
    given = [G.spoil(xs[0], 2)] + xs[1:]
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, 4)
    inp3, blob = G.inputs_mont(given), data.tobytes()
    s_ok, s_folded = ctx.groth16_verify_aggregate(vkeys[3], inp3, blob, coeffs=coeffs)
    ok, folded = ctx.verify_keys_aggregate([vkeys[3], vkeys[3]], [0, 1, 0, 1], K.flat_inputs(given), blob, coeffs=coeffs)
    assert ok is False and s_ok is False and np.array_equal(folded, s_folded) and not api.gt_is_one(folded)
    two = [keys[3], keys[3]]
    _, want = K.product_of_single_key(single_host(two), api.gt_mul, two, [0, 1, 0, 1], given, data, coeffs)
    assert np.array_equal(folded, want)
    assert ctx.verify_keys_batch([vkeys[3], vkeys[3]], [0, 1, 0, 1], K.flat_inputs(given), blob).tolist() == [0, 1, 1, 1]


def test_one_used_key_is_the_single_key_call(ctx):
    keys, vkeys = four(ctx)
    rng = O.Prng(0x0111)
    count = 70
    xs, abcs = K.forge_batch(keys, [2] * count, rng)
    data = device_batch(ctx, keys, [2] * count, abcs)
    given = [G.spoil(x, i % 3) if i % 9 == 4 else x for i, x in enumerate(xs)]
    want = [0 if i % 9 == 4 else 1 for i in range(count)]
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, count)
    inp3, blob = G.inputs_mont(given), data.tobytes()
    s_ok, s_folded = ctx.groth16_verify_aggregate(vkeys[2], inp3, blob, coeffs=coeffs)
    for vks, k in ((vkeys, 2), ([vkeys[2]], 0)):
        ok, folded = ctx.verify_keys_aggregate(vks, [k] * count, K.flat_inputs(given), blob, coeffs=coeffs)
        assert ok is False and s_ok is False and np.array_equal(folded, s_folded) and folded.any()
        for check in (False, True):
            got = ctx.verify_keys_batch(vks, [k] * count, K.flat_inputs(given), blob, check_subgroup=check).tolist()
            assert got == want and got == ctx.groth16_verify_batch(vkeys[2], inp3, blob, check_subgroup=check).tolist()
        assert ctx.verify_keys_aggregate(vks, [k] * count, K.flat_inputs(given), blob, seed=SEED, each=True)[1].tolist() == want


# ---- 6: the second level of the keyed sum ---------------------------------------------------------------------------------------------
LONG = 64 * 64 + 1      # 65 partials behind level 0: the smallest run with a second level (XYZZ in, no coefficients, the tree alone)
POOL = 8


def long_run(ctx):
    """Two keys (3 inputs and 1), POOL forged proofs each, and LONG coefficients below 2^100 for the long key's proofs plus one for the
    lone proof of the other key.  The long key's proof n is pool member n % POOL under r[n], so by bilinearity its folded value is the
    host form's on the POOL proofs under R_j = sum of r[n] over n % POOL == j (below 2^113).  Member 5's first input is spoiled in
    `given`.  The expected values are computed once, by the host form alone."""
    if "long" not in _DEV:
        four_keys, four_vkeys = four(ctx)
        keys, vkeys = [four_keys[2], four_keys[1]], [four_vkeys[2], four_vkeys[1]]
        rng = O.Prng(0x4097)
        key_of = [0] * POOL + [1] * POOL
        xs, abcs = K.forge_batch(keys, key_of, rng)
        data = device_batch(ctx, keys, key_of, abcs)
        given = [G.spoil(x, 0) if i == 5 else x for i, x in enumerate(xs)]
        r = [(rng.fr() % (1 << 100)) | 1 for _ in range(LONG + 1)]
        big = [sum(r[j:LONG:POOL]) for j in range(POOL)]
        assert all(0 < v < 1 << 128 for v in big) and sum(big) == sum(r[:LONG])
        want = {}
        for name, vecs in (("clean", xs), ("spoiled", given)):
            a_ok, a = single_host(keys)(0, G.inputs_mont(vecs[:POOL]), data[:POOL], big)
            b_ok, b = single_host(keys)(1, G.inputs_mont(vecs[POOL:POOL + 1]), data[POOL:POOL + 1], r[LONG:])
            assert b_ok is True and a_ok is (name == "clean") and api.gt_is_one(a) == a_ok and a.any()
            want[name] = (a, api.gt_mul(a, b))
        _DEV["long"] = SimpleNamespace(keys=keys, vkeys=vkeys, xs=xs, given=given, data=data, r=r, want=want)
    return _DEV["long"]


@pytest.mark.parametrize("shape", ["one_key", "two_keys_grouped", "lone_proof_in_the_middle"])
def test_the_second_level_of_the_keyed_sum(ctx, shape):
    """4 097 proofs of one key: 65 partials, so the keyed kernel runs a second time on its own output.  Alone (also through the
    single-key entry points, which plan one slot), with one proof of a second key behind it (the last wave of level 0 and wave 1 of
    level 1 hold pieces of two slots), and with that proof in the middle of the caller's order (a permutation that is not the identity)."""
    L = long_run(ctx)
    at = {"one_key": None, "two_keys_grouped": LONG, "lone_proof_in_the_middle": 2000}[shape]
    member = [(0, n % POOL, L.r[n]) for n in range(LONG)]      # (key, pool member, coefficient) per proof
    if at is not None:
        member.insert(at, (1, 0, L.r[LONG]))
    key_of = [k for k, _, _ in member]
    rows = [k * POOL + j for k, j, _ in member]
    coeffs = [c for _, _, c in member]
    blob = L.data[rows].tobytes()
    vkeys = L.vkeys if at is not None else L.vkeys[:1]
    for name, vecs in (("spoiled", L.given), ("clean", L.xs)):
        pool_in = [K.flat_inputs([x]) for x in vecs]
        inp = np.concatenate([pool_in[i] for i in rows])
        want = L.want[name][0 if at is None else 1]
        for mode in MUL_MODES:
            with keys_mul(mode):
                ok, folded = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, coeffs=coeffs)
                if at is None:
                    s_ok, s_folded = ctx.groth16_verify_aggregate(vkeys[0], inp.reshape(LONG, 3, 4), blob, coeffs=coeffs)
                    assert s_ok is ok and np.array_equal(s_folded, folded), (name, mode)
            assert ok is (name == "clean") and api.gt_is_one(folded) == ok, (name, mode)
            assert np.array_equal(folded, want), (name, mode)
        verdicts = [0 if (name == "spoiled" and i == 5) else 1 for i in rows]
        assert ctx.verify_keys_batch(vkeys, key_of, inp, blob, check_subgroup=True).tolist() == verdicts
        if at is None:
            assert ctx.groth16_verify_batch(vkeys[0], inp.reshape(LONG, 3, 4), blob).tolist() == verdicts
        ok, each = ctx.verify_keys_aggregate(vkeys, key_of, inp, blob, seed=SEED, each=True)
        assert ok is (name == "clean") and each.tolist() == verdicts


def test_refusals_name_the_index_and_leave_the_outputs_untouched(ctx):
    keys, vkeys = four(ctx)
    rng = O.Prng(0x4EF0)
    key_of = [1, 0, 2, 3, 1]
    xs, abcs = K.forge_batch(keys, key_of, rng)
    data = device_batch(ctx, keys, key_of, abcs)
    inp, blob = K.flat_inputs(xs), data.tobytes()
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, 5)
    assert inp.shape[0] == 8
    # through the Python API: the message names the first offending index
    bad_in = inp.copy()
    bad_in[6] = np.array([2 ** 64 - 1] * 4, dtype=np.uint64)
    for kw in (dict(coeffs=coeffs), dict(seed=SEED, each=True)):
        with pytest.raises(ZkError, match=r"key_of\[3\] = 4"):
            ctx.verify_keys_aggregate(vkeys, [1, 0, 2, 4, 7], inp, blob, **kw)
        with pytest.raises(ZkError, match=r"inputs_len = 7.*take 8"):
            ctx.verify_keys_aggregate(vkeys, key_of, inp[:7], blob, **kw)
        with pytest.raises(ZkError, match=r"public input 6 "):
            ctx.verify_keys_aggregate(vkeys, key_of, bad_in, blob, **kw)
        with pytest.raises(ZkError, match=r"take 10"):
            ctx.verify_keys_aggregate(vkeys, [1, 0, 2, 3, 3], inp, blob, **kw)
    with pytest.raises(ZkError, match=r"key_of\[3\] = 4"):
        ctx.verify_keys_batch(vkeys, [1, 0, 2, 4, 7], inp, blob)
    with pytest.raises(ZkError, match=r"public input 6 "):
        ctx.verify_keys_batch(vkeys, key_of, bad_in, blob)
    with pytest.raises(ZkError, match=r"inputs_len = 9"):
        ctx.verify_keys_batch(vkeys, key_of, np.concatenate([inp, inp[:1]]), blob)

    # through the C calls: every refusal, and the outputs as they were
    lib = ctx.lib
    handles = (C.c_void_p * 4)(*[v.h for v in vkeys])
    ko = np.array(key_of, dtype=np.uint32)
    buf = np.frombuffer(blob, dtype=np.uint8)
    seed = bytes(SEED)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    good = dict(ctx=ctx.h, vkeys=handles, n_keys=4, count=5, key_of=ko, inputs=inp, inputs_len=8, proofs=buf, coeffs=coeffs, seed=seed)

    def calls(**change):
        a = dict(good, **change)
        head = (a["ctx"], a["vkeys"], a["n_keys"], a["count"], p(a["key_of"]), p(a["inputs"]), a["inputs_len"], p(a["proofs"]))
        n_ok = max(a["count"], 1) if a["count"] < 100 else 1
        ok_all, folded = [C.c_int(7), C.c_int(7)], np.full(72, 9, dtype=np.uint64)
        ok = [np.full(n_ok, 7, dtype=np.int32), np.full(n_ok, 7, dtype=np.int32)]
        rcs = [lib.zk_groth16_vkeys_verify_aggregate_coeffs(*head, p(a["coeffs"]), C.byref(ok_all[0]), p(folded)),
               lib.zk_groth16_vkeys_verify_aggregate(*head, a["seed"], C.byref(ok_all[1]), p(ok[0])),
               lib.zk_groth16_vkeys_verify_batch(*head, 1, p(ok[1]))]
        assert rcs[0] == 0 or (ok_all[0].value == 7 and (folded == 9).all()), change
        assert rcs[1] == 0 or (ok_all[1].value == 7 and (ok[0] == 7).all()), change
        assert rcs[2] == 0 or (ok[1] == 7).all(), change
        return rcs

    assert calls() == [0, 0, 0]
    for name in ("ctx", "vkeys", "key_of", "inputs", "proofs"):
        assert calls(**{name: None}) == [ZK_ERR_ARG] * 3, name
    assert calls(coeffs=None, seed=None) == [ZK_ERR_ARG, ZK_ERR_ARG, 0]
    with_null = (C.c_void_p * 4)(vkeys[0].h, vkeys[1].h, None, vkeys[3].h)
    assert calls(vkeys=with_null) == [ZK_ERR_ARG] * 3
    assert calls(count=0) == [ZK_ERR_ARG] * 3 and calls(n_keys=0) == [ZK_ERR_ARG] * 3
    assert calls(n_keys=3) == [ZK_ERR_ARG] * 3                      # key_of holds a 3
    assert calls(inputs_len=7) == [ZK_ERR_ARG] * 3 and calls(inputs_len=9) == [ZK_ERR_ARG] * 3
    assert calls(inputs=bad_in) == [ZK_ERR_ARG] * 3
    head = (ctx.h, handles, 4, 5, p(ko), p(inp), 8, p(buf))
    assert lib.zk_groth16_vkeys_verify_aggregate_coeffs(*head, p(coeffs), None, None) == ZK_ERR_ARG
    assert lib.zk_groth16_vkeys_verify_aggregate(*head, seed, None, None) == ZK_ERR_ARG
    assert lib.zk_groth16_vkeys_verify_batch(*head, 0, None) == ZK_ERR_ARG
    # the lane limits, on two entries of the key without inputs (refused before a byte of the proofs is read; the pages are never touched)
    two = (C.c_void_p * 2)(vkeys[0].h, vkeys[0].h)
    for count, want in (((1 << 22) - 5, [ZK_ERR_ARG] * 3), ((1 << 22) // 3 + 1, None)):
        big_ko = np.zeros(count, dtype=np.uint32)
        big_ko[1::2] = 1
        big = dict(vkeys=two, n_keys=2, count=count, key_of=big_ko, inputs=None, inputs_len=0, proofs=np.zeros(count * 192, dtype=np.uint8),
                   coeffs=np.zeros((count, 2), dtype=np.uint64))
        if want is not None:
            assert calls(**big) == want
        else:      # 3 count above 2^22 is the batch form's limit alone
            ok = np.full(1, 7, dtype=np.int32)
            assert lib.zk_groth16_vkeys_verify_batch(ctx.h, two, 2, count, p(big_ko), None, 0, p(big["proofs"]), 0, p(ok)) == ZK_ERR_ARG and ok[0] == 7
            assert "3 count" in (lib.zk_last_error(ctx.h) or b"").decode()
