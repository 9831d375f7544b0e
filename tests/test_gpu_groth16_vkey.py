"""The verifier's own key on the device (csrc/groth16_vkey.hip: zk_vkey) and prepare_inputs as a fixed-base kernel
(csrc/g1_prepare_inputs.hip): loading and writing a verifying key, every verification form on it held to the pk forms, the host forms
and the construction (groth16_verify_cases.py), the kernel on synthetic keys whose gamma_abc discrete logs are chosen so that its
additions degenerate, prepared verification, a key with 1000 public inputs end to end, the path without a window table, refusals.

A synthetic key takes alpha .. delta from the oracle's one-input key and gamma_abc[j] = k_j G; the expected prepared input is
(k_0 + sum x_j k_{j+1}) G, one zk_fixed_base_g1_dev call per case.  Proofs for it are forged from the same trapdoor with gamma_abc's
logs relative to the key's G1 generator."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from zk_mpc_amd import api
from zk_mpc_amd._lib import ZkError
from helpers import mont1
from marlin_verify_cases import cofactor_torsion_point
import groth16_verify_cases as G
from test_gpu_groth16_verify_inputs import SEED, check_forms, device_proofs, forged, key

pytestmark = pytest.mark.gpu

R = O.R_MOD
ZK_ERR_ARG = -2
NINP_SEAMS = (1, 2, 15, 16, 17, 63, 64, 65, 130, 1000)      # the seams of the stripe and segment packing
KINDS = ("same", "pairs", "pow16", "one_inf", "random")
BASE = G.host_key(2)                                         # alpha .. delta and their trapdoor


def gmul(ctx, ks):
    """k G1 for every k (mod r) as (n, 12) uint64; zero words for k = 0"""
    d = ctx.upload(cv.fr_to_mont([k % R for k in ks]))
    tb = ctx.fixed_base(d.ptr, len(ks), 1, mont1(1))
    out = tb.download()
    tb.free()
    d.free()
    for i, k in enumerate(ks):
        assert out[i].any() == (k % R != 0)
    return out


def logs(kind, ninp, rng):
    """k_0 .. k_ninp of a synthetic key"""
    n = ninp + 1
    if kind == "same":
        return [G.nonzero(rng)] * n
    if kind == "pairs":
        half = [G.nonzero(rng) for _ in range((n + 1) // 2)]
        return [half[j // 2] if j % 2 == 0 else R - half[j // 2] for j in range(n)]
    if kind == "pow16":
        return [pow(16, j, R) for j in range(n)]
    ks = [G.nonzero(rng) for _ in range(n)]
    if kind == "one_inf":
        ks[(ninp + 1) // 2] = 0
    return ks


def synthetic(ctx, ks):
    """-> (vkey, host view) of the key with gamma_abc[j] = ks[j] G"""
    vk = dict(BASE.vk, gamma_abc_g1=gmul(ctx, ks))
    return ctx.vkey_upload(**vk), vk


def pool(ninp, rng, equal):
    """69 input vectors: zeros, ones, tops, one non-zero digit in every window position (vector i: input j holds d 16^((i + j) % 64)),
    then random ones; equal: every input of a vector holds the vector's first value"""
    digit = lambda w, d: (1 if w == 63 else d) << (4 * w)
    xs = [[0] * ninp, [1] * ninp, [R - 1] * ninp]
    xs += [[digit((i + j) % 64, 1 + (i + j) % 15) for j in range(ninp)] for i in range(64)]
    xs += [[rng.fr() for _ in range(ninp)] for _ in range(2)]
    assert len(xs) == 69 and all(v < R for x in xs for v in x)
    return [[x[0]] * ninp for x in xs] if equal else xs


def expected(ctx, ks, xs):
    return gmul(ctx, [ks[0] + sum(v * k for v, k in zip(x, ks[1:])) for x in xs])


# ---- 1. loading ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ninp", G.NINPS)
def test_loading_from_bytes_host_view_and_proving_key(ctx, ninp):
    ky = key(ctx, ninp)
    made = []
    for compressed in (True, False):
        data = O.vk_serialize(ky.k.opk, compressed)
        assert data == S.verifying_key_bytes(ctx, ky.pk, compressed=compressed)
        made += [ctx.vkey_deserialize(data, compressed=compressed), S.verifying_key_from_bytes(ctx, data, compressed=compressed, check_subgroup=True)]
    made += [ctx.vkey_upload(**ky.vk), ctx.vkey_upload(check_subgroup=True, **ky.vk), ky.pk.vkey()]
    for vk in made:
        assert vk.num_inputs == ninp
        for compressed in (True, False):
            assert vk.serialize(compressed) == O.vk_serialize(ky.k.opk, compressed)
        vk.free()


# ---- 2. verdict parity ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ninp", G.NINPS)
def test_every_form_on_a_vkey_gives_the_verdicts_of_the_pk_and_host_forms(ctx, ninp):
    """check_forms holds every device form to the construction and to the host forms, the folded value to the host's word for word:
    on the key's own pk forms, on a vkey from the oracle's bytes and on a vkey copied from the pk."""
    ky = key(ctx, ninp)
    rng = O.Prng(0x7E11 + ninp)
    vkeys = [ky.pk, ctx.vkey_deserialize(O.vk_serialize(ky.k.opk)), ky.pk.vkey()]
    if ninp == 0:
        abcs = [G.forge(ky.pks, ky.td, [], rng)[0] for _ in range(2)]
        abcs.append((abcs[0][0], abcs[0][1], abcs[1][2]))
        data = device_proofs(ctx, ky.td, abcs)
        for vk in vkeys:
            check_forms(ctx, vk, ky.vk, [[]] * 3, data, {2})
    else:
        true = [G.vector(name, ky.pks, rng) for name in G.vector_names(ninp)]
        proofs = forged(ctx, ky, true, rng)
        xs, rows, spoiled = [], [], set()
        for i, x in enumerate(true):
            xs += [x, G.spoil(x, (i * 7) % ninp)]
            rows += [i, i]
            spoiled.add(len(xs) - 1)
        s_true, s_given, s_spoiled = G.sensitivity(ky.pks, rng)
        s_proofs = forged(ctx, ky, s_true, rng)
        for n, vk in enumerate(vkeys):
            check_forms(ctx, vk, ky.vk, true, proofs, set(), host=n == 1)
            check_forms(ctx, vk, ky.vk, xs, proofs[rows], spoiled, host=n == 1 and ninp <= 8)
            check_forms(ctx, vk, ky.vk, s_given, s_proofs, s_spoiled, host=False)
    for vk in vkeys[1:]:
        vk.free()


@pytest.mark.parametrize("name", G.fold_case_names(3))
def test_folded_only_cases_on_a_vkey(ctx, name):
    ky = key(ctx, 3)
    rng = O.Prng(0xF01F + sum(name.encode()))
    coeffs, xs = G.fold_case(name, ky.pks, rng)
    blob = forged(ctx, ky, xs, rng).tobytes()
    vk = ky.pk.vkey()
    for given, clean in ((xs, True), ([G.spoil(xs[0], 1)] + xs[1:], False)):
        inp = G.inputs_mont(given)
        ok, folded = ctx.groth16_verify_aggregate(vk, inp, blob, coeffs=coeffs)
        p_ok, p_folded = ctx.groth16_verify_aggregate(ky.pk, inp, blob, coeffs=coeffs)
        h_ok, h_folded = api.groth16_verify_aggregate_host(inputs_mont=inp, proofs=blob, coeffs=coeffs, **ky.vk)
        assert ok is clean and p_ok is clean and h_ok is clean
        assert np.array_equal(folded, h_folded) and np.array_equal(p_folded, h_folded) and api.gt_is_one(folded) == clean
    vk.free()


# ---- 3. the kernel on synthetic keys --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ninp", NINP_SEAMS)
@pytest.mark.parametrize("kind", KINDS)
def test_prepare_inputs_on_synthetic_keys(ctx, kind, ninp):
    rng = O.Prng(0x5EA0 + 31 * ninp + KINDS.index(kind))
    ks = logs(kind, ninp, rng)
    vkey, vk = synthetic(ctx, ks)
    xs = pool(ninp, rng, equal=kind == "pairs")
    want = expected(ctx, ks, xs)
    assert want[0].tolist() == vk["gamma_abc_g1"][0].tolist()                  # all-zero inputs: gamma_abc[0]
    for lo, count in ((0, 65), (65, 3), (68, 1)):
        got = ctx.groth16_prepare_inputs(vkey, G.inputs_mont(xs[lo:lo + count]))
        assert np.array_equal(got, want[lo:lo + count]), (lo, count)
    if ninp <= 65:
        for i in (2, 3, 67):
            assert api.groth16_prepare_inputs_host(inputs_mont=G.inputs_mont([xs[i]])[0], **vk).tolist() == want[i].tolist(), i
    vkey.free()


# ---- 4, 5: proofs for a synthetic key ---------------------------------------------------------------------------------------------------
def synthetic_with_proofs(ctx, ninp, count, seed):
    """a random synthetic key, count input vectors, their forged proofs -> (vkey, vk, ks, xs, proofs)"""
    rng = O.Prng(seed)
    ks = logs("random", ninp, rng)
    vkey, vk = synthetic(ctx, ks)
    pks = SimpleNamespace(gamma_abc=[k * G.inv(BASE.td.g1_k) % R for k in ks])
    xs = [[rng.fr() for _ in range(ninp)] for _ in range(count)]
    proofs = device_proofs(ctx, BASE.td, [G.forge(pks, BASE.td, x, rng)[0] for x in xs])
    return vkey, vk, ks, xs, proofs


def test_prepared_verification(ctx):
    vkey, vk, ks, xs, proofs = synthetic_with_proofs(ctx, 17, 5, 0x94E9)
    blob = proofs.tobytes()
    given = [list(x) for x in xs]
    given[1] = G.spoil(xs[1], 16)
    for check in (False, True):
        for inputs, want in ((xs, [1] * 5), (given, [1, 0, 1, 1, 1])):
            inp = G.inputs_mont(inputs)
            prepared = ctx.groth16_prepare_inputs(vkey, inp)
            assert np.array_equal(prepared, expected(ctx, ks, inputs))
            assert ctx.groth16_verify_batch(vkey, inp, blob, check_subgroup=check).tolist() == want
            assert ctx.groth16_verify_prepared(vkey, prepared, blob, check_subgroup=check).tolist() == want
    moved = ctx.groth16_prepare_inputs(vkey, G.inputs_mont(xs))
    moved[2] = gmul(ctx, [ks[0] + sum(v * k for v, k in zip(xs[2], ks[1:])) + 1])[0]      # + G
    assert ctx.groth16_verify_prepared(vkey, moved, blob).tolist() == [1, 1, 0, 1, 1]
    vkey.free()


def thousand_inputs_end_to_end(ctx, count):
    vkey, vk, ks, xs, proofs = synthetic_with_proofs(ctx, 1000, count, 0x1000 + count)
    assert vkey.num_inputs == 1000
    bad = count // 2
    given = [list(x) for x in xs]
    given[bad] = G.spoil(xs[bad], 999)
    for inputs, spoiled in ((xs, set()), (given, {bad})):
        check_forms(ctx, vkey, vk, inputs, proofs, spoiled, host=False)
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, count)
    out = [ctx.groth16_verify_aggregate(vkey, G.inputs_mont(inputs), proofs.tobytes(), coeffs=coeffs) for inputs in (xs, given)]
    vkey.free()
    return out


@pytest.mark.parametrize("count", [1, 5])
def test_a_thousand_public_inputs_end_to_end(ctx, count):
    (ok, folded), (bad_ok, bad_folded) = thousand_inputs_end_to_end(ctx, count)
    assert ok is True and api.gt_is_one(folded) and bad_ok is False and not api.gt_is_one(bad_folded)


# ---- 6. beyond the table limit ------------------------------------------------------------------------------------------------------------
def test_without_a_window_table_the_results_are_the_same(ctx):
    results = {}
    try:
        for limit in (0, None):
            ctx.groth16_prepare_table_limit(limit)
            for ninp in (1, 255, 256, 300):
                rng = O.Prng(0x6A00 + ninp)
                ks = logs("random", ninp, rng)
                vkey, _ = synthetic(ctx, ks)
                xs = [[rng.fr() for _ in range(ninp)] for _ in range(5)]
                want = expected(ctx, ks, xs)
                for count in (1, 5):
                    got = ctx.groth16_prepare_inputs(vkey, G.inputs_mont(xs[:count]))
                    assert np.array_equal(got, want[:count]), (limit, ninp, count)
                vkey.free()
            results[limit] = thousand_inputs_end_to_end(ctx, 1)
    finally:
        ctx.groth16_prepare_table_limit(None)
    (ok, folded), (bad_ok, bad_folded) = results[0]
    assert ok is True and bad_ok is False
    assert np.array_equal(folded, results[None][0][1]) and np.array_equal(bad_folded, results[None][1][1])


# ---- 7. refusals ------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    ky = key(ctx, 3)
    rng = O.Prng(0x4EF0)
    xs = [G.vector("random", ky.pks, rng) for _ in range(2)]
    proofs = forged(ctx, ky, xs, rng)
    inp, blob = G.inputs_mont(xs), proofs.tobytes()
    good = O.vk_serialize(ky.k.opk)
    vkey = ctx.vkey_deserialize(good)
    lib, h = ctx.lib, C.c_void_p()
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    buf, ok, prep = np.frombuffer(blob, dtype=np.uint8), np.zeros(2, np.int32), np.zeros((2, 12), np.uint64)
    host_vk, _abc = api._vk_host(**ky.vk)

    def nothing_made():
        assert h.value is None
        assert ctx.groth16_verify_batch(vkey, inp, blob).tolist() == [1, 1]      # ... and the context still verifies a good batch

    # null pointers, count = 0
    raw = np.frombuffer(good, dtype=np.uint8)
    assert lib.zk_vkey_upload(ctx.h, None, 0, C.byref(h)) == ZK_ERR_ARG and lib.zk_vkey_upload(ctx.h, C.byref(host_vk), 0, None) == ZK_ERR_ARG
    assert lib.zk_vkey_deserialize(ctx.h, None, len(good), 1, 0, C.byref(h)) == ZK_ERR_ARG
    assert lib.zk_vkey_deserialize(ctx.h, p(raw), len(good), 1, 0, None) == ZK_ERR_ARG
    assert lib.zk_vkey_from_pk(ctx.h, None, C.byref(h)) == ZK_ERR_ARG
    for count, key_h, inputs, data, out in ((0, vkey.h, inp, buf, ok), (2, None, inp, buf, ok), (2, vkey.h, None, buf, ok), (2, vkey.h, inp, None, ok),
                                            (2, vkey.h, inp, buf, None)):
        assert lib.zk_groth16_vkey_verify_batch(ctx.h, key_h, count, p(inputs), 3, p(data), 0, p(out)) == ZK_ERR_ARG
    for count, key_h, inputs, out in ((0, vkey.h, inp, prep), (2, None, inp, prep), (2, vkey.h, None, prep), (2, vkey.h, inp, None)):
        assert lib.zk_groth16_prepare_inputs(ctx.h, key_h, count, p(inputs), 3, p(out)) == ZK_ERR_ARG
    assert lib.zk_groth16_vkey_verify_prepared(ctx.h, vkey.h, 2, None, p(buf), 0, p(ok)) == ZK_ERR_ARG
    assert lib.zk_groth16_vkey_verify_prepared(ctx.h, vkey.h, 0, p(prep), p(buf), 0, p(ok)) == ZK_ERR_ARG
    nothing_made()
    # inputs_per_proof off by one; an input equal to r
    at_r = inp.copy()
    at_r[1, 2] = cv.fr_raw([R])[0]
    for wrong, words in ((np.zeros((2, 2, 4), np.uint64), "inputs_per_proof"), (np.zeros((2, 4, 4), np.uint64), "inputs_per_proof"), (at_r, "not below r")):
        for call in (lambda a: ctx.groth16_verify_batch(vkey, a, blob), lambda a: ctx.groth16_verify_batch(vkey, a, blob, check_subgroup=True),
                     lambda a: ctx.groth16_verify_aggregate(vkey, a, blob, seed=SEED, each=True),
                     lambda a: ctx.groth16_verify_aggregate(vkey, a, blob, coeffs=[1, 1]), lambda a: ctx.groth16_prepare_inputs(vkey, a)):
            with pytest.raises(ZkError, match=words):
                call(wrong)
    # gamma_g2 at infinity
    with pytest.raises(ZkError, match="gamma_g2"):
        ctx.vkey_upload(**dict(ky.vk, gamma_g2=np.zeros(24, np.uint64)))
    # bytes truncated by one, one trailing byte, a length word that does not fit, an abscissa that is q
    q_bytes = O.Q_MOD.to_bytes(48, "little")
    for compressed in (True, False):
        data = O.vk_serialize(ky.k.opk, compressed)
        at = (48 + 3 * 96) if compressed else (96 + 3 * 192)
        per = 48 if compressed else 96
        cases = [data[:-1], data + b"\0", data[:at] + (5).to_bytes(8, "little") + data[at + 8:], data[:at] + (2 ** 40).to_bytes(8, "little") + data[at + 8:],
                 q_bytes + data[48:], data[:at + 8 + per] + q_bytes + data[at + 8 + per + 48:]]
        for n, case in enumerate(cases):
            for check in (False, True):
                with pytest.raises(ZkError):
                    ctx.vkey_deserialize(case, compressed=compressed, check_subgroup=check)
    nothing_made()
    # a gamma_abc point moved by a point of the cofactor torsion: refused with check_subgroup, loaded without
    moved = list(ky.k.opk.gamma_abc_g1)
    moved[2] = O.g1_add(moved[2], cofactor_torsion_point())
    opk = SimpleNamespace(**dict(vars(ky.k.opk), gamma_abc_g1=moved))
    for compressed in (True, False):
        data = O.vk_serialize(opk, compressed)
        with pytest.raises(ZkError, match="subgroup"):
            ctx.vkey_deserialize(data, compressed=compressed, check_subgroup=True)
        loaded = ctx.vkey_deserialize(data, compressed=compressed)
        assert loaded.serialize(compressed) == data
        loaded.free()
    host_moved = dict(ky.vk, gamma_abc_g1=cv.g1_affine_to_array(moved))
    with pytest.raises(ZkError, match=r"gamma_abc_g1\[2\] is outside the subgroup"):
        ctx.vkey_upload(check_subgroup=True, **host_moved)
    ctx.vkey_upload(**host_moved).free()
    nothing_made()
    vkey.free()
