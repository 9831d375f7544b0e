"""Groth16 verification on the device (csrc/groth16_verify_keys.hip on a one-slot plan, csrc/groth16_verify.hip) on keys with 0, 1, 2, 3, 8 and 33 public inputs: zk_groth16_verify_batch
plain and checked, zk_groth16_verify_aggregate with coefficients, with a seed and with the verdicts of each.  The proofs are forged
from the trapdoor (groth16_verify_cases.py) for input vectors placed where k_verify_prepare's sum and the folded sum degenerate;
their points come from the scalars alone (zk_fixed_base_*_dev, serialised on the device), so a batch of thousands costs
milliseconds.  Verdicts are held to the construction (model_verdicts) and to the host forms on the same bytes, the folded value to
the host's word for word (tests/test_groth16_verify_inputs_host.py holds the host forms to the oracle)."""
import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from zk_mpc_amd import api
from zk_mpc_amd._lib import ZkError
from helpers import circuit_system, csr, mont1, td_mont
import groth16_verify_cases as G

pytestmark = pytest.mark.gpu

SEED = bytes(range(11, 43))
_KEYS = {}


class Key:
    """system(ni) set up on the device; its verifying key is the oracle's, point for point"""

    def __init__(self, ctx, ni):
        k = G.host_key(ni)
        self.k, self.td, self.pks, self.ninp, self.vk = k, k.td, k.pks, k.ninp, k.vk
        self.dr = ctx.r1cs_upload(k.r1cs.num_instance, k.r1cs.num_witness, csr(k.r1cs.a), csr(k.r1cs.b), csr(k.r1cs.c))
        self.pk = ctx.groth16_setup(self.dr, *td_mont(k.td))
        assert cv.g1_array_to_affine(self.pk.download("gamma_abc_g1")) == k.opk.gamma_abc_g1
        assert cv.g1_array_to_affine([self.pk.vk_g1(i) for i in range(3)]) == [k.opk.alpha_g1, k.opk.beta_g1, k.opk.delta_g1]
        assert cv.g2_array_to_affine([self.pk.vk_g2(i) for i in range(3)]) == [k.opk.beta_g2, k.opk.delta_g2, k.opk.gamma_g2]
        assert self.pk.points_in_subgroup


def key(ctx, ninp):
    if ninp not in _KEYS:
        _KEYS[ninp] = Key(ctx, ninp + 1)
    return _KEYS[ninp]


def device_proofs(ctx, td, abcs):
    """The proofs of the discrete logs abcs as (count, 192) bytes A | B | C: the points by zk_fixed_base_*_dev on g1_k G1 and
    g2_k G2, compressed on the device; the first two held to the oracle's points."""
    n = len(abcs)
    cols = []
    for which, group, gen_k in ((0, 1, td.g1_k), (1, 2, td.g2_k), (2, 1, td.g1_k)):
        d = ctx.upload(cv.fr_to_mont([abc[which] for abc in abcs]))
        tb = ctx.fixed_base(d.ptr, n, group, mont1(gen_k))
        cols.append(np.frombuffer(tb.serialize(compressed=True), dtype=np.uint8).reshape(n, 48 * group))
        tb.free()
        d.free()
    data = np.ascontiguousarray(np.concatenate(cols, axis=1))
    assert data.shape == (n, 192)
    for i in range(min(n, 2)):
        assert data[i].tobytes() == G.proof_bytes(td, abcs[i]), i
    return data


def forged(ctx, ky, xs, rng):
    return device_proofs(ctx, ky.td, [G.forge(ky.pks, ky.td, x, rng)[0] for x in xs])


def check_forms(ctx, pk, vk, xs, data, spoiled, host=True, coeffs=None):
    """Every device form on one batch: the verdicts are the construction's and (host) the host forms', the folded value the host's."""
    count = len(xs)
    inp, blob = G.inputs_mont(xs), data.tobytes()
    want, clean = G.model_verdicts(count, spoiled), not spoiled
    assert ctx.groth16_verify_batch(pk, inp, blob).tolist() == want
    assert ctx.groth16_verify_batch(pk, inp, blob, check_subgroup=True).tolist() == want
    ok, each = ctx.groth16_verify_aggregate(pk, inp, blob, seed=SEED, each=True)
    assert ok is clean and each.tolist() == want
    assert ctx.groth16_verify_aggregate(pk, inp, blob, seed=SEED) is clean
    if coeffs is None:
        coeffs = api.verify_aggregate_coeffs_from_seed(SEED, count)
    ok, folded = ctx.groth16_verify_aggregate(pk, inp, blob, coeffs=coeffs)
    assert ok is clean and api.gt_is_one(folded) == clean and folded.any()
    if host:
        for check in (False, True):
            got = [int(api.groth16_verify_host(inputs_mont=inp[i], proof=data[i].tobytes(), check_subgroup=check, **vk)) for i in range(count)]
            assert got == want, check
        h_ok, h_folded = api.groth16_verify_aggregate_host(inputs_mont=inp, proofs=blob, coeffs=coeffs, **vk)
        assert h_ok is clean and np.array_equal(folded, h_folded)


# ---- every named vector ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ninp", G.NINPS)
def test_every_named_vector_on_every_form(ctx, ninp):
    """One batch per key: every named vector clean, then once more per changed input (beyond 8 inputs: the first, the middle and the
    last one).  Without public inputs: two proofs, and the first with the C of the second."""
    ky = key(ctx, ninp)
    rng = O.Prng(0xD16A + ninp)
    if ninp == 0:
        abcs = [G.forge(ky.pks, ky.td, [], rng)[0] for _ in range(2)]
        abcs.append((abcs[0][0], abcs[0][1], abcs[1][2]))
        data = device_proofs(ctx, ky.td, abcs)
        check_forms(ctx, ky.pk, ky.vk, [[]] * 2, data[:2], set())
        check_forms(ctx, ky.pk, ky.vk, [[]] * 3, data, {2})
        return
    some = range(ninp) if ninp <= 8 else (0, ninp // 2, ninp - 1)
    true = [G.vector(name, ky.pks, rng) for name in G.vector_names(ninp)]
    proofs = forged(ctx, ky, true, rng)
    check_forms(ctx, ky.pk, ky.vk, true, proofs, set())
    xs, rows, spoiled = [], [], set()
    for i, x in enumerate(true):
        xs.append(x)
        rows.append(i)
        for j in some:
            spoiled.add(len(xs))
            xs.append(G.spoil(x, j))
            rows.append(i)
    check_forms(ctx, ky.pk, ky.vk, xs, proofs[rows], spoiled)


@pytest.mark.parametrize("swap", [False, True], ids=["plus_one", "rows_swapped"])
@pytest.mark.parametrize("ninp", [n for n in G.NINPS if n])
def test_sensitivity_batches(ctx, ninp, swap):
    ky = key(ctx, ninp)
    rng = O.Prng(0x5E46 + 2 * ninp + swap)
    true, given, spoiled = G.sensitivity(ky.pks, rng, swap)
    proofs = forged(ctx, ky, true, rng)
    check_forms(ctx, ky.pk, ky.vk, true, proofs, set(), host=ninp <= 8)
    check_forms(ctx, ky.pk, ky.vk, given, proofs, spoiled, host=ninp <= 8)


@pytest.mark.parametrize("name", G.fold_case_names(3))
def test_folded_only_cases(ctx, name):
    ky = key(ctx, 3)
    rng = O.Prng(0xF01E + sum(name.encode()))
    coeffs, xs = G.fold_case(name, ky.pks, rng)
    proofs = forged(ctx, ky, xs, rng)
    blob = proofs.tobytes()

    def both(given):
        inp = G.inputs_mont(given)
        ok, folded = ctx.groth16_verify_aggregate(ky.pk, inp, blob, coeffs=coeffs)
        h_ok, h_folded = api.groth16_verify_aggregate_host(inputs_mont=inp, proofs=blob, coeffs=coeffs, **ky.vk)
        assert ok is h_ok and np.array_equal(folded, h_folded) and folded.any()
        return ok, folded

    ok, folded = both(xs)
    assert ok is True and api.gt_is_one(folded)
    for i in range(len(xs)):
        for j in range(3):
            moved = [list(x) for x in xs]
            moved[i] = G.spoil(xs[i], j)
            ok, folded = both(moved)
            assert ok is False and not api.gt_is_one(folded), (i, j)


# ---- lane seams, three public inputs ---------------------------------------------------------------------------------------------------
_POOL = {}


def pool(ctx, count):
    """count forged proofs of the three-input key, the named vectors in turn (every ninth lane has its prepared input at infinity)"""
    if count not in _POOL:
        ky = key(ctx, 3)
        rng = O.Prng(0x9001 + count)
        names = G.vector_names(3)
        xs = [G.vector(names[i % len(names)], ky.pks, rng) for i in range(count)]
        _POOL[count] = (xs, forged(ctx, ky, xs, rng))
    return _POOL[count]


def spoiled_at(xs, at):
    given = [list(x) for x in xs]
    for n, k in enumerate(sorted(at)):
        given[k] = G.spoil(xs[k], n % 3)
    return given


@pytest.mark.parametrize("count", [1, 63, 64, 65, 130])
def test_batch_lane_seams(ctx, count):
    """proof k is lane k of k_verify_prepare and lanes 3 k .. 3 k + 2 of the Miller launch: a changed input in the last proof, in
    proofs 63 and 64, and in proof 21 (Miller lanes 63 .. 65), where present"""
    ky = key(ctx, 3)
    xs, proofs = pool(ctx, 130)
    at = {k for k in (21, 63, 64, count - 1) if k < count}
    check_forms(ctx, ky.pk, ky.vk, xs[:count], proofs[:count], set(), host=False)
    check_forms(ctx, ky.pk, ky.vk, spoiled_at(xs[:count], at), proofs[:count], at, host=count in (1, 65))


@pytest.mark.parametrize("count", [61, 62])      # Miller lanes 64 and 65
def test_aggregate_lane_seams(ctx, count):
    ky = key(ctx, 3)
    xs, proofs = pool(ctx, 130)
    check_forms(ctx, ky.pk, ky.vk, xs[:count], proofs[:count], set())
    check_forms(ctx, ky.pk, ky.vk, spoiled_at(xs[:count], {count - 1}), proofs[:count], {count - 1})


@pytest.mark.parametrize("count", [4096, 4097])
def test_aggregate_beyond_one_range_of_proofs(ctx, count):
    """4097 proofs: two ranges of the coefficient sums (2049 proofs each at most) and 65 partial sums of C for the device to sum
    down.  One changed input at proof 0, on either side of the range seam, in the last proof: rejected, and `each` names it."""
    ky = key(ctx, 3)
    xs, proofs = pool(ctx, 4097)
    xs, proofs = xs[:count], proofs[:count]
    inp, blob = G.inputs_mont(xs), proofs.tobytes()
    coeffs = api.verify_aggregate_coeffs_from_seed(SEED, count)
    ok, folded = ctx.groth16_verify_aggregate(ky.pk, inp, blob, coeffs=coeffs)
    assert ok is True and api.gt_is_one(folded)
    ok, each = ctx.groth16_verify_aggregate(ky.pk, inp, blob, seed=SEED, each=True)
    assert ok is True and each.tolist() == [1] * count
    for k in (0, 2048, 2049, count - 1):
        given = inp.copy()
        given[k] = G.inputs_mont([G.spoil(xs[k], k % 3)])[0]
        ok, folded = ctx.groth16_verify_aggregate(ky.pk, given, blob, coeffs=coeffs)
        assert ok is False and folded.any() and not api.gt_is_one(folded), k
        ok, each = ctx.groth16_verify_aggregate(ky.pk, given, blob, seed=SEED, each=True)
        assert ok is False and each.tolist() == G.model_verdicts(count, {k}), k


# ---- a proof from the prover; a key from its bytes ------------------------------------------------------------------------------------
def test_a_proof_of_the_prover_with_seven_public_inputs(ctx):
    rng = O.Prng(0x7107)
    r1cs, z = circuit_system((110, 7, 3), 2024)
    ni = r1cs.num_instance
    assert ni == 8
    dr = ctx.r1cs_upload(ni, r1cs.num_witness, csr(r1cs.a), csr(r1cs.b), csr(r1cs.c))
    pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])
    proof = ctx.create_proof(pk, dr, cv.fr_to_mont(z), mont1(rng.fr()), mont1(rng.fr()))
    vk = dict(alpha_g1=pk.vk_g1(0), beta_g2=pk.vk_g2(0), gamma_g2=pk.vk_g2(2), delta_g2=pk.vk_g2(1), gamma_abc_g1=pk.download("gamma_abc_g1"))
    x = z[1:ni]
    one = np.frombuffer(proof, dtype=np.uint8).reshape(1, 192)
    check_forms(ctx, pk, vk, [x], one, set())
    check_forms(ctx, pk, vk, [x] + [G.spoil(x, j) for j in range(7)], np.repeat(one, 8, axis=0), set(range(1, 8)))
    pk.free()


@pytest.mark.parametrize("compressed", [True, False], ids=["compressed", "uncompressed"])
def test_a_key_from_its_bytes_gives_the_same_verdicts(ctx, compressed):
    """(a loaded key is not known to lie in the subgroup: the folded form multiplies its points without the endomorphism)"""
    ky = key(ctx, 3)
    pk2, _, _ = S.proving_key_from_bytes(ctx, S.proving_key_bytes(ctx, ky.pk, compressed=compressed), compressed=compressed)
    assert not pk2.points_in_subgroup
    rng = O.Prng(0xB17E)
    for swap in (False, True):
        true, given, spoiled = G.sensitivity(ky.pks, rng, swap)
        proofs = forged(ctx, ky, true, rng)
        check_forms(ctx, pk2, ky.vk, true, proofs, set(), host=not swap)
        check_forms(ctx, pk2, ky.vk, given, proofs, spoiled, host=not swap)
    names = G.vector_names(3)
    xs = [G.vector(name, ky.pks, rng) for name in names]
    check_forms(ctx, pk2, ky.vk, xs, forged(ctx, ky, xs, rng), set())
    pk2.free()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals(ctx):
    ky = key(ctx, 3)
    xs, proofs = pool(ctx, 130)
    inp, blob = G.inputs_mont(xs[:2]), proofs[:2].tobytes()
    for width in (2, 4):                                # inputs_per_proof is not num_instance - 1
        wrong = np.zeros((2, width, 4), np.uint64)
        for check in (False, True):
            with pytest.raises(ZkError, match="inputs_per_proof"):
                ctx.groth16_verify_batch(ky.pk, wrong, blob, check_subgroup=check)
        with pytest.raises(ZkError, match="inputs_per_proof"):
            ctx.groth16_verify_aggregate(ky.pk, wrong, blob, seed=SEED)
        with pytest.raises(ZkError, match="inputs_per_proof"):
            ctx.groth16_verify_aggregate(ky.pk, wrong, blob, coeffs=[1, 1])
    with pytest.raises(ZkError, match="inputs_per_proof"):
        ctx.groth16_verify_batch(key(ctx, 0).pk, inp, blob)
    for i, j in ((0, 0), (1, 2)):                       # an input whose words are r
        at_r = inp.copy()
        at_r[i, j] = cv.fr_raw([O.R_MOD])[0]
        for check in (False, True):
            with pytest.raises(ZkError, match="not below r"):
                ctx.groth16_verify_batch(ky.pk, at_r, blob, check_subgroup=check)
        with pytest.raises(ZkError, match="not below r"):
            ctx.groth16_verify_aggregate(ky.pk, at_r, blob, seed=SEED, each=True)
        with pytest.raises(ZkError, match="not below r"):
            ctx.groth16_verify_aggregate(ky.pk, at_r, blob, coeffs=[1, 1])
    # no inputs where there are some: refused; without public inputs NULL is legal
    ok = np.zeros(2, np.int32)
    data = np.frombuffer(blob, dtype=np.uint8)
    assert ctx.lib.zk_groth16_verify_batch(ctx.h, ky.pk.h, 2, None, 3, data.ctypes.data, ok.ctypes.data) == -2
    k0 = key(ctx, 0)
    data0 = forged(ctx, k0, [[]], O.Prng(0x0E0))
    ok[:] = 7
    assert ctx.lib.zk_groth16_verify_batch(ctx.h, k0.pk.h, 1, None, 0, data0.ctypes.data, ok.ctypes.data) == 0 and ok[0] == 1
    one = api.C.c_int(7)
    co = np.array([[1, 0]], dtype=np.uint64)
    assert ctx.lib.zk_groth16_verify_aggregate_coeffs(ctx.h, k0.pk.h, 1, None, 0, data0.ctypes.data, co.ctypes.data, api.C.byref(one), None) == 0
    assert one.value == 1
    assert ctx.groth16_verify_batch(ky.pk, inp, blob).tolist() == [1, 1]      # the context is usable after the refusals
