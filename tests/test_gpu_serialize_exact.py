"""The byte layer on the device (csrc/serialize.hip), exactly: every case of serialize_cases.py through the loaders and the
serializer, the rule's refusals by name, the per-point verdicts of the batch verifier, the sign bit at its boundary, both launch
shapes past their grid (the loops that stride), and one bad bit inside a key and an SRS.  The expected reading of every byte string
is serialize_cases.classify (Python integers), which tests/test_serialize_model.py holds to the oracle."""
import functools
import time

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
from zk_mpc_amd import serialize as S
from helpers import golden, ih, mont1, r1cs_from_json, trapdoor_from_json
from pairing_cases import flip_sign
import serialize_cases as sc

pytestmark = pytest.mark.gpu

Q = O.Q_MOD
FORMS = [(g, c) for g in (1, 2) for c in (True, False)]
MESSAGE = {"noncanonical": "not below q", "flags": "flag", "curve": "not on the curve"}
CUTS = (1, 63, 64, 65, 255, 256, 257)          # the block edges of both launch shapes (64 lanes compressed, 256 otherwise)


def _to_array(group, pts):
    return cv.g1_affine_to_array(pts) if group == 1 else cv.g2_affine_to_array(pts)


def _to_affine(group, arr):
    return cv.g1_array_to_affine(arr) if group == 1 else cv.g2_array_to_affine(arr)


def _load(ctx, group, compressed, data, n, **kw):
    fn = ctx.bases_deserialize_compressed if compressed else ctx.bases_deserialize_uncompressed
    return fn(data, n, group, **kw)


# ---- accepted points ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,compressed", FORMS)
def test_accepted_points_load_and_serialise_back(ctx, group, compressed):
    pts, data, _ = sc.accepted(group, compressed)
    other = sc.accepted(group, not compressed)[1]
    size = sc.point_size(group, compressed)
    t = _load(ctx, group, compressed, data, len(pts))
    assert _to_affine(group, t.download()) == pts
    assert t.serialize(compressed) == data and t.serialize(not compressed) == other
    up = ctx.bases_upload(_to_array(group, pts), group)
    assert up.serialize(compressed) == data and up.serialize(not compressed) == other
    up.free()
    for cut in CUTS:                                  # `cut` points from index `cut` on: as a table of their own and as a range of the whole
        part = data[cut * size:2 * cut * size]
        assert t.serialize(compressed, offset=cut, n=cut) == part
        p = _load(ctx, group, compressed, part, cut)
        assert len(p) == cut and p.serialize(compressed) == part
        assert np.array_equal(p.download(), t.download(cut, cut))
        p.free()
    t.free()


# ---- rejections -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,compressed", FORMS)
def test_one_bad_point_anywhere_is_refused_by_the_name_of_its_rule(ctx, group, compressed):
    pts, data, inside = sc.accepted(group, compressed)
    size = sc.point_size(group, compressed)
    n = 130
    good = data[:n * size]
    assert all(inside[:n])
    bad = sc.one_bad_per_kind(group, compressed)
    assert {cls for _, cls, _ in bad} == set(MESSAGE)
    for kind, cls, b in bad:
        for at in (0, 77, n - 1):
            with pytest.raises(Z.ZkError, match="error -2: .*" + MESSAGE[cls]) as e:
                _load(ctx, group, compressed, good[:at * size] + b + good[(at + 1) * size:], n)
            assert sum(m in str(e.value) for m in MESSAGE.values()) == 1, (kind, str(e.value))
    # the checked loader refuses a subgroup point in non-canonical bytes too, and the context still loads the good table
    kind, cls, b = next(x for x in bad if x[0].endswith("=q+x"))
    with pytest.raises(Z.ZkError, match="not below q"):
        _load(ctx, group, compressed, good[:size] + b + good[2 * size:], n, check_subgroup=True)
    for check in (False, True):
        t = _load(ctx, group, compressed, good, n, check_subgroup=check)
        assert t.serialize(compressed) == good
        t.free()


# ---- per-point flags of the batch verifier ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verifier(ctx):
    """The D = 8 key of tests/golden/groth16.json made resident from the oracle's bytes, and its golden proof."""
    j = golden("groth16.json")["mul_chain_5"]
    r1cs, td = r1cs_from_json(j), trapdoor_from_json(j["trapdoor"])
    pk, _, _ = S.proving_key_from_bytes(ctx, O.pk_serialize(O.ProvingKey(O.ProvingKeyScalars(r1cs, td)), False))
    z = [ih(v) for v in j["z"]]
    yield pk, bytes.fromhex(j["proof"]), cv.fr_to_mont(z[1:j["num_instance"]])
    pk.free()


@pytest.mark.parametrize("check_subgroup", [False, True])
def test_batch_verdicts_are_per_proof(ctx, verifier, check_subgroup):
    pk, good, inputs = verifier
    alt = sc.altered_proofs(good)
    proofs = [good] * 65
    proofs[0], proofs[31], proofs[63] = alt["A.x + q"], alt["B.c0 + 2^377"], alt["C flags 0xC0"]
    proofs[64] = sc._add_to_element(good, 144, Q)            # C.x + q
    proofs[17] = flip_sign(good, 0)                          # canonical bytes of another point: refused by the pairing
    want = [0 if k in (0, 17, 31, 63, 64) else 1 for k in range(65)]
    got = ctx.groth16_verify_batch(pk, np.stack([inputs] * 65), proofs, check_subgroup=check_subgroup)
    assert got.tolist() == want
    for k in (0, 1, 31, 63):
        assert ctx.groth16_verify(pk, inputs, proofs[k], check_subgroup=check_subgroup) is bool(want[k])


# ---- the sign bit at its boundary ---------------------------------------------------------------------------------------------------
def test_sign_bit_at_the_boundary(ctx):
    """zk_bases_upload does not test the curve equation, so any y can be put under the serializer: y > -y changes between
    (q - 1) / 2 and (q + 1) / 2; on G2 the comparison is on c1 and falls through to c0 only when c1 = 0."""
    edge = [1, (Q - 1) // 2, (Q + 1) // 2, Q - 1]
    p1 = [(5 + k, y) for k, y in enumerate(edge)]
    p2 = [((3, 4 + k), (c0, 0)) for k, c0 in enumerate(edge)]
    p2 += [((6, 7), (c0, c1)) for c1 in edge for c0 in (0, 7, (Q - 1) // 2, (Q + 1) // 2, Q - 1)]
    assert [O._fq_gt_neg(y) for _, y in p1] == [False, False, True, True]
    assert [O._fq2_gt_neg(y) for _, y in p2[:4]] == [False, False, True, True]
    assert {O._fq2_gt_neg(y) == (y[1] > Q // 2) for _, y in p2[4:]} == {True}
    for group, pts, ser in ((1, p1, O.g1_serialize), (2, p2, O.g2_serialize)):
        t = ctx.bases_upload(_to_array(group, pts), group)
        assert t.serialize(True) == b"".join(ser(P) for P in pts)
        assert t.serialize(False) == b"".join(sc.serialize(group, False, P) for P in pts)
        t.free()


# ---- past the grid ----------------------------------------------------------------------------------------------------------------
BETA, GEN_K = 0x5E71A11CE5 * 0x9E3779B97F4A7C15 % O.R_MOD, 0xB10C5 * 0xC2B2AE3D27D4EB4F % O.R_MOD


@functools.lru_cache(maxsize=None)
def _oracle_point(group, i):
    k = GEN_K * pow(BETA, i, O.R_MOD) % O.R_MOD
    return O.g1_mul(O.G1_GEN, k) if group == 1 else O.g2_mul(O.G2_GEN, k)


def _table(ctx, group, n):
    """n points GEN_K * BETA^i * G made on the device: nothing of it passes through Python integers"""
    sc_dev = ctx.alloc(n * 32)
    ctx.fr_powers_dev(mont1(BETA), mont1(1), n, sc_dev.ptr)
    t = ctx.fixed_base(sc_dev.ptr, n, group, mont1(GEN_K))
    sc_dev.free()
    return t


@pytest.mark.parametrize("group,compressed,n,ends", [(1, True, (1 << 22) + 77, 64), (1, False, (1 << 16) + 77, 64), (2, False, (1 << 16) + 77, 64),
                                                     (1, False, (1 << 20) + 77, 8), (2, False, (1 << 20) + 77, 8)])
def test_tables_larger_than_the_launch(ctx, group, compressed, n, ends):
    """A lane takes a second point only in a table larger than its launch: the compressed loader launches at most 65 536 blocks of
    64 lanes (2^22 points), the uncompressed loader and the serializer at most 4 096 blocks of 256 (zk_grid's default cap: 2^20
    points).  So these cases are as large as they are: 2^22 + 77 compressed, 2^20 + 77 uncompressed for each group; 2^16 + 77 is a
    block count that is a multiple of nothing.  Bytes are compared as arrays; the oracle sees `ends` points at each end."""
    size = sc.point_size(group, compressed)
    t0 = time.time()
    t = _table(ctx, group, n)
    first = np.frombuffer(t.serialize(compressed), dtype=np.uint8)
    t1 = time.time()
    back = _load(ctx, group, compressed, first, n)
    second = np.frombuffer(back.serialize(compressed), dtype=np.uint8)
    t2 = time.time()
    assert first.size == n * size and np.array_equal(first, second)
    want = [sc.serialize(group, compressed, _oracle_point(group, i)) for i in list(range(ends)) + list(range(n - ends, n))]
    assert first[:ends * size].tobytes() == b"".join(want[:ends]) and first[-ends * size:].tobytes() == b"".join(want[ends:])
    assert np.array_equal(back.download(n - 64, 64), t.download(n - 64, 64))
    print("group %d %s n=%d: table+serialize %.2f s, load+serialize %.2f s, oracle %.2f s" % (
        group, "compressed" if compressed else "uncompressed", n, t1 - t0, t2 - t1, time.time() - t2))
    t.free()
    back.free()


# ---- keys and SRS -----------------------------------------------------------------------------------------------------------------
def _set_bit_381(data, last_byte_of_element):
    b = bytearray(data)
    assert not b[last_byte_of_element] & 0x20
    b[last_byte_of_element] |= 0x20
    return bytes(b)


def test_one_high_bit_in_a_key_or_an_srs_is_refused(ctx):
    rng = O.Prng(0x5E7)
    r1cs, _ = O.mul_chain_r1cs(9, rng.fr(), rng.fr())
    opk = O.ProvingKey(O.ProvingKeyScalars(r1cs, O.Trapdoor(*[rng.fr() for _ in range(7)])))
    for compressed in (True, False):
        data = O.pk_serialize(opk, compressed)
        pk, _, _ = S.proving_key_from_bytes(ctx, data, compressed=compressed)
        pk.free()
        for at in (47, len(data) - 1):                     # alpha_g1.x, and the last element of the last point of l_query
            for check in (False, True):
                with pytest.raises(Z.ZkError, match="not below q"):
                    S.proving_key_from_bytes(ctx, _set_bit_381(data, at), compressed=compressed, check_subgroup=check)
    max_degree = 6
    pp = O.KzgParams(max_degree, rng.fr(), g_k=rng.fr(), gg_k=rng.fr(), h_k=rng.fr())
    u64 = lambda v: v.to_bytes(8, "little")
    for compressed in (True, False):
        s1, s2 = (O.g1_serialize, O.g2_serialize) if compressed else (O.g1_serialize_uncompressed, O.g2_serialize_uncompressed)
        data = u64(max_degree + 1) + b"".join(s1(p) for p in pp.powers_of_g)
        data += u64(max_degree + 2) + b"".join(u64(i) + s1(p) for i, p in enumerate(pp.powers_of_gamma_g))
        at_h = len(data)
        data += s2(pp.h) + s2(pp.beta_h) + u64(0)
        pg, pgg, _, _ = S.kzg_srs_from_bytes(ctx, data, compressed)
        assert cv.g1_array_to_affine(pg.download()) == pp.powers_of_g
        pg.free(); pgg.free()
        for at in (8 + 3 * len(s1(None)) + 47, at_h + 47):   # x of powers_of_g[3]; the first element (x.c0) of h
            for check in (False, True):
                with pytest.raises(Z.ZkError, match="not below q"):
                    S.kzg_srs_from_bytes(ctx, _set_bit_381(data, at), compressed, check_subgroup=check)
