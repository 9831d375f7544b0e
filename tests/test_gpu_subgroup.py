"""GPU: subgroup membership on the device (csrc/subgroup.hip) -- the kernel over tables, the checked loaders, the key check and the
checked Groth16 verification.  The expected verdict everywhere is the reference's own test r P == O through the oracle's plain
double-and-add (subgroup_cases.py); every case of every table is compared."""
import ctypes as C
import functools

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from zk_mpc_amd import api
from helpers import golden, ih, r1cs_from_json, trapdoor_from_json
from marlin_verify_cases import cofactor_torsion_point
import subgroup_cases as sc

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 200]      # a partial wave, a full wave, a one-lane tail, several blocks


def _to_affine(group, arr):
    return (cv.g1_array_to_affine if group == 1 else cv.g2_array_to_affine)(arr)


def _add(group, P, Q):
    return O.ec_add(P, Q, O.FqOps if group == 1 else O.Fq2Ops)


def _torsion(group):
    return cofactor_torsion_point() if group == 1 else sc.g2_cofactor_torsion_point()


@functools.lru_cache(maxsize=None)
def _clean(group, n=65):
    rng = O.Prng(0x5B60 + group)
    gen, ops = (O.G1_GEN, O.FqOps) if group == 1 else (O.G2_GEN, O.Fq2Ops)
    pts = [O.ec_mul_raw(gen, rng.fr(), ops) for _ in range(n)]
    pts[7] = None
    return pts


# ---- the kernel against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", SIZES)
def test_kernel_flags_equal_the_oracle(ctx, group, n):
    pts, want = sc.table(group, n)
    b = ctx.bases_upload(sc.abi_array(group, pts), group)
    each, n_out, first = ctx.bases_subgroup_check(b)
    assert [int(v) for v in each] == [int(f) for f in want]
    assert n_out == want.count(False)
    assert first == (want.index(False) if False in want else None)
    # the host form agrees on the same list
    assert [int(v) for v in api.in_subgroup_host(sc.abi_array(group, pts), group)] == [int(v) for v in each]
    b.free()


@pytest.mark.parametrize("group", [1, 2])
def test_a_sub_range_sees_only_its_own_points(ctx, group):
    pts, want = sc.table(group, 200)
    b = ctx.bases_upload(sc.abi_array(group, pts), group)
    each, n_out, first = ctx.bases_subgroup_check(b, offset=3, n=70)
    sub = want[3:73]
    assert [int(v) for v in each] == [int(f) for f in sub]
    assert n_out == sub.count(False) and first == sub.index(False)
    # a range of points that are all inside, between points that are not
    inside = [i for i, f in enumerate(want) if f]
    run = next(i for i in inside if want[i:i + 2] == [True, True])
    each, n_out, first = ctx.bases_subgroup_check(b, offset=run, n=2)
    assert list(each) == [1, 1] and n_out == 0 and first is None
    each, n_out, first = ctx.bases_subgroup_check(b, offset=200, n=0)
    assert len(each) == 0 and n_out == 0 and first is None
    b.free()


# ---- checked loaders -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("compressed", [True, False])
def test_checked_loader_accepts_a_clean_table_and_names_the_bad_point(ctx, group, compressed):
    pts = list(_clean(group))
    data = sc.serialize(group, pts, compressed)
    load = ctx.bases_deserialize_compressed if compressed else ctx.bases_deserialize_uncompressed
    plain, checked = load(data, 65, group), load(data, 65, group, check_subgroup=True)
    assert np.array_equal(plain.download(), checked.download())
    assert _to_affine(group, checked.download()) == pts
    plain.free(); checked.free()
    pts[64] = _add(group, pts[64], _torsion(group))
    data = sc.serialize(group, pts, compressed)
    load(data, 65, group).free()                              # on the curve: the unchecked loader takes it
    with pytest.raises(Z.ZkError, match=r"error -2: .*point 64 is not in the prime-order subgroup"):
        load(data, 65, group, check_subgroup=True)


def test_checked_loader_refuses_the_order_3_point(ctx):
    """Compressed G1 bytes with x = 0 and no infinity flag: (0, +-1), a point of order 3 -- where (0, 1) WITH the flag is how the
    uncompressed form writes infinity."""
    for sign in (0, 0x80):
        data = bytes(47) + bytes([sign])
        b = ctx.bases_deserialize_compressed(data, 1, 1)
        (P,) = _to_affine(1, b.download())
        assert P in ((0, 1), (0, O.Q_MOD - 1))
        b.free()
        with pytest.raises(Z.ZkError, match="error -2: .*point 0 is not in the prime-order subgroup"):
            ctx.bases_deserialize_compressed(data, 1, 1, check_subgroup=True)
    unc = O.g1_serialize_uncompressed(sc.G1_ORDER3)
    with pytest.raises(Z.ZkError, match="error -2: .*point 0 is not in the prime-order subgroup"):
        ctx.bases_deserialize_uncompressed(unc, 1, 1, check_subgroup=True)
    inf = ctx.bases_deserialize_uncompressed(O.g1_serialize_uncompressed(None), 1, 1, check_subgroup=True)
    assert _to_affine(1, inf.download()) == [None]
    inf.free()


def test_checked_srs_loader(ctx):
    rng = O.Prng(0x5B65)
    max_degree = 15                                           # 2^4 powers
    pp = O.KzgParams(max_degree, rng.fr(), g_k=rng.fr(), gg_k=rng.fr(), h_k=rng.fr())
    u64 = lambda v: v.to_bytes(8, "little")

    def srs_bytes(powers_g, powers_gamma_g, h, beta_h):
        out = u64(len(powers_g)) + b"".join(O.g1_serialize(p) for p in powers_g)
        out += u64(len(powers_gamma_g)) + b"".join(u64(i) + O.g1_serialize(p) for i, p in enumerate(powers_gamma_g))
        return out + O.g2_serialize(h) + O.g2_serialize(beta_h) + u64(0)

    pg, pgg = list(pp.powers_of_g), list(pp.powers_of_gamma_g)
    good = srs_bytes(pg, pgg, pp.h, pp.beta_h)
    a, b, h, bh = S.kzg_srs_from_bytes(ctx, good, True, check_subgroup=True)
    assert cv.g1_array_to_affine(a.download()) == pg and cv.g1_array_to_affine(b.download()) == pgg
    assert cv.g2_array_to_affine(h.reshape(1, 24)) == [pp.h] and cv.g2_array_to_affine(bh.reshape(1, 24)) == [pp.beta_h]
    a.free(); b.free()
    T, T2 = cofactor_torsion_point(), sc.g2_cofactor_torsion_point()
    moved_g = pg[:9] + [O.g1_add(pg[9], T)] + pg[10:]
    moved_gg = pgg[:3] + [O.g1_add(pgg[3], T)] + pgg[4:]
    for data, what in ((srs_bytes(moved_g, pgg, pp.h, pp.beta_h), r"powers_of_g\[9\]"),
                       (srs_bytes(pg, moved_gg, pp.h, pp.beta_h), r"powers_of_gamma_g\[3\]"),
                       (srs_bytes(pg, pgg, O.g2_add(pp.h, T2), pp.beta_h), "h is not"),
                       (srs_bytes(pg, pgg, pp.h, O.g2_add(pp.beta_h, T2)), "beta_h is not")):
        a, b, _, _ = S.kzg_srs_from_bytes(ctx, data, True)    # on the curve: the unchecked loader takes it
        a.free(); b.free()
        with pytest.raises(Z.ZkError, match="error -2: .*" + what):
            S.kzg_srs_from_bytes(ctx, data, True, check_subgroup=True)
    # the outputs are not written on a refusal
    pgh, pggh = C.c_void_p(), C.c_void_p()
    hh, bhh = np.zeros(24, np.uint64), np.zeros(24, np.uint64)
    data = srs_bytes(pg, pgg, pp.h, O.g2_add(pp.beta_h, T2))
    rc = ctx.lib.zk_kzg_srs_deserialize_checked(ctx.h, data, len(data), 1, C.byref(pgh), C.byref(pggh), hh.ctypes.data, bhh.ctypes.data)
    assert rc == -2 and not pgh.value and not pggh.value and not hh.any() and not bhh.any()


# ---- keys ------------------------------------------------------------------------------------------------------------------------------
LOG_D = 6


class KeyCase:
    """A setup key of a mul-chain system that fills its domain (D = 2^6), its uncompressed bytes and where the queries sit in them."""

    def __init__(self, ctx):
        rng = O.Prng(0x5B66)
        n = (1 << LOG_D) - 2
        self.tdm = cv.fr_to_mont([rng.fr() for _ in range(7)])
        self.dr = ctx.r1cs_mul_chain(n)
        self.pk = ctx.groth16_setup(self.dr, *[self.tdm[i] for i in range(7)])
        self.data = S.proving_key_bytes(ctx, self.pk, False)
        # vk: alpha_g1 | beta_g2 gamma_g2 delta_g2 | Vec gamma_abc_g1; then beta_g1 delta_g1 | Vec a | b_g1 | b_g2 | h | l
        u64 = lambda at: int.from_bytes(self.data[at:at + 8], "little")
        at = 96 + 3 * 192
        self.off = {}
        for name, size in (("gamma_abc_g1", 96), (None, 0), ("a_query", 96), ("b_g1_query", 96), ("b_g2_query", 192), ("h_query", 96), ("l_query", 96)):
            if name is None:
                at += 2 * 96
                continue
            self.off[name] = (at + 8, u64(at), size)
            at += 8 + u64(at) * size
        assert at == len(self.data)

    def moved(self, name, index):
        """the key's bytes with query[index] moved by a torsion point of its group"""
        at, n, size = self.off[name]
        assert index < n
        group = 2 if size == 192 else 1
        lo = at + index * size
        (P,) = _to_affine(group, self.pk.download(name, index, 1))
        Pm = _add(group, P, _torsion(group))
        ser = O.g1_serialize_uncompressed if group == 1 else O.g2_serialize_uncompressed
        assert self.data[lo:lo + size] == ser(P)
        return self.data[:lo] + ser(Pm) + self.data[lo + size:]


@pytest.fixture(scope="module")
def key(ctx):
    k = KeyCase(ctx)
    yield k
    k.pk.free()
    k.dr.free()


PARTS = api.ProvingKey.SUBGROUP_PARTS


def test_a_clean_loaded_key_is_reported_clean(ctx, key):
    """The check is a report: it leaves a loaded key unmarked (zk_pk_points_in_subgroup says which keys take the endomorphism in the
    proof tail: those of zk_groth16_setup) and the key serialises to the bytes it was loaded from."""
    clean = {name: (0, None) for name in PARTS}
    assert key.pk.points_in_subgroup                          # from zk_groth16_setup
    assert key.pk.check_subgroups() == clean and key.pk.points_in_subgroup
    pk, _, _ = S.proving_key_from_bytes(ctx, key.data)
    assert not pk.points_in_subgroup
    assert pk.check_subgroups() == clean
    assert not pk.points_in_subgroup
    assert S.proving_key_bytes(ctx, pk, False) == key.data
    pk.free()
    for compressed in (False, True):
        data = S.proving_key_bytes(ctx, key.pk, compressed)
        pk, _, _ = S.proving_key_from_bytes(ctx, data, compressed, check_subgroup=True)
        assert not pk.points_in_subgroup
        assert S.proving_key_bytes(ctx, pk, compressed) == data
        pk.free()


@pytest.mark.parametrize("name,index", [("h_query", 5), ("b_g2_query", 11), ("a_query", 63), ("l_query", 0), ("b_g1_query", 64)])
def test_a_key_with_a_point_outside_is_reported_and_left_alone(ctx, key, name, index):
    """The report names the part and the index, the key is not marked and serialises to the bytes it was loaded from."""
    data = key.moved(name, index)
    pk, _, _ = S.proving_key_from_bytes(ctx, data)
    want = {part: (0, None) for part in PARTS}
    want[name] = (1, index)
    assert pk.check_subgroups() == want
    assert not pk.points_in_subgroup
    assert pk.check_subgroups() == want and not pk.points_in_subgroup
    assert S.proving_key_bytes(ctx, pk, False) == data
    pk.free()
    h = C.c_void_p()
    assert ctx.lib.zk_pk_deserialize_checked(ctx.h, data, len(data), 0, C.byref(h)) == -2 and not h.value
    with pytest.raises(Z.ZkError, match=r"error -2: .*%s: point %d is not in the prime-order subgroup" % (name, index)):
        S.proving_key_from_bytes(ctx, data, check_subgroup=True)


def test_a_single_point_outside_is_reported(ctx, key):
    """delta_g1 sits behind the Vec gamma_abc_g1, after beta_g1"""
    at, n, size = key.off["gamma_abc_g1"]
    lo = at + n * size + 96
    (P,) = cv.g1_array_to_affine(key.pk.vk_g1(2).reshape(1, 12))
    assert key.data[lo:lo + 96] == O.g1_serialize_uncompressed(P)
    data = key.data[:lo] + O.g1_serialize_uncompressed(O.g1_add(P, cofactor_torsion_point())) + key.data[lo + 96:]
    pk, _, _ = S.proving_key_from_bytes(ctx, data)
    rep = pk.check_subgroups()
    assert rep["single_points"] == (1, 2) and all(rep[p] == (0, None) for p in PARTS[:-1])
    assert not pk.points_in_subgroup
    pk.free()
    with pytest.raises(Z.ZkError, match="error -2: .*single points: point 2"):
        S.proving_key_from_bytes(ctx, data, check_subgroup=True)


# ---- verification ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def verifier(ctx):
    """The D = 8 key of tests/golden/groth16.json made resident from the oracle's bytes, with two accepted proofs from the oracle's
    known-trapdoor prediction (the golden one and one with other r, s)."""
    j = golden("groth16.json")["mul_chain_5"]
    r1cs, td = r1cs_from_json(j), trapdoor_from_json(j["trapdoor"])
    scal = O.ProvingKeyScalars(r1cs, td)
    pk, _, _ = S.proving_key_from_bytes(ctx, O.pk_serialize(O.ProvingKey(scal), False), check_subgroup=True)
    z = [ih(v) for v in j["z"]]
    rng = O.Prng(0x5B67)
    pts = [O.predict_proof(r1cs, scal, z, ih(j["r"]), ih(j["s"])), O.predict_proof(r1cs, scal, z, rng.fr(), rng.fr())]
    assert O.proof_serialize(*pts[0]) == bytes.fromhex(j["proof"])
    yield pk, pts, cv.fr_to_mont(z[1:j["num_instance"]])
    pk.free()


def test_checked_verification_rejects_torsion_the_pairing_cannot_see(ctx, verifier):
    pk, ((A0, B0, C0), (A1, B1, C1)), inputs = verifier
    T, T2 = cofactor_torsion_point(), sc.g2_cofactor_torsion_point()
    good = [O.proof_serialize(A0, B0, C0), O.proof_serialize(A1, B1, C1)]
    a_moved = O.proof_serialize(O.g1_add(A0, T), B0, C0)
    c_moved = O.proof_serialize(A1, B1, O.g1_add(C1, T))
    b_moved = O.proof_serialize(A0, O.g2_add(B0, T2), C0)
    data = [good[0], a_moved, good[1], c_moved, good[0], good[1], b_moved, good[1]]
    inp = np.stack([inputs] * 8)
    assert list(ctx.groth16_verify_batch(pk, inp, data, check_subgroup=True)) == [1, 0, 1, 0, 1, 1, 0, 1]
    plain = list(ctx.groth16_verify_batch(pk, inp, data))
    assert plain[:6] == [1, 1, 1, 1, 1, 1] and plain[7] == 1      # (B + T2 unchecked: not pinned)
    assert ctx.groth16_verify(pk, inputs, a_moved) is True and ctx.groth16_verify(pk, inputs, a_moved, check_subgroup=True) is False
    # the host form on the same proofs
    assert pk.verify_host(inputs, a_moved) is True and pk.verify_host(inputs, a_moved, check_subgroup=True) is False
    assert pk.verify_host(inputs, c_moved, check_subgroup=True) is False and pk.verify_host(inputs, b_moved, check_subgroup=True) is False
    assert pk.verify_host(inputs, good[0], check_subgroup=True) is True
    # a tampered proof (a wrong public input) is 0 in both forms, and so are bytes that are no curve point; neighbours are undisturbed
    wrong = inputs.copy()
    wrong[0] = cv.fr_to_mont([12345])[0]
    two = np.stack([wrong, inputs])
    assert list(ctx.groth16_verify_batch(pk, two, [good[0], good[1]])) == [0, 1]
    assert list(ctx.groth16_verify_batch(pk, two, [good[0], good[1]], check_subgroup=True)) == [0, 1]
    x = 5
    while pow((x ** 3 + 1) % O.Q_MOD, (O.Q_MOD - 1) // 2, O.Q_MOD) == 1:
        x += 1
    off = x.to_bytes(48, "little") + good[0][48:]
    both = np.stack([inputs, inputs])
    assert list(ctx.groth16_verify_batch(pk, both, [off, good[0]], check_subgroup=True)) == [0, 1]


# ---- argument errors -------------------------------------------------------------------------------------------------------------------
def test_argument_errors(ctx, key, verifier):
    lib = ctx.lib
    b = ctx.bases_upload(sc.abi_array(1, _clean(1)[:5]), 1)
    n_out, first = C.c_size_t(), C.c_size_t()
    args = (None, C.byref(n_out), C.byref(first))
    assert lib.zk_bases_subgroup_check(None, b.h, 0, 5, *args) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, None, 0, 5, *args) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, b.h, 0, 5, None, None, C.byref(first)) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, b.h, 0, 5, None, C.byref(n_out), None) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, b.h, 3, 3, *args) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, b.h, 6, 0, *args) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, b.h, 2, 2 ** 64 - 1, *args) == -2
    assert lib.zk_bases_subgroup_check(ctx.h, b.h, 0, 5, *args) == 0 and n_out.value == 0
    b.free()
    out = C.c_void_p()
    one = O.g1_serialize(O.G1_GEN)
    assert lib.zk_bases_deserialize_checked(None, 1, one, 1, 1, C.byref(out)) == -2
    assert lib.zk_bases_deserialize_checked(ctx.h, 3, one, 1, 1, C.byref(out)) == -2
    assert lib.zk_bases_deserialize_checked(ctx.h, 1, None, 1, 1, C.byref(out)) == -2
    assert lib.zk_bases_deserialize_checked(ctx.h, 1, one, 1, 1, None) == -2
    rep = Z._lib.PkSubgroupReport()
    assert lib.zk_pk_check_subgroups(None, key.pk.h, C.byref(rep)) == -2
    assert lib.zk_pk_check_subgroups(ctx.h, None, C.byref(rep)) == -2
    assert lib.zk_pk_check_subgroups(ctx.h, key.pk.h, None) == -2
    assert lib.zk_pk_points_in_subgroup(None) == 0
    assert lib.zk_pk_deserialize_checked(ctx.h, None, 10, 0, C.byref(out)) == -2
    assert lib.zk_pk_deserialize_checked(ctx.h, key.data, len(key.data), 0, None) == -2
    vpk, _, vin = verifier
    proofs = np.frombuffer(bytes(192), np.uint8)
    inp = np.zeros((max(len(vin), 1), 4), np.uint64)
    ni = len(vin)
    ok = np.zeros(1, np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.zk_groth16_verify_batch_checked(ctx.h, vpk.h, 0, p(inp), ni, p(proofs), p(ok)) == -2
    assert lib.zk_groth16_verify_batch_checked(ctx.h, None, 1, p(inp), ni, p(proofs), p(ok)) == -2
    assert lib.zk_groth16_verify_batch_checked(ctx.h, vpk.h, 1, p(inp), ni, None, p(ok)) == -2
    assert lib.zk_groth16_verify_batch_checked(ctx.h, vpk.h, 1, p(inp), ni, p(proofs), None) == -2
    assert lib.zk_groth16_verify_batch_checked(ctx.h, vpk.h, 1, p(inp), ni + 1, p(proofs), p(ok)) == -2
    assert lib.zk_groth16_verify_batch_checked(ctx.h, vpk.h, 1, p(inp), ni, p(proofs), p(ok)) == 0 and ok[0] == 0
    assert lib.zk_groth16_verify_host_checked(None, p(inp), 1, p(proofs), p(ok)) == -2
