"""GPU: zk_pk_derive_eval_h -- the tables of H over coset values for a key that was LOADED, from the key's own points (a transform
over G1 points and the transposed product with C).  Two points equal as group elements have the same canonical words, so the
derived tables must equal word for word the tables zk_groth16_setup makes from the trapdoor, and the proofs of the loaded key must
equal the setup key's and the oracle's known-trapdoor prediction.  A key with a point outside the prime-order subgroup fails the
call's self-check and keeps the old path with the old bytes."""
import hashlib

import numpy as np
import pytest

import zkref as O
import zkref_c as OC
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from helpers import circuit_system, csr, mont1

pytestmark = pytest.mark.gpu

P = O.R_MOD
# mul-chains filling their domain, the circuit-shaped system of tests/test_gpu_eval_h.py at 2^7, and a system of 200 rows (D = 2^8)
# in which every row of C has a term in column 0 (the constant) and in column 1 (an instance column): two columns of 200 terms, more
# than one segment of the linear-combination kernel takes
CASES = {"mul3": 3, "mul6": 6, "mul10": 10, "synth7": (110, 7, 3), "wide8": "wide"}


def _sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


def _dot(row, z):
    return sum(c * z[j] for c, j in row) % P


def _wide_system(nc, n_pub, n_free, seed):
    """tests/test_eval_h_model.py::_system: rows <A_i, z> <B_i, z> = c0 o_i + c1 * 1 + c2 * p_1 + c3 * (an earlier variable), solved
    in order for the new witness o_i"""
    rng = O.Prng(seed)
    nv = 1 + n_pub + n_free
    a_rows, b_rows, c_rows = [], [], []
    for i in range(nc):
        a_rows.append([(rng.fr(), rng.fr() % nv) for _ in range(3)])
        b_rows.append([(rng.fr(), rng.fr() % nv) for _ in range(2)])
        c_rows.append([(2 + rng.fr() % 5, nv), (rng.fr(), 0), (rng.fr(), 1), (rng.fr(), rng.fr() % nv)])
        nv += 1
    ni = 1 + n_pub
    return O.R1CS(ni, nv - ni, a_rows, b_rows, c_rows)


def _wide_assignment(r1cs, n_head, rng):
    z = [1] + [rng.fr() for _ in range(n_head - 1)]
    for i in range(len(r1cs.c)):
        (c0, j), rest = r1cs.c[i][0], r1cs.c[i][1:]
        assert j == len(z)
        z.append((_dot(r1cs.a[i], z) * _dot(r1cs.b[i], z) - _dot(rest, z)) * pow(c0, -1, P) % P)
    return z


def _other_assignment(r1cs, z0, rng):
    """another satisfying assignment of a circuit-shaped system: every output wire solved from its row (tools/synth_r1cs.py)"""
    first_out = len(z0) - len(r1cs.c)
    z = [1] + [rng.fr() for _ in range(first_out - 1)]
    for i in range(len(r1cs.c)):
        c0, j = r1cs.c[i][-1]
        assert j == first_out + i
        z.append((_dot(r1cs.a[i], z) * _dot(r1cs.b[i], z) - _dot(r1cs.c[i][:-1], z)) * pow(c0, -1, P) % P)
    return z


def _satisfies(r1cs, z):
    return all(_dot(r1cs.a[i], z) * _dot(r1cs.b[i], z) % P == _dot(r1cs.c[i], z) for i in range(len(r1cs.c)))


def _prove_all(ctx, pk, dr, zs, rs):
    out = []
    for z, (r, s) in zip(zs, rs):
        dz = ctx.upload(z)
        out.append(ctx.create_proof_dev(pk, dr, dz.ptr, r, s))
        dz.free()
    return out


def _upload_key(ctx, pk, h_query=None):
    """a second resident key from the queries of `pk` (zk_pk_upload)"""
    return ctx.pk_upload(pk.vk_g1(0), pk.vk_g1(1), pk.vk_g1(2), pk.vk_g2(0), pk.vk_g2(1), pk.download("a_query"), pk.download("b_g1_query"),
                         pk.download("b_g2_query"), pk.download("h_query") if h_query is None else h_query, pk.download("l_query"))


class Case:
    """One system with its setup key (the reference: tables from the trapdoor), three assignments (two satisfying, one not) and their
    (r, s); everything from seeds."""

    def __init__(self, ctx, name):
        spec = CASES[name]
        rng = O.Prng(0xDE71 + sum(name.encode()))
        self.td = cv.fr_to_mont([rng.fr() for _ in range(7)])
        if isinstance(spec, int):
            n = (1 << spec) - 2
            self.dr = ctx.r1cs_mul_chain(n)
            self.cr = OC.R1cs(2, n + 1, *OC.mul_chain_csr(n))
            self.log_d = spec
            zs = []
            for _ in range(2):
                dz = ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr()))
                zs.append(ctx.download(dz, (n + 3, 4)))
                dz.free()
        else:
            if spec == "wide":
                r1cs = _wide_system(200, 2, 3, 808)
                z0, z1 = _wide_assignment(r1cs, 6, rng), _wide_assignment(r1cs, 6, rng)
                self.log_d = 8
                for col in (0, 1):                                      # the chunked product runs
                    assert sum(1 for row in r1cs.c for _, k in row if k == col) > 64
            else:
                r1cs, z0 = circuit_system(spec, 77)
                z1 = _other_assignment(r1cs, z0, rng)
                self.log_d = 7
            assert _satisfies(r1cs, z0) and _satisfies(r1cs, z1) and z0 != z1
            a, b, c = csr(r1cs.a), csr(r1cs.b), csr(r1cs.c)
            self.dr = ctx.r1cs_upload(r1cs.num_instance, r1cs.num_witness, a, b, c)
            self.cr = OC.R1cs(r1cs.num_instance, r1cs.num_witness, a, b, c)
            zs = [cv.fr_to_mont(z0), cv.fr_to_mont(z1)]
        assert self.dr.domain_log == self.log_d
        bad = zs[0].copy()                                              # satisfies nothing from the changed wire on
        bad[len(bad) // 2] = mont1(rng.fr())
        bad[-1] = mont1(rng.fr())
        self.zs = zs + [bad]
        self.rs = [(mont1(rng.fr()), mont1(rng.fr())) for _ in range(3)]
        self.pk = ctx.groth16_setup(self.dr, *self.td)
        assert self.pk.eval_h(self.dr)
        self.want = _prove_all(ctx, self.pk, self.dr, self.zs, self.rs)
        self.tables = {t: self.pk.download_eval(t) for t in ("h_eval", "l_eval_pad", "l_eval_0")}
        self.loaded = None

    def loaded_keys(self, ctx):
        """the key read back from its bytes and the key uploaded from its queries, both derived for (once per session)"""
        if self.loaded is None:
            k1, _, _ = S.proving_key_from_bytes(ctx, S.proving_key_bytes(ctx, self.pk, False), compressed=False)
            k2 = _upload_key(ctx, self.pk)
            self.before = []
            for k in (k1, k2):
                assert not k.eval_h(self.dr)
                self.before.append((_sha(k.download("h_query")), _sha(k.download("l_query"))))
                k.derive_eval_h(self.dr)
            self.loaded = [k1, k2]
        return self.loaded


_CASES = {}


@pytest.fixture
def case(ctx, request):
    name = request.param
    if name not in _CASES:
        _CASES[name] = Case(ctx, name)
    return _CASES[name]


@pytest.mark.parametrize("case", list(CASES), indirect=True)
def test_derived_tables_are_the_setup_keys_tables(ctx, case):
    c = case
    for k, before in zip(c.loaded_keys(ctx), c.before):
        assert k.eval_h(c.dr)
        for t in ("h_eval", "l_eval_pad", "l_eval_0"):
            got = k.download_eval(t)
            assert got.shape == c.tables[t].shape and np.array_equal(got, c.tables[t]), t
        assert c.tables["h_eval"].shape[0] == 1 << c.log_d and np.array_equal(c.tables["l_eval_0"][0], c.tables["l_eval_pad"][0])
        # a second call does nothing, and the key's own queries are what they were
        k.derive_eval_h(c.dr)
        assert k.eval_h(c.dr)
        assert (_sha(k.download("h_query")), _sha(k.download("l_query"))) == before
        assert before == (_sha(c.pk.download("h_query")), _sha(c.pk.download("l_query")))


@pytest.mark.parametrize("case", list(CASES), indirect=True)
def test_proofs_of_the_derived_key_are_the_setup_keys_and_the_predicted(ctx, case):
    c = case
    assert len(set(c.want)) == 3
    assert c.want == [OC.groth16_predict(c.cr, c.td, z, OC.witness_map(c.cr, z), r, s) for z, (r, s) in zip(c.zs, c.rs)]
    for k in c.loaded_keys(ctx):
        assert _prove_all(ctx, k, c.dr, c.zs, c.rs) == c.want


@pytest.mark.parametrize("case", ["mul10"], indirect=True)
def test_batch_and_queue_of_a_derived_key(ctx, case):
    c = case
    k = c.loaded_keys(ctx)[0]
    dz = ctx.upload(np.concatenate(c.zs))
    assert ctx.create_proofs_batch_dev(k, c.dr, dz.ptr, 3, [r for r, _ in c.rs], [s for _, s in c.rs]) == c.want
    dz.free()
    z = [np.ascontiguousarray(c.zs[0]), np.ascontiguousarray(c.zs[1])]
    got = [ctx.create_proof_queued(k, c.dr, z[i & 1], *c.rs[i & 1], z[(i + 1) & 1]) for i in range(3)]
    got.append(ctx.create_proof_queued(k, c.dr, z[1], *c.rs[1]))
    assert got == [c.want[0], c.want[1]] * 2


@pytest.mark.parametrize("case", ["mul6"], indirect=True)
def test_a_key_with_a_point_outside_the_subgroup_is_refused_and_left_alone(ctx, case):
    import marlin_verify_cases as MC
    c = case
    h = c.pk.download("h_query")
    moved = O.g1_add(cv.g1_array_to_affine(h[5:6])[0], MC.cofactor_torsion_point())
    h[5] = cv.g1_affine_to_array([moved])[0]
    k = _upload_key(ctx, c.pk, h_query=h)
    assert not k.eval_h(c.dr)
    before = _prove_all(ctx, k, c.dr, c.zs, c.rs)
    assert before != c.want
    with pytest.raises(Z.ZkError, match=r"error -2: .*h_query / l_query do not satisfy the identity"):
        k.derive_eval_h(c.dr)
    assert not k.eval_h(c.dr)
    with pytest.raises(Z.ZkError, match="error -2"):
        k.download_eval("h_eval")
    assert _sha(k.download("h_query")) == _sha(h)
    assert _prove_all(ctx, k, c.dr, c.zs, c.rs) == before
    k.free()


@pytest.mark.parametrize("case", ["mul6"], indirect=True)
def test_argument_errors(ctx, case):
    c = case
    k = _upload_key(ctx, c.pk)
    other = ctx.r1cs_mul_chain((1 << 3) - 2)                            # a system of another size
    with pytest.raises(Z.ZkError, match="error -2"):
        k.derive_eval_h(other)
    assert ctx.lib.zk_pk_derive_eval_h(ctx.h, None, c.dr.h) == -2 and ctx.lib.zk_pk_derive_eval_h(ctx.h, k.h, None) == -2
    assert ctx.lib.zk_pk_derive_eval_h(None, k.h, c.dr.h) == -2
    short = _upload_key(ctx, c.pk, h_query=c.pk.download("h_query")[:-1])        # h_query of D - 2 points
    with pytest.raises(Z.ZkError, match="error -2"):
        short.derive_eval_h(c.dr)
    assert not k.eval_h(c.dr) and not short.eval_h(c.dr)
    k.derive_eval_h(c.dr)                                               # the refusals left the key usable
    assert k.eval_h(c.dr)
    other.free(); k.free(); short.free()
