"""H over coset values (zk_pk::h_eval / l_eval_pad): a key made by zk_groth16_setup proves with a witness map that stops at
a o b on the coset.  For every key here three sets of proof bytes must be equal: the new path, the old path (ZK_G16_EVAL_H=0, which
only a fresh process can have: ONE child proves every case of this module and also hashes its keys' h_query / l_query), and the
oracle's known-trapdoor prediction.  Each case has two satisfying assignments and one that satisfies nothing: the identity is linear
in the assignment and holds for all three.

Run as a program (the child): prints one JSON object {case: {"proofs": [hex..], "h_query": sha, "l_query": sha}}."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (_root, os.path.join(_root, "oracle"), os.path.join(_root, "tests"), os.path.join(_root, "tools")):
        sys.path.insert(0, _p)

import zkref as O
import zkref_c as OC
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from helpers import circuit_system, csr, mont1

pytestmark = pytest.mark.gpu

# mul-chains filling their domain (2^3 is the domain of the smallest circuit the suite proves), and one circuit-shaped system at 2^7:
# 110 rows, 7 public inputs, non-unit coefficients, several terms per row -- C touches the constant's and the instance columns
CASES = {"mul3": 3, "mul6": 6, "mul10": 10, "synth7": (110, 7, 3)}


def _sha(arr):
    return hashlib.sha256(np.ascontiguousarray(arr).tobytes()).hexdigest()


class Case:
    """One key with three assignments (host arrays, Montgomery form) and their (r, s); everything from seeds, the same in the child."""

    def __init__(self, ctx, name):
        spec = CASES[name]
        rng = O.Prng(0xE7A1 + sum(name.encode()))
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
            r1cs, z0 = circuit_system(spec, 77)
            a, b, c = csr(r1cs.a), csr(r1cs.b), csr(r1cs.c)
            assert any(k == 0 for row in r1cs.c for _, k in row) and any(1 <= k < r1cs.num_instance for row in r1cs.c for _, k in row)
            self.dr = ctx.r1cs_upload(r1cs.num_instance, r1cs.num_witness, a, b, c)
            self.cr = OC.R1cs(r1cs.num_instance, r1cs.num_witness, a, b, c)
            self.log_d = 7
            zs = [cv.fr_to_mont(z0), cv.fr_to_mont(_other_assignment(r1cs, z0, rng))]
        assert self.dr.domain_log == self.log_d
        bad = zs[0].copy()                                              # satisfies nothing from the changed wire on
        bad[len(bad) // 2] = mont1(rng.fr())
        bad[-1] = mont1(rng.fr())
        self.zs = zs + [bad]
        self.rs = [(mont1(rng.fr()), mont1(rng.fr())) for _ in range(3)]
        self.pk = ctx.groth16_setup(self.dr, *self.td)

    def prove_all(self, ctx):
        out = []
        for z, (r, s) in zip(self.zs, self.rs):
            dz = ctx.upload(z)
            out.append(ctx.create_proof_dev(self.pk, self.dr, dz.ptr, r, s))
            dz.free()
        return out

    def predicted(self):
        return [OC.groth16_predict(self.cr, self.td, z, OC.witness_map(self.cr, z), r, s) for z, (r, s) in zip(self.zs, self.rs)]


def _other_assignment(r1cs, z0, rng):
    """another satisfying assignment of a circuit-shaped system: every output wire solved from its row (tools/synth_r1cs.py)"""
    first_out = len(z0) - len(r1cs.c)
    z = [1] + [rng.fr() for _ in range(first_out - 1)]
    for i in range(len(r1cs.c)):
        dot = lambda row: sum(c * z[j] for c, j in row) % O.R_MOD
        c0, j = r1cs.c[i][-1]
        assert j == first_out + i
        z.append((dot(r1cs.a[i]) * dot(r1cs.b[i]) - dot(r1cs.c[i][:-1])) * pow(c0, -1, O.R_MOD) % O.R_MOD)
    return z


def _child_main():
    import zk_mpc_amd as Z
    assert os.environ.get("ZK_G16_EVAL_H") == "0"
    ctx = Z.Context(0)
    out = {}
    try:
        for name in CASES:
            c = Case(ctx, name)
            assert not c.pk.eval_h(c.dr)
            out[name] = {"proofs": [p.hex() for p in c.prove_all(ctx)], "h_query": _sha(c.pk.download("h_query")),
                         "l_query": _sha(c.pk.download("l_query"))}
            c.pk.free(); c.dr.free()
    finally:
        ctx.close()
    print("EVAL_H_CHILD " + json.dumps(out))


@pytest.fixture(scope="module")
def old_path():
    """what a process with ZK_G16_EVAL_H=0 proves and holds for every case"""
    env = dict(os.environ, ZK_G16_EVAL_H="0")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("EVAL_H_CHILD ")][-1]
    return json.loads(line[len("EVAL_H_CHILD "):])


_CASES = {}


@pytest.fixture
def case(ctx, request):
    name = request.param
    if name not in _CASES:
        assert os.environ.get("ZK_G16_EVAL_H", "1") != "0", "this module tests the default path"
        _CASES[name] = Case(ctx, name)
        _CASES[name].new = _CASES[name].prove_all(ctx)
    return name, _CASES[name]


@pytest.mark.parametrize("case", list(CASES), indirect=True)
def test_new_path_old_path_and_prediction_agree(ctx, case, old_path):
    name, c = case
    assert c.pk.eval_h(c.dr)
    assert len(set(c.new)) == 3
    assert c.new == [bytes.fromhex(p) for p in old_path[name]["proofs"]]
    assert c.new == c.predicted()
    # h_query and l_query are what a key without the new tables holds
    assert c.pk.query_len("h_query") == (1 << c.log_d) - 1
    assert _sha(c.pk.download("h_query")) == old_path[name]["h_query"]
    assert _sha(c.pk.download("l_query")) == old_path[name]["l_query"]


@pytest.mark.parametrize("case", ["mul6"], indirect=True)
def test_batch_of_three(ctx, case, old_path):
    name, c = case
    dz = ctx.upload(np.concatenate(c.zs))
    got = ctx.create_proofs_batch_dev(c.pk, c.dr, dz.ptr, 3, [r for r, _ in c.rs], [s for _, s in c.rs])
    dz.free()
    assert got == c.new == [bytes.fromhex(p) for p in old_path[name]["proofs"]]


@pytest.mark.parametrize("case", ["mul10"], indirect=True)
def test_two_contexts_of_one_device(ctx, case):
    import zk_mpc_amd as Z
    name, c = case
    other = Z.Context(0)
    try:
        dr2 = other.r1cs_mul_chain((1 << 10) - 2)
        pk2 = other.groth16_setup(dr2, *c.td)
        dz = ctx.upload(c.zs[0])
        assert ctx.create_proof_multi([other], [c.pk, pk2], [c.dr, dr2], dz.ptr, *c.rs[0]) == c.new[0]
        assert ctx.create_proof_dev(c.pk, c.dr, dz.ptr, *c.rs[0]) == c.new[0]
        dz.free(); pk2.free(); dr2.free()
    finally:
        other.close()


@pytest.mark.parametrize("case", ["mul10"], indirect=True)
def test_queue_with_an_announced_next_proof(ctx, case):
    """the front of an announced proof (its witness map and H sort enqueued behind the current proof) reads the jobs table too"""
    name, c = case
    z = [np.ascontiguousarray(c.zs[0]), np.ascontiguousarray(c.zs[1])]
    got = [ctx.create_proof_queued(c.pk, c.dr, z[k & 1], *c.rs[k & 1], z[(k + 1) & 1]) for k in range(5)]
    got.append(ctx.create_proof_queued(c.pk, c.dr, z[1], *c.rs[1]))
    assert got == [c.new[0], c.new[1]] * 3
    dz = [ctx.upload(v) for v in z]
    got = []
    for k in range(4):
        ctx.groth16_hint_next_dev(dz[(k + 1) & 1].ptr)
        got.append(ctx.create_proof_dev(c.pk, c.dr, dz[k & 1].ptr, *c.rs[k & 1]))
    ctx.groth16_hint_next_dev(None)
    assert got == [c.new[0], c.new[1]] * 2
    for d in dz:
        d.free()


@pytest.mark.parametrize("case", ["synth7"], indirect=True)
def test_a_key_read_back_from_its_bytes_takes_the_old_path(ctx, case):
    """the wire format has no place for the new tables: a deserialised key proves over h_query / l_query, to the same bytes"""
    name, c = case
    pk2, _, _ = S.proving_key_from_bytes(ctx, S.proving_key_bytes(ctx, c.pk, False), compressed=False)
    assert not pk2.eval_h(c.dr)
    dz = ctx.upload(c.zs[2])
    assert ctx.create_proof_dev(pk2, c.dr, dz.ptr, *c.rs[2]) == c.new[2]
    dz.free(); pk2.free()


if __name__ == "__main__":
    _child_main()
