"""zk_groth16_prove_batch_dev / zk_groth16_prove_batch: count proofs of one key in one call.  Every proof must be the bytes
create_proof_dev gives for the same (z, r, s) -- and, on a small circuit-shaped system, the oracle's prediction."""
import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.serialize as S
from zk_mpc_amd._lib import ZkError
from helpers import circuit_system, csr, mont1, td_mont

pytestmark = pytest.mark.gpu

_KEYS = {}


def mul_chain_key(ctx, log_n):
    if log_n not in _KEYS:
        rng = O.Prng(5150 + log_n)
        n = (1 << log_n) - 4
        dr = ctx.r1cs_mul_chain(n)
        pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])
        _KEYS[log_n] = (n, dr, pk)
    return _KEYS[log_n]


def assignments(ctx, n, count, rng, same=False):
    """count mul-chain assignments, downloaded and laid back to back; also the single buffers"""
    m = n + 3
    singles = []
    for k in range(count):
        if same and k:
            singles.append(singles[0])
            continue
        singles.append(ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr())))
    host = np.concatenate([ctx.download(z, (m, 4)) for z in singles])
    return host, ctx.upload(host), singles


def rs_lists(rng, count):
    return [mont1(rng.fr()) for _ in range(count)], [mont1(rng.fr()) for _ in range(count)]


@pytest.mark.parametrize("log_n,count", [(10, 64), (12, 64), (14, 16), (16, 4), (10, 2), (10, 1)])
def test_batch_matches_single_proofs(ctx, log_n, count):
    n, dr, pk = mul_chain_key(ctx, log_n)
    rng = O.Prng(77 + log_n * 100 + count)
    host, dz, singles = assignments(ctx, n, count, rng)
    rl, sl = rs_lists(rng, count)
    if count > 2:
        rl[1] = sl[1] = mont1(0)                      # r = s = 0
    got = ctx.create_proofs_batch_dev(pk, dr, dz.ptr, count, rl, sl)
    want = [ctx.create_proof_dev(pk, dr, singles[k].ptr, rl[k], sl[k]) for k in range(count)]
    assert got == want
    assert len(set(got)) == count
    if count <= 16:
        assert ctx.create_proofs_batch(pk, dr, host, rl, sl) == want        # host form
    dz.free()


def test_batch_of_identical_witnesses(ctx):
    n, dr, pk = mul_chain_key(ctx, 10)
    rng = O.Prng(4242)
    host, dz, singles = assignments(ctx, n, 9, rng, same=True)
    rl = [mont1(5)] * 9
    sl = [mont1(6)] * 9
    got = ctx.create_proofs_batch_dev(pk, dr, dz.ptr, 9, rl, sl)
    assert got == [ctx.create_proof_dev(pk, dr, singles[0].ptr, rl[0], sl[0])] * 9
    dz.free()


def other_assignment(r1cs, z0, rng):
    """another satisfying assignment of the same circuit-shaped system: new public inputs and free witnesses, then every output
    wire o_i solved from its row, whose C side ends with (c0, o_i) (tools/synth_r1cs.py)"""
    first_out = len(z0) - len(r1cs.c)
    z = [1] + [rng.fr() for _ in range(first_out - 1)]
    for i in range(len(r1cs.c)):
        dot = lambda row: sum(c * z[j] for c, j in row) % O.R_MOD
        c0, j = r1cs.c[i][-1]
        assert j == first_out + i
        z.append((dot(r1cs.a[i]) * dot(r1cs.b[i]) - dot(r1cs.c[i][:-1])) * pow(c0, -1, O.R_MOD) % O.R_MOD)
    return z


def test_batch_circuit_shaped_against_oracle(ctx):
    """non-unit coefficients, several public inputs, a different witness per proof; the oracle's prediction for every proof"""
    rng = O.Prng(9001)
    count = 5
    r1cs, z0 = circuit_system((60, 3, 2), 31)
    td = O.Trapdoor(*[rng.fr() for _ in range(7)])
    pks = O.ProvingKeyScalars(r1cs, td)
    dr = ctx.r1cs_upload(r1cs.num_instance, r1cs.num_witness, csr(r1cs.a), csr(r1cs.b), csr(r1cs.c))
    pk = ctx.groth16_setup(dr, *td_mont(td))
    zs = [z0] + [other_assignment(r1cs, z0, rng) for _ in range(count - 1)]
    assert len({tuple(z) for z in zs}) == count
    rr = [rng.fr() for _ in range(count)]
    ss = [rng.fr() for _ in range(count)]
    rr[2] = ss[2] = 0
    zm = np.concatenate([cv.fr_to_mont(z) for z in zs])
    dz = ctx.upload(zm)
    got = ctx.create_proofs_batch_dev(pk, dr, dz.ptr, count, [mont1(x) for x in rr], [mont1(x) for x in ss])
    for k in range(count):
        assert got[k] == O.proof_serialize(*O.predict_proof(r1cs, pks, zs[k], rr[k], ss[k])), k
    # a key loaded from its bytes (not known to be in the subgroup: the plain scalar multiplications of the tail)
    pk2, _, _ = S.proving_key_from_bytes(ctx, S.proving_key_bytes(ctx, pk, False), compressed=False)
    assert ctx.create_proofs_batch_dev(pk2, dr, dz.ptr, count, [mont1(x) for x in rr], [mont1(x) for x in ss]) == got
    dz.free()
    pk2.free()
    pk.free()


def test_batch_between_hinted_and_queued_proofs(ctx):
    """a single proof with an announced successor, then a batch (which drops the announcement), then single and queued proofs"""
    n, dr, pk = mul_chain_key(ctx, 12)
    rng = O.Prng(606)
    host, dz, singles = assignments(ctx, n, 4, rng)
    rl, sl = rs_lists(rng, 4)
    plain = [ctx.create_proof_dev(pk, dr, singles[k].ptr, rl[k], sl[k]) for k in range(4)]
    m = n + 3
    ctx.groth16_hint_next_dev(singles[1].ptr)
    assert ctx.create_proof_dev(pk, dr, singles[0].ptr, rl[0], sl[0]) == plain[0]
    assert ctx.create_proofs_batch_dev(pk, dr, dz.ptr, 4, rl, sl) == plain
    assert ctx.create_proof_dev(pk, dr, singles[2].ptr, rl[2], sl[2]) == plain[2]
    zh = [np.ascontiguousarray(host[k * m:(k + 1) * m]) for k in range(4)]
    assert ctx.create_proof_queued(pk, dr, zh[0], rl[0], sl[0], zh[1]) == plain[0]
    assert ctx.create_proofs_batch(pk, dr, host, rl, sl) == plain
    assert ctx.create_proof_queued(pk, dr, zh[1], rl[1], sl[1], zh[3]) == plain[1]
    assert ctx.create_proof_queued(pk, dr, zh[3], rl[3], sl[3]) == plain[3]
    ctx.groth16_hint_next_dev(singles[3].ptr)
    assert ctx.create_proof_dev(pk, dr, singles[2].ptr, rl[2], sl[2]) == plain[2]
    assert ctx.create_proof_dev(pk, dr, singles[3].ptr, rl[3], sl[3]) == plain[3]
    dz.free()


def test_batch_too_large_and_bad_arguments(ctx):
    """a batch whose working set cannot fit fails with ZK_ERR_NOMEM before any device work; the context stays usable"""
    rng = O.Prng(31337)
    n20 = (1 << 20) - 4
    dr20 = ctx.r1cs_mul_chain(n20)
    pk20 = ctx.groth16_setup(dr20, *[mont1(rng.fr()) for _ in range(7)])
    dz = ctx.upload(np.zeros((n20 + 3, 4), dtype=np.uint64))  # never read: the size check comes first
    big = 4096                                                  # 4096 proofs of 2^20 constraints: ~0.9 TB of working set
    rl = [mont1(1)] * big
    with pytest.raises(ZkError, match="error -3"):
        ctx.create_proofs_batch_dev(pk20, dr20, dz.ptr, big, rl, rl)
    with pytest.raises(ZkError, match="error -2"):
        ctx.create_proofs_batch_dev(pk20, dr20, dz.ptr, 0, [], [])
    n10, dr10, pk10 = mul_chain_key(ctx, 10)
    with pytest.raises(ZkError, match="error -2"):                # key of another system
        ctx.create_proofs_batch_dev(pk20, dr10, dz.ptr, 2, rl[:2], rl[:2])
    dz.free()
    pk20.free()
    host, dz, singles = assignments(ctx, n10, 3, rng)
    rl, sl = rs_lists(rng, 3)
    assert ctx.create_proofs_batch_dev(pk10, dr10, dz.ptr, 3, rl, sl) == \
        [ctx.create_proof_dev(pk10, dr10, singles[k].ptr, rl[k], sl[k]) for k in range(3)]
    dz.free()
