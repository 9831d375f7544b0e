"""Work started ahead of a proof and left pending on the context (groth16_pipeline.hip): a presort, a begun set, the front of an
announced proof and a chained front, each followed by every entry point that may find it there.  Whatever the next call is, its
bytes or sums equal those of a context that never had anything pending.  One small key (mul-chain, n = 1000, D = 2^10: the
grouped path; test_gpu_groth16.py has the large path and the plain tables)."""
import numpy as np
import pytest

import zkref as O
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv

pytestmark = pytest.mark.gpu

N = 1000
D = 1 << 10
M = N + 3
KINDS = ["presort", "begun", "front", "chained_front"]
CONSUMERS = ["prove_same_z", "prove_other_z", "msms_same_z", "msms_other_z", "msms_begin", "prove_batch", "msm_batch", "free_key"]


def _inputs():
    rng = O.Prng(0xF11647)
    mont = lambda v: cv.fr_to_mont([v])[0]
    td = [mont(rng.fr()) for _ in range(7)]
    ws = [(mont(rng.fr()), mont(rng.fr())) for _ in range(3)]          # a: pending, b: the proof that carries a's front, c: another
    rs = [(mont(rng.fr()), mont(rng.fr())) for _ in range(3)]
    return td, ws, rs


class _World:
    """One context with the key, the three assignments, their quotients and the two-assignment buffer of the batch."""

    def __init__(self, ctx):
        self.ctx = ctx
        self.td, ws, self.rs = _inputs()
        self.dr = ctx.r1cs_mul_chain(N)
        self.pk = ctx.groth16_setup(self.dr, *self.td)
        self.z = [ctx.mul_chain_assignment_dev(N, *w) for w in ws]
        self.h = [ctx.alloc(D * 32) for _ in range(3)]
        for z, h in zip(self.z, self.h):
            ctx.witness_map_dev(self.dr, z.ptr, h.ptr)
        self.z_ac = ctx.upload(np.concatenate([ctx.download(self.z[0], (M, 4)), ctx.download(self.z[2], (M, 4))]))

    def prove(self, k):
        return self.ctx.create_proof_dev(self.pk, self.dr, self.z[k].ptr, *self.rs[k])

    def msms(self, k):
        g1, g2 = self.ctx.groth16_msms_dev(self.pk, self.dr, self.z[k].ptr, self.h[k].ptr)
        return g1.tobytes() + g2.tobytes()

    def prove_batch(self):
        return self.ctx.create_proofs_batch_dev(self.pk, self.dr, self.z_ac.ptr, 2, [self.rs[0][0], self.rs[2][0]], [self.rs[0][1], self.rs[2][1]])

    def msm_batch(self):
        jobs = [(self.pk.query_bases(q), 1, self.z[0].ptr + 32, M - 1) for q in ("a_query", "b_g2_query", "b_g1_query")]
        jobs.append((self.pk.query_bases("h_query"), 0, self.h[2].ptr, D - 1))
        return [o.tobytes() for o in self.ctx.msm_batch_dev(jobs)]


@pytest.fixture(scope="module")
def want():
    """The results of a context that never has anything pending."""
    c = Z.Context(0)
    try:
        w = _World(c)
        out = {"prove": [w.prove(k) for k in range(3)], "msms": [w.msms(k) for k in (0, 1, 2)], "prove_batch": w.prove_batch(),
               "msm_batch": w.msm_batch()}
        w.pk.free()
    finally:
        c.close()
    assert len(set(out["prove"])) == 3 and len(set(out["msms"])) == 3
    assert out["prove_batch"] == [out["prove"][0], out["prove"][2]]
    return out


@pytest.fixture(scope="module")
def world(ctx):
    w = _World(ctx)
    yield w
    ctx.groth16_chain_fronts(True)
    ctx.groth16_hint_next_dev(None)
    if w.pk.h:
        w.pk.free()


def leave_pending(w, kind, want):
    ctx = w.ctx
    if kind == "presort":
        ctx.groth16_msms_presort_dev(w.pk, w.dr, w.z[0].ptr)
    elif kind == "begun":
        ctx.groth16_msms_begin_dev(w.pk, w.dr, w.z[0].ptr)
    else:
        ctx.groth16_chain_fronts(kind == "chained_front")
        ctx.groth16_hint_next_dev(w.z[0].ptr)
        assert w.prove(1) == want["prove"][1]          # leaves the front of z[0] behind


@pytest.mark.parametrize("consumer", CONSUMERS)
@pytest.mark.parametrize("kind", KINDS)
def test_pending_flight_then_consumer(world, want, kind, consumer):
    w = world
    leave_pending(w, kind, want)
    if consumer == "prove_same_z":
        assert w.prove(0) == want["prove"][0]
    elif consumer == "prove_other_z":
        assert w.prove(2) == want["prove"][2]
    elif consumer == "msms_same_z":
        assert w.msms(0) == want["msms"][0]
    elif consumer == "msms_other_z":
        assert w.msms(2) == want["msms"][2]
    elif consumer == "msms_begin":
        w.ctx.groth16_msms_begin_dev(w.pk, w.dr, w.z[0].ptr)
        assert w.msms(0) == want["msms"][0]
    elif consumer == "prove_batch":
        assert w.prove_batch() == want["prove_batch"]
    elif consumer == "msm_batch":
        assert w.msm_batch() == want["msm_batch"]
    else:
        w.pk.free()                                     # the pending work points into the key: it goes with it
        w.pk = w.ctx.groth16_setup(w.dr, *w.td)
        assert w.prove(0) == want["prove"][0]
    # and the context is as good as new afterwards
    assert w.prove(2) == want["prove"][2]
    assert w.msms(0) == want["msms"][0]
