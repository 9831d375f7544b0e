"""GPU: count collaborative Groth16 proofs in one call (zk_groth16_prove_shared_batch / _spdz_batch; parties = threads on device 0
over LocalNet).  Proof k of every party is the oracle's known-trapdoor prediction for the summed inputs of k and the bytes of the
single call for the same shares; the call makes the exchanges of ONE single call and sends count times its bytes; a moved MAC share
fails every party and leaves the output alone; bad arguments come back as error codes."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import zkref as O
import zkref_c as OC
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
import pyseq.mpc_seq as mpc
from zk_mpc_amd.mpc import _fr_array
from helpers import td_mont, mont1
from oracle_backend import additive_shares

pytestmark = pytest.mark.gpu

ZK_ERR_ARG, ZK_ERR_NOMEM = -2, -3


def run_parties(n_parties, fn):
    """fn(p, ctx, net) per party, each on a thread with its own context on device 0 (as tests/test_gpu_mpc.py::run_parties)."""
    nets = mpc.LocalNet.create(n_parties)
    out, err = [None] * n_parties, []

    def work(p):
        ctx = Z.Context(0, p, n_parties)
        try:
            out[p] = fn(p, ctx, nets[p])
        except Exception as e:  # pragma: no cover
            import traceback
            err.append("party %d: %s\n%s" % (p, e, traceback.format_exc()))
            try:
                nets[p].sh.barrier.abort()
            except Exception:
                pass
        finally:
            ctx.close()

    ts = [threading.Thread(target=work, args=(p,)) for p in range(n_parties)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    assert not err, "\n".join(err)
    return out


@functools.lru_cache(maxsize=None)
def case(n_parties, n, count, spdz=False):
    """count mul-chain proofs of n constraints, each with its own w0, w1, r, s, shared among n_parties; the oracle's proofs.  Computed
    once per shape and read by every test that needs it."""
    rng = O.Prng(7000 + 131 * n + 17 * count + n_parties + (1 << 20) * int(spdz))
    td = O.Trapdoor(rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr())
    tdm = td_mont(td)
    cr = OC.R1cs(2, n + 1, *OC.mul_chain_csr(n))
    lanes = 2 if spdz else 1
    z_sh = [[[] for _ in range(n_parties)] for _ in range(lanes)]          # [lane][party] -> count * m values
    r_sh = [[[] for _ in range(n_parties)] for _ in range(lanes)]
    s_sh = [[[] for _ in range(n_parties)] for _ in range(lanes)]
    want = []
    for _ in range(count):
        _, z = O.mul_chain_r1cs(n, rng.fr(), rng.fr())
        r, s = rng.fr(), rng.fr()
        for l in range(lanes):                                             # (the MAC lane: an independent sharing of alpha * v, alpha = 1)
            zs = additive_shares(z, n_parties, rng, public_prefix=2)
            rs, ss = O.additive_share(r, n_parties, rng), O.additive_share(s, n_parties, rng)
            for p in range(n_parties):
                z_sh[l][p] += zs[p]
                r_sh[l][p].append(mont1(rs[p]))
                s_sh[l][p].append(mont1(ss[p]))
        zm = cv.fr_to_mont(z)
        want.append(OC.groth16_predict(cr, tdm, zm, OC.witness_map(cr, zm), mont1(r), mont1(s)))
    z_mont = [[cv.fr_to_mont(z_sh[l][p]) for p in range(n_parties)] for l in range(lanes)]
    return dict(tdm=tdm, m=n + 3, D=1 << cr.domain_log, z=z_mont, r=r_sh, s=s_sh, want=want)


def setup(ctx, n, tdm):
    dr = ctx.r1cs_mul_chain(n)
    return dr, ctx.groth16_setup(dr, *[tdm[i] for i in range(7)])


@pytest.mark.parametrize("n_parties,n,count", [(3, 6, 5), (2, 1000, 3), (1, 1000, 8), (8, 77, 2), (3, 1000, 1)])
def test_batch_matches_the_oracle_and_the_single_call(n_parties, n, count):
    cs = case(n_parties, n, count)
    m = cs["m"]

    def fn(p, ctx, net):
        party = mpc.Party(ctx, net=net)
        dr, pk = setup(ctx, n, cs["tdm"])
        dz = ctx.upload(cs["z"][0][p])
        batch = party.create_proofs_shared_native(pk, dr, dz.ptr, cs["r"][0][p], cs["s"][0][p])
        single = [party.create_proof_shared_native(pk, dr, dz.ptr + k * m * 32, cs["r"][0][p][k], cs["s"][0][p][k]) for k in range(count)]
        return batch, single

    for batch, single in run_parties(n_parties, fn):
        assert len(batch) == count
        for k in range(count):
            assert batch[k] == cs["want"][k], "proof %d differs from the oracle" % k
            assert batch[k] == single[k], "proof %d differs from the single call" % k


def test_batch_with_real_beaver_triples():
    n_parties, n, count = 2, 6, 4
    cs = case(n_parties, n, count)
    total = count * cs["D"]
    rng = O.Prng(7777)
    ta, tb = [rng.fr() for _ in range(total)], [rng.fr() for _ in range(total)]
    tc = [a * b % O.R_MOD for a, b in zip(ta, tb)]
    tr = [additive_shares(v, n_parties, rng) for v in (ta, tb, tc)]

    def fn(p, ctx, net):
        party = mpc.Party(ctx, net=net)
        dr, pk = setup(ctx, n, cs["tdm"])
        dz = ctx.upload(cs["z"][0][p])
        up = [ctx.upload(cv.fr_to_mont(t[p])) for t in tr]
        real = party.create_proofs_shared_native(pk, dr, dz.ptr, cs["r"][0][p], cs["s"][0][p], triple=tuple(u.ptr for u in up))
        dummy = party.create_proofs_shared_native(pk, dr, dz.ptr, cs["r"][0][p], cs["s"][0][p])
        return real, dummy

    for real, dummy in run_parties(n_parties, fn):
        assert real == cs["want"]
        assert dummy == cs["want"]


def test_batch_makes_the_exchanges_of_one_single_call():
    n_parties, n, count = 3, 6, 5
    cs = case(n_parties, n, count)

    def fn(p, ctx, net):
        party = mpc.Party(ctx, net=net)
        dr, pk = setup(ctx, n, cs["tdm"])
        dz = ctx.upload(cs["z"][0][p])
        calls = {"small": 0, "vec": 0}
        gather, open_vec = net.all_gather_small, party.be.open_vec

        def counted_gather(*a, **kw):
            calls["small"] += 1
            return gather(*a, **kw)

        def counted_open(*a, **kw):
            calls["vec"] += 1
            return open_vec(*a, **kw)
        net.all_gather_small, party.be.open_vec = counted_gather, counted_open
        sent0 = party.bytes_sent
        party.create_proof_shared_native(pk, dr, dz.ptr, cs["r"][0][p][0], cs["s"][0][p][0])
        single, single_sent = dict(calls), party.bytes_sent - sent0
        calls.update(small=0, vec=0)
        sent0 = party.bytes_sent
        proofs = party.create_proofs_shared_native(pk, dr, dz.ptr, cs["r"][0][p], cs["s"][0][p])
        return single, dict(calls), single_sent, party.bytes_sent - sent0, proofs

    for single, batch, single_sent, batch_sent, proofs in run_parties(n_parties, fn):
        assert single == {"small": 2, "vec": 2}            # (the two small opens and the two vector opens of a proof)
        assert batch == single
        assert batch_sent == count * single_sent
        assert proofs == cs["want"]


@pytest.mark.parametrize("n_parties,n,count", [(2, 100, 3), (3, 6, 2)])
def test_spdz_batch(n_parties, n, count):
    cs = case(n_parties, n, count, True)
    m = cs["m"]

    def fn(p, ctx, net):
        party = mpc.SpdzParty(ctx, net=net)
        dr, pk = setup(ctx, n, cs["tdm"])
        dzs, dzm = ctx.upload(cs["z"][0][p]), ctx.upload(cs["z"][1][p])
        rr, ss = (cs["r"][0][p], cs["r"][1][p]), (cs["s"][0][p], cs["s"][1][p])
        batch = party.create_proofs_shared_spdz_native(pk, dr, (dzs.ptr, dzm.ptr), rr, ss)
        single = [party.create_proof_shared_spdz_native(pk, dr, (dzs.ptr + k * m * 32, dzm.ptr + k * m * 32), (rr[0][k], rr[1][k]),
                                                        (ss[0][k], ss[1][k])) for k in range(count)]
        # one word flipped in the last party's MAC share of assignment 1: every party's check fails, nothing is written
        bad = cs["z"][1][p].copy()
        if p == n_parties - 1:
            bad[m + 5, 0] ^= np.uint64(1)
        dbad = ctx.upload(bad)
        out = np.full(192 * count, 0xA5, dtype=np.uint8)
        try:
            party.create_proofs_shared_spdz_native(pk, dr, (dzs.ptr, dbad.ptr), rr, ss, out=out)
            caught = False
        except mpc.MacCheckError:
            caught = True
        return batch, single, caught, bool(np.all(out == 0xA5))

    for batch, single, caught, untouched in run_parties(n_parties, fn):
        assert batch == cs["want"]
        assert batch == single
        assert caught and untouched


def test_bad_arguments_and_a_working_set_that_cannot_fit():
    n, count = 6, 2
    cs = case(1, n, count)

    def fn(p, ctx, net):
        party = mpc.Party(ctx, net=net)
        dr, pk = setup(ctx, n, cs["tdm"])
        dr_other, pk_other = setup(ctx, 77, cs["tdm"])
        dz = ctx.upload(cs["z"][0][p])
        dt = ctx.alloc(count * cs["D"] * 32)
        z, t = C.c_void_p(dz.ptr), C.c_void_p(dt.ptr)
        r, s = _fr_array(cs["r"][0][p]), _fr_array(cs["s"][0][p])
        out = np.full(192 * count, 0xA5, dtype=np.uint8)
        o = out.ctypes.data_as(C.c_void_p)
        call = lambda pk_, cnt, tx, ty, tz: ctx.lib.zk_groth16_prove_shared_batch(ctx.h, pk_.h, dr.h, cnt, z, r, s, tx, ty, tz, None, o, None)
        rc = dict(zero=call(pk, 0, None, None, None), partial=call(pk, count, t, None, t), key=call(pk_other, count, None, None, None),
                  nomem=call(pk, 1 << 40, None, None, None))
        untouched = bool(np.all(out == 0xA5))
        return rc, untouched, party.create_proofs_shared_native(pk, dr, dz.ptr, cs["r"][0][p], cs["s"][0][p])

    (rc, untouched, proofs), = run_parties(1, fn)
    assert rc == dict(zero=ZK_ERR_ARG, partial=ZK_ERR_ARG, key=ZK_ERR_ARG, nomem=ZK_ERR_NOMEM)
    assert untouched
    assert proofs == cs["want"]             # the context proves normally afterwards
