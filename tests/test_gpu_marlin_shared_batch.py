"""GPU: count collaborative Marlin proofs of one index in one call (zk_marlin_prove_shared_batch / _spdz_batch; parties = threads on
device 0 over LocalNet).  The contract is "proof k at every party is byte for byte what zk_marlin_prove_shared[_spdz] writes for (z_k,
rngs[k], triple_k), rngs[k] is left as that call leaves it, and the call makes one exchange for its plan plus the single call's per
chunk": every test compares with the single call on the same shares under generators of the same seeds -- over mul-chains with an
assignment per proof, circuit-shaped systems, a system without public input, the device mask sampler, the seam between chunks, real
Beaver triples, a moved MAC share, an unsatisfied proof in the middle, and the argument checks."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import marlin_full_ref as MF
import marlin_ref as M
import zkref as O
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
import pyseq.marlin_seq as DM
import pyseq.mpc_seq as mpc
from helpers import marlin_test_system
from oracle_backend import additive_shares
from zk_mpc_amd.api import Rng

pytestmark = pytest.mark.gpu

ZK_ERR_ARG, ZK_ERR_STATE, ZK_ERR_MAC = -2, -4, -5
FILL = 0xA5


def run_parties(n_parties, fn):
    """fn(p, ctx, net) per party, each on a thread with its own context on device 0 (as tests/test_gpu_groth16_shared_batch.py::run_parties)."""
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


class _SumRng:
    """The single prover's view of P parties' generators: every draw is the sum of the parties' draws (MpcField::rand gives each
    party a share of the prover's randomness)."""

    def __init__(self, seeds):
        self.rngs = [Rng.from_seed(s, 20) for s in seeds]

    def fill_fr(self, n):
        tot = [0] * n
        for r in self.rngs:
            for i, v in enumerate(cv.fr_from_mont(r.fill_fr(n))):
                tot[i] = (tot[i] + v) % O.R_MOD
        return cv.fr_to_mont(tot) if n else np.zeros((0, 4), dtype=np.uint64)


def _seed(p, k):
    return bytes((11 * p + 37 * k + i) & 0xff for i in range(32))


def _private_chain(n, w0, w1):
    """The mul-chain whose last product stays a witness: variables [1] ++ [w_0 .. w_{n+1}], no public input (num_instance == 1)."""
    w = [w0 % O.R_MOD, w1 % O.R_MOD]
    for i in range(n):
        w.append(w[i] * w[i + 1] % O.R_MOD)
    rows = lambda d: [[(1, 1 + i + d)] for i in range(n)]
    return O.R1CS(1, n + 2, rows(0), rows(1), rows(2)), [1] + w


@functools.lru_cache(maxsize=None)
def case(n_parties, system, count):
    """count assignments of one system shared among n_parties, in a share lane and an independent MAC lane (key 1).  The mul-chains get an
    assignment per proof, the circuit-shaped systems one assignment shared afresh per proof.  Built once per shape and left unchanged."""
    rng = O.Prng(0x5ba7c4 + 131 * n_parties + 17 * count + sum(map(ord, str(system))))
    sq, zz = None, []
    for k in range(count):
        if system == "private6":
            r1cs, z = _private_chain(6, rng.fr(), rng.fr())
        elif isinstance(system, int) or k == 0:
            r1cs, z = marlin_test_system(system, rng)
        sq, z_sq = M.pad_and_square(r1cs, z)
        zz.append(z_sq)
    ni, nv = sq.num_instance, len(zz[0])
    lanes = [[additive_shares(z, n_parties, rng, public_prefix=ni) for z in zz] for _ in range(2)]       # [lane][proof][party]
    per_party = [[cv.fr_to_mont([v for k in range(count) for v in lanes[l][k][p]]) for p in range(n_parties)] for l in range(2)]
    srs = (rng.fr(), rng.fr(), rng.fr(), rng.fr())      # beta, g_k, gg_k, h_k
    csr = tuple(DM.Csr.from_rows(m) for m in (sq.a, sq.b, sq.c))
    n_h = 1 << (nv - 1).bit_length()                   # |H|; the multiplication domain of round 2 holds 3 |H| + 1 coefficients
    return dict(sq=sq, zz=zz, nv=nv, z=per_party, srs=srs, csr=csr, n_mul=4 * n_h)


def _keys(ctx, cs):
    sq = cs["sq"]
    index = DM.Index(ctx, sq.num_instance, sq.num_witness, *cs["csr"])
    return DM.IndexKeys(index, DM.UniversalSrs(ctx, DM.ahp_max_degree(index) + 3, *cs["srs"][:3]))


def _party(ctx, net, spdz):
    return (mpc.SpdzParty if spdz else mpc.Party)(ctx, net=net)


def _batch(party, keys, z, nv, count, p, spdz, mask_dev=False, triple=None):
    """The batch under fresh generators of the proofs' seeds: (proofs, the next draw of each generator)."""
    rngs = [Rng.from_seed(_seed(p, k), 20) for k in range(count)]
    if spdz:
        got = party.marlin_prove_shared_spdz_batch_native(keys, (z[0], z[1]), nv, rngs, triple=triple, mask_on_device=mask_dev)
    else:
        got = party.marlin_prove_shared_batch_native(keys, z[0], nv, rngs, triple=triple, mask_on_device=mask_dev)
    return got, [r.next_u64() for r in rngs]


def _single(party, keys, z, nv, k, p, spdz, mask_dev=False):
    rng = Rng.from_seed(_seed(p, k), 20)
    at = lambda buf: buf.ptr + k * nv * 32
    if spdz:
        proof = party.marlin_prove_shared_spdz_native(keys, (at(z[0]), at(z[1])), rng, mask_on_device=mask_dev)
    else:
        proof = party.marlin_prove_shared_native(keys, at(z[0]), rng, mask_on_device=mask_dev)
    return proof, rng.next_u64()


def _upload(ctx, cs, p):
    return [ctx.upload(cs["z"][l][p]) for l in range(2)]


@pytest.mark.parametrize("n_parties,system,count,spdz,mask_dev", [
    (3, 6, 5, False, False), (2, 40, 3, False, True), (1, 13, 4, False, False), (2, 13, 3, True, True), (8, 6, 2, True, False),
    (3, "dense5", 2, False, False), (3, "tiny9", 2, True, False), (3, 6, 1, False, False), (2, "private6", 2, False, False)])
def test_batch_equals_singles(n_parties, system, count, spdz, mask_dev):
    """(3, 6, 1): count == 1 forwards.  "private6": num_instance == 1, so there is no public-input open."""
    cs = case(n_parties, system, count)
    if system == "private6":
        assert cs["sq"].num_instance == 1

    def fn(p, ctx, net):
        party, keys, z = _party(ctx, net, spdz), _keys(ctx, cs), _upload(ctx, cs, p)
        batch, batch_draws = _batch(party, keys, z, cs["nv"], count, p, spdz, mask_dev)
        singles = [_single(party, keys, z, cs["nv"], k, p, spdz, mask_dev) for k in range(count)]
        return batch, batch_draws, [s[0] for s in singles], [s[1] for s in singles]

    res = run_parties(n_parties, fn)
    for batch, batch_draws, single, single_draws in res:
        assert len(batch) == count
        assert batch == single, [k for k in range(count) if batch[k] != single[k]]
        assert batch_draws == single_draws
        assert batch == res[0][0]                       # every party writes the same bytes
    assert len(set(res[0][0])) == count


def test_the_joint_proof_is_a_proof():
    """Proof k is the plain prover's proof of the summed assignment under the summed randomness; the oracle's verifier accepts the last
    proof of the batch and rejects it with the public input moved by one."""
    n_parties, n, count = 3, 6, 3
    cs = case(n_parties, n, count)

    def fn(p, ctx, net):
        return _batch(_party(ctx, net, False), _keys(ctx, cs), _upload(ctx, cs, p), cs["nv"], count, p, False)[0]

    res = run_parties(n_parties, fn)
    assert all(r == res[0] for r in res)
    ctx = Z.Context(0)
    try:
        keys = _keys(ctx, cs)
        for k in range(count):
            local = DM.prove(keys, ctx.upload(cv.fr_to_mont(cs["zz"][k])), _SumRng([_seed(p, k) for p in range(n_parties)]))
            assert local.serialize(ctx) == res[0][k], "proof %d" % k
        beta, g_k, gg_k, h_k = cs["srs"]
        oix = M.Index(cs["sq"])
        okeys = MF.Keys(oix, O.KzgParams(keys.srs.max_degree, beta, g_k=g_k, gg_k=gg_k, h_k=h_k))
        pub = cs["zz"][count - 1][1:oix.num_instance]
        proof = MF.proof_deserialize(res[0][count - 1])
        assert MF.verify(okeys, pub, proof)
        assert not MF.verify(okeys, [(pub[0] + 1) % O.R_MOD] + pub[1:], proof)
    finally:
        ctx.close()


def _counted(party, net):
    """Counts net.all_gather_small and party.be.open_vec from here on."""
    calls = {"small": 0, "vec": 0}
    gather, open_vec = net.all_gather_small, party.be.open_vec

    def counted_gather(*a, **kw):
        calls["small"] += 1
        return gather(*a, **kw)

    def counted_open(*a, **kw):
        calls["vec"] += 1
        return open_vec(*a, **kw)
    net.all_gather_small, party.be.open_vec = counted_gather, counted_open
    return calls


def _exchanges(n_parties, n, count, spdz):
    """Per party: the single call's exchanges and bytes, the batch's, and the batch's proofs."""
    cs = case(n_parties, n, count)

    def fn(p, ctx, net):
        party, keys, z = _party(ctx, net, spdz), _keys(ctx, cs), _upload(ctx, cs, p)
        calls = _counted(party, net)
        sent0 = party.bytes_sent
        _single(party, keys, z, cs["nv"], 0, p, spdz)
        single, single_sent = dict(calls), party.bytes_sent - sent0
        calls.update(small=0, vec=0)
        sent0 = party.bytes_sent
        proofs, _ = _batch(party, keys, z, cs["nv"], count, p, spdz)
        return single, dict(calls), single_sent, party.bytes_sent - sent0, proofs

    return run_parties(n_parties, fn)


def test_the_batch_makes_the_exchanges_of_one_single_call_and_one_for_its_plan():
    count = 5
    for single, batch, single_sent, batch_sent, _ in _exchanges(3, 6, count, False):
        # the four small opens (round 1, round 2, the evaluations, the witness at beta) and the four vector opens (the public input, the
        # two masked Beaver operands, the outer sum-check's constant term) of a proof over additive shares
        assert single == {"small": 4, "vec": 4}
        assert batch == {"small": single["small"] + 1, "vec": single["vec"]}
        assert batch_sent == count * single_sent + 8


@pytest.mark.parametrize("spdz", [False, True])
def test_the_seam_between_chunks(spdz, monkeypatch):
    """count 5 in chunks of 2, 2 and 1: the bytes of the uncut call, and 1 + 3 x the single call's exchanges."""
    count = 5
    whole = _exchanges(3, 6, count, spdz)
    monkeypatch.setenv("ZK_MARLIN_BATCH_CHUNK", "2")        # before the parties start
    cut = _exchanges(3, 6, count, spdz)
    for (single, _, single_sent, _, want), (_, batch, _, batch_sent, got) in zip(whole, cut):
        assert got == want and len(set(got)) == count
        assert batch["small"] + batch["vec"] == 1 + 3 * (single["small"] + single["vec"])
        assert batch == {"small": 1 + 3 * single["small"], "vec": 3 * single["vec"]}
        assert batch_sent == count * single_sent + 8


@pytest.mark.parametrize("spdz", [False, True])
def test_batch_with_real_beaver_triples(spdz):
    """count |MUL| triple shares per lane, proof k's at k |MUL|: the proofs of the dummy source (triples do not move opened values)."""
    n_parties, n, count = 2, 6, 3
    cs = case(n_parties, n, count)
    total = count * cs["n_mul"]
    rng = O.Prng(0x7a1b1e + spdz)
    ta, tb = [rng.fr() for _ in range(total)], [rng.fr() for _ in range(total)]
    tc = [a * b % O.R_MOD for a, b in zip(ta, tb)]
    tr = [[additive_shares(v, n_parties, rng) for v in (ta, tb, tc)] for _ in range(2)]      # [lane][x, y, z][party]

    def fn(p, ctx, net):
        party, keys, z = _party(ctx, net, spdz), _keys(ctx, cs), _upload(ctx, cs, p)
        up = [[ctx.upload(cv.fr_to_mont(tr[l][i][p])) for i in range(3)] for l in range(2)]
        triple = tuple((up[0][i].ptr, up[1][i].ptr) for i in range(3)) if spdz else tuple(up[0][i].ptr for i in range(3))
        real, _ = _batch(party, keys, z, cs["nv"], count, p, spdz, triple=triple)
        dummy, _ = _batch(party, keys, z, cs["nv"], count, p, spdz)
        return real, dummy

    res = run_parties(n_parties, fn)
    for real, dummy in res:
        assert real == dummy == res[0][1] and len(set(real)) == count


def _raw(party, keys, z_lanes, z_stride, count, rngs, spdz, triple=(None, None, None), slot=None):
    """The C call itself on buffers of the fill pattern: (code, last error, output untouched, lengths untouched, proofs)."""
    import zk_mpc_amd.marlin as NM
    ctx = party.be.ctx
    d, _keep_index = NM.native_index(keys)
    vt, errors, _keep = party._net_vtable()
    net = C.byref(vt) if party.net.n > 1 else None
    cap = ctx.lib.zk_marlin_proof_max_size()
    slot = cap if slot is None else slot
    out = np.full(max(count, 1) * cap, FILL, dtype=np.uint8)
    lens = (C.c_size_t * max(count, 1))(*([0xA5A5] * max(count, 1)))
    sent = C.c_uint64(0)
    handles = (C.c_void_p * max(count, 1))(*[r.h if r is not None else None for r in rngs]) if rngs is not None else None
    args = [ctx.h, C.byref(d), keys.srs.powers_g.h, keys.srs.powers_gamma_g.h, count]
    if spdz:
        P2 = C.c_void_p * 2
        lanes = lambda v: P2(*[int(x) if x else None for x in v]) if v is not None else None
        fn, zarg, targs = ctx.lib.zk_marlin_prove_shared_spdz_batch, lanes(z_lanes), [lanes(t) for t in triple]
    else:
        fn, zarg, targs = ctx.lib.zk_marlin_prove_shared_batch, C.c_void_p(int(z_lanes[0])), [C.c_void_p(int(t)) if t else None for t in triple]
    rc = fn(*args, zarg, z_stride, handles, 0, *targs, net, out.ctypes.data_as(C.c_void_p), slot, lens, C.byref(sent))
    assert not errors, errors
    text = (ctx.lib.zk_last_error(ctx.h) or b"").decode()
    proofs = [out[k * slot:k * slot + lens[k]].tobytes() for k in range(count)] if rc == 0 else None
    return rc, text, bool(np.all(out == FILL)), all(v == 0xA5A5 for v in lens), proofs


def test_a_lie_fails_every_party_and_writes_nothing():
    """One word of the last party's MAC share of assignment 1 flipped: ZK_ERR_MAC at every party, the output and the lengths still the fill
    pattern, and the next batch on the same contexts proves correctly."""
    n_parties, n, count = 2, 13, 3
    cs = case(n_parties, n, count)
    nv = cs["nv"]

    def fn(p, ctx, net):
        party, keys, z = _party(ctx, net, True), _keys(ctx, cs), _upload(ctx, cs, p)
        bad = cs["z"][1][p].copy()
        if p == n_parties - 1:
            bad[nv + cs["sq"].num_instance + 2, 0] ^= np.uint64(1)
        dbad = ctx.upload(bad)
        rngs = [Rng.from_seed(_seed(p, k), 20) for k in range(count)]
        rc, text, out_untouched, lens_untouched, _ = _raw(party, keys, (z[0].ptr, dbad.ptr), nv, count, rngs, True)
        try:
            party.marlin_prove_shared_spdz_batch_native(keys, (z[0], dbad), nv, [Rng.from_seed(_seed(p, k), 20) for k in range(count)])
            raised = False
        except mpc.MacCheckError:
            raised = True
        after, _ = _batch(party, keys, z, nv, count, p, True)
        single = [_single(party, keys, z, nv, k, p, True)[0] for k in range(count)]
        return rc, text, out_untouched, lens_untouched, raised, after, single

    for rc, text, out_untouched, lens_untouched, raised, after, single in run_parties(n_parties, fn):
        assert rc == ZK_ERR_MAC and "MAC" in text
        assert out_untouched and lens_untouched
        assert raised
        assert after == single


def test_an_unsatisfied_proof_in_the_middle_fails_every_party_alike():
    """Party 0's share of one witness of assignment 1 plus one: every party gets ZK_ERR_STATE and the same text behind "proof 1: ", nothing
    is written, nobody hangs, and the next call proves correctly."""
    n_parties, n, count = 2, 13, 3
    cs = case(n_parties, n, count)
    nv = cs["nv"]

    def fn(p, ctx, net):
        party, keys, z = _party(ctx, net, False), _keys(ctx, cs), _upload(ctx, cs, p)
        bad = cv.fr_from_mont(cs["z"][0][p])
        if p == 0:
            at = nv + cs["sq"].num_instance + 2
            bad[at] = (bad[at] + 1) % O.R_MOD
        dbad = ctx.upload(cv.fr_to_mont(bad))
        rngs = [Rng.from_seed(_seed(p, k), 20) for k in range(count)]
        res = _raw(party, keys, (dbad.ptr,), nv, count, rngs, False)
        after, _ = _batch(party, keys, z, nv, count, p, False)
        single = [_single(party, keys, z, nv, k, p, False)[0] for k in range(count)]
        return res[:4], after, single

    res = run_parties(n_parties, fn)
    for (rc, text, out_untouched, lens_untouched), after, single in res:
        assert rc == ZK_ERR_STATE
        assert text.startswith("proof 1: ") and "sum over H is not zero" in text
        assert text == res[0][0][1]
        assert out_untouched and lens_untouched
        assert after == single


def test_arguments():
    n, count = 6, 2
    cs = case(1, n, count)
    nv = cs["nv"]

    def fn(p, ctx, net):
        keys, z = _keys(ctx, cs), _upload(ctx, cs, p)
        add, spdz = _party(ctx, net, False), _party(ctx, net, True)
        rngs = lambda: [Rng.from_seed(_seed(p, k), 20) for k in range(count)]
        cap = ctx.lib.zk_marlin_proof_max_size()
        t = ctx.alloc(count * cs["n_mul"] * 32).ptr
        zl = (z[0].ptr, z[1].ptr)
        got = dict(
            zero=_raw(add, keys, zl, nv, 0, [], False),
            generator=_raw(add, keys, zl, nv, count, [rngs()[0], None], False),
            slot=_raw(add, keys, zl, nv, count, rngs(), False, slot=cap - 1),
            stride=_raw(add, keys, zl, nv - 1, count, rngs(), False),
            partial=_raw(add, keys, zl, nv, count, rngs(), False, triple=(t, None, t)),
            partial_lane=_raw(spdz, keys, zl, nv, count, rngs(), True, triple=((t, t), (t, t), (t, None))),
            mac_lane=_raw(spdz, keys, (z[0].ptr, None), nv, count, rngs(), True),
        )
        after = [_batch(add, keys, z, nv, count, p, False)[0], _batch(spdz, keys, z, nv, count, p, True)[0]]
        single = [[_single(add, keys, z, nv, k, p, False)[0] for k in range(count)], [_single(spdz, keys, z, nv, k, p, True)[0] for k in range(count)]]
        return got, after, single

    (got, after, single), = run_parties(1, fn)
    for name, (rc, _, out_untouched, lens_untouched, _) in got.items():
        assert rc == ZK_ERR_ARG, name
        assert out_untouched and lens_untouched, name
    assert after == single                  # the context proves normally afterwards
