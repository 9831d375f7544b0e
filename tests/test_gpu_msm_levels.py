"""Shifted window multiples on the device (zk_msm_mul_levels; msm_digits.cuh: level_bucket; msm.hip: msm_set_sum): a key whose tables
also hold 2^m times every window multiple, m <= M, reduces 2^(c-2) + 2^(c-2-M) buckets instead of 2^(c-1) and must give the same
sums, hence the same proof bytes, for M = 0 .. 3 -- through the single prover, the batch prover, the additive shared prover, and for
MSMs over a key's query tables with scalars whose signed window digits sit on every edge of the mapping."""
import threading

import numpy as np
import pytest

import zkref as O
import zkref_c as OC
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
import pyseq.mpc_seq as mpc
from helpers import mont1, td_mont
from oracle_backend import additive_shares

pytestmark = pytest.mark.gpu

_CASES = {}


def mul_chain_case(log_n):
    """one mul-chain system per size with its trapdoor, assignment, (r, s) and the known-trapdoor prediction: computed once"""
    if log_n not in _CASES:
        rng = O.Prng(0x1e7e15 + log_n)
        n = (1 << log_n) - 2
        w0, w1, r, s = rng.fr(), rng.fr(), rng.fr(), rng.fr()
        td = O.Trapdoor(rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr())
        _, z = O.mul_chain_r1cs(n, w0, w1)
        cr = OC.R1cs(2, n + 1, *OC.mul_chain_csr(n))
        tdm, zm = td_mont(td), cv.fr_to_mont(z)
        want = OC.groth16_predict(cr, tdm, zm, OC.witness_map(cr, zm), mont1(r), mont1(s))
        _CASES[log_n] = dict(n=n, z=z, zm=zm, r=r, s=s, tdm=tdm, want=want, cr=cr)
    return _CASES[log_n]


def key_with_levels(ctx, case, M):
    ctx.msm_mul_levels(M)
    try:
        dr = ctx.r1cs_mul_chain(case["n"])
        pk = ctx.groth16_setup(dr, *[case["tdm"][i] for i in range(7)])
    finally:
        ctx.msm_mul_levels(-1)
    return dr, pk


@pytest.mark.parametrize("log_n", [10, 12])
@pytest.mark.parametrize("M", [0, 1, 2, 3])
def test_proof_bytes_do_not_depend_on_the_levels(ctx, log_n, M):
    case = mul_chain_case(log_n)
    dr, pk = key_with_levels(ctx, case, M)
    c = ctx.lib.zk_bases_window_bits(pk.query_bases("a_query").h)
    assert pk.mul_levels() == ctx.lib.zk_msm_mul_levels_clamp(c, M) == M        # (c = 13 / 15: no clamp at these sizes)
    dz = ctx.upload(case["zm"])
    for _ in range(3):                                    # (the third sort with the same arguments replays a captured graph)
        assert ctx.create_proof_dev(pk, dr, dz.ptr, mont1(case["r"]), mont1(case["s"])) == case["want"]
    dz.free(); pk.free()


def test_levels_are_clamped_for_the_smallest_tables(ctx):
    """a key of 2^8 constraints has windows of c = 10 bits: three levels would leave reduce windows of 2^5 buckets, so it gets two"""
    rng = O.Prng(0xc1a9)
    n = (1 << 8) - 2
    w0, w1, r, s = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    td = O.Trapdoor(rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr(), rng.fr())
    _, z = O.mul_chain_r1cs(n, w0, w1)
    case = dict(n=n, tdm=td_mont(td))
    dr, pk = key_with_levels(ctx, case, 3)
    c = ctx.lib.zk_bases_window_bits(pk.query_bases("a_query").h)
    assert 8 <= c <= 10, c
    assert pk.mul_levels() == ctx.lib.zk_msm_mul_levels_clamp(c, 3) == c - 8
    assert c - 2 - pk.mul_levels() >= 6
    cr = OC.R1cs(2, n + 1, *OC.mul_chain_csr(n))
    zm = cv.fr_to_mont(z)
    dz = ctx.upload(zm)
    assert ctx.create_proof_dev(pk, dr, dz.ptr, mont1(r), mont1(s)) == OC.groth16_predict(cr, case["tdm"], zm, OC.witness_map(cr, zm), mont1(r), mont1(s))
    dz.free(); pk.free()


def test_batch_prover_over_a_key_with_levels(ctx):
    case = mul_chain_case(10)
    dr, pk = key_with_levels(ctx, case, 2)
    assert pk.mul_levels() == 2
    rng = O.Prng(0xba7c4)
    n, count = case["n"], 5
    zs = [case["zm"]] + [ctx.download(ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr())), (n + 3, 4)) for _ in range(count - 1)]
    rl = [mont1(case["r"])] + [mont1(rng.fr()) for _ in range(count - 1)]
    sl = [mont1(case["s"])] + [mont1(rng.fr()) for _ in range(count - 1)]
    dz = ctx.upload(np.concatenate(zs))
    got = ctx.create_proofs_batch_dev(pk, dr, dz.ptr, count, rl, sl)
    assert got[0] == case["want"]
    cr = case["cr"]
    assert got[1:] == [OC.groth16_predict(cr, case["tdm"], zs[k], OC.witness_map(cr, zs[k]), rl[k], sl[k]) for k in range(1, count)]
    dz.free(); pk.free()


def test_additive_shared_prover_over_a_key_with_levels():
    case = mul_chain_case(10)
    rng = O.Prng(0x5a4ed)
    n_parties = 2
    zsh = additive_shares(case["z"], n_parties, rng, public_prefix=2)
    rsh, ssh = O.additive_share(case["r"], n_parties, rng), O.additive_share(case["s"], n_parties, rng)
    nets = mpc.LocalNet.create(n_parties)
    out, err = [None] * n_parties, []

    def work(p):
        ctx = Z.Context(0, p, n_parties)
        try:
            party = mpc.Party(ctx, net=nets[p])
            dr, pk = key_with_levels(ctx, case, 3)
            assert pk.mul_levels() == 3
            dz = ctx.upload(cv.fr_to_mont(zsh[p]))
            out[p] = (party.create_proof_shared(pk, dr, dz.ptr, mont1(rsh[p]), mont1(ssh[p])),
                      party.create_proof_shared_native(pk, dr, dz.ptr, mont1(rsh[p]), mont1(ssh[p])))
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
    assert all(o == (case["want"], case["want"]) for o in out)


# ---- MSMs over a key's query tables with scalars built from their signed window digits ----

def signed_digits(v, c):
    """the digits d_w in [-2^(c-1), 2^(c-1) - 1] with v = sum_w d_w 2^(c w) (msm_digits.cuh: the bias makes every window independent)"""
    W = (255 + c - 1) // c
    out = []
    for w in range(W):
        d = v & ((1 << c) - 1)
        v >>= c
        if d >= 1 << (c - 1):
            d -= 1 << c
            v += 1
        out.append(d)
    assert v == 0
    return out


def from_digits(ds, c):
    return sum(d << (c * w) for w, d in enumerate(ds))


def scalar_sets(c, n, rng):
    """name -> n scalars in [0, r)"""
    r = O.R_MOD
    W = (255 + c - 1) // c
    top_bits = r.bit_length() - 1 - c * (W - 1)           # a top digit below 2^top_bits keeps the scalar below r
    assert top_bits >= 1
    sets = {"zero": [0] * n, "all_equal": [rng.fr()] * n, "r_minus_1": [r - 1] * n}
    # every digit of scalar i is +-2^k, k = i mod c: v = k below, at and above every M.  +2^(c-1) is not a digit (the range ends at
    # 2^(c-1) - 1), so k = c - 1 is -2^(c-1) everywhere; the top digit is positive and small enough for the scalar to stay below r
    pow2, edge = [], []
    for i in range(n):
        k = i % c
        ds = [(-1 if (k == c - 1 or (w + i // c) % 2) else 1) << k for w in range(W - 1)] + [1 << min(k, top_bits - 1)]
        v = from_digits(ds, c)
        assert 0 < v < r and signed_digits(v, c) == ds
        pow2.append(v)
        ds = [-(1 << (c - 1))] * (W - 1) + [1 + i % 2]    # magnitude 2^(c-1) in every window (the top one cannot hold it: 1 or 2 there)
        v = from_digits(ds, c)
        assert 0 < v < r and signed_digits(v, c) == ds
        edge.append(v)
    sets["pow2_digits"], sets["half_digits"] = pow2, edge
    # carries through all windows: 2^252 - 1 - j (unsigned windows all ones: -1 - j, zeros, a carry into the top), and unsigned
    # windows that all read 2^(c-1): every one turns negative and hands a carry on
    ripple = []
    for i in range(n):
        if i % 2:
            v = (1 << 252) - 1 - i // 2
        else:
            v = sum(((1 << (c - 1)) + (i // 2) % 3) << (c * w) for w in range(W - 1))
        ds = signed_digits(v, c)
        assert 0 < v < r and (all(d <= 0 for d in ds[:-1]) and ds[-1] >= 1)
        ripple.append(v)
    sets["carries"] = ripple
    return sets


_MSM_WANT = {}


@pytest.mark.parametrize("M", [0, 1, 2, 3])
def test_key_query_msms_on_digit_edges(ctx, M):
    """A G1 and a G2 MSM over the a_query / b_g2_query tables of the smallest key that is not clamped (2^10 constraints: c = 13),
    against the oracle's MSM over the downloaded points.  The expected sums do not depend on M: computed once."""
    case = mul_chain_case(10)
    dr, pk = key_with_levels(ctx, case, M)
    assert pk.mul_levels() == M
    for name, group in (("a_query", 1), ("b_g2_query", 2)):
        q = pk.query_bases(name)
        n = len(q)
        c = ctx.lib.zk_bases_window_bits(q.h)
        assert c >= 2 + 3 + 6                                # all of M = 0 .. 3 unclamped
        sets = scalar_sets(c, n, O.Prng(0xd161 + group))
        if group not in _MSM_WANT:
            pts = pk.download(name)
            ref = OC.msm_g1 if group == 1 else OC.msm_g2
            to_aff = cv.g1_projective_to_affine if group == 1 else cv.g2_projective_to_affine
            _MSM_WANT[group] = {k: to_aff(ref(pts, cv.fr_to_mont(v))) for k, v in sets.items()}
            _MSM_WANT[group]["offset"] = to_aff(ref(pts[1:], cv.fr_to_mont(sets["pow2_digits"][:n - 1])))      # query[1..] as the provers use it
        to_aff = cv.g1_projective_to_affine if group == 1 else cv.g2_projective_to_affine
        for k, v in sets.items():
            ds = ctx.upload(cv.fr_to_mont(v))
            assert to_aff(ctx.msm_dev(q, 0, ds.ptr, n)) == _MSM_WANT[group][k], (name, k, M)
            if k == "pow2_digits":
                assert to_aff(ctx.msm_dev(q, 1, ds.ptr, n - 1)) == _MSM_WANT[group]["offset"], (name, k, M, "offset")
            ds.free()
    pk.free()
