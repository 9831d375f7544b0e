"""GPU: zk_marlin_prove_batch (csrc/marlin_prove_batch.hip) against zk_marlin_prove.  The whole contract is "proof k is byte for
byte the single prover's proof of (z_k, rngs[k]), and rngs[k] is left as the single call leaves it": every test here compares with
prove_native on the same index under a generator of the same seed -- over mul-chains with different assignments per proof,
circuit-shaped systems (|K| = 4 |H|, eight public inputs), a stride larger than the assignment, the device mask sampler, the seam
between chunks, polynomials of one span and of several in the batched division by X - z, a failing proof in the middle, and the
argument checks."""
import ctypes as C

import numpy as np
import pytest

import marlin_ref as M
import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from helpers import marlin_test_system
from zk_mpc_amd._lib import ZkError
from zk_mpc_amd.api import Rng

pytestmark = pytest.mark.gpu

SPAN = 4096      # coefficients one span of poly.hip's division by X - z holds
_SYSTEMS = {}    # system name -> (index, keys, srs parameters): built once, shared and left unchanged


def _seed(k, salt=0):
    return bytes((7 * k + 3 * i + salt) & 0xff for i in range(32))


def _system(ctx, name):
    """An index with its keys: an int is the mul-chain of that many constraints, a string a system of helpers.marlin_test_system."""
    if name not in _SYSTEMS:
        fixed = None
        if isinstance(name, int):
            index = DM.Index(ctx, *DM.mul_chain_system(ctx, name))
        else:
            r1cs, z = marlin_test_system(name, O.Prng(0xb47c + len(name)))
            sq, zz = M.pad_and_square(r1cs, z)
            index = DM.Index(ctx, sq.num_instance, sq.num_witness, DM.Csr.from_rows(sq.a), DM.Csr.from_rows(sq.b), DM.Csr.from_rows(sq.c))
            fixed = zz
        srs_par = (DM.ahp_max_degree(index) + 5, 0x1234567, 3, 7)
        _SYSTEMS[name] = (index, DM.IndexKeys(index, DM.UniversalSrs(ctx, *srs_par)), srs_par, fixed)
    return _SYSTEMS[name]


def _assignments(ctx, name, count, z_stride=None, salt=0):
    """count padded assignments back to back, z_stride elements apart: (buffer, stride, the single buffers).  The mul-chain gets
    different w0, w1 per proof (so assignments, public inputs and transcripts differ); the other systems one assignment."""
    index, _, _, fixed = _system(ctx, name)
    m = DM.HostField.m
    if fixed is None:
        singles = [ctx.mul_chain_assignment_dev(name, m(3 + 2 * k + salt), m(5 + 11 * k + salt)) for k in range(count)]
    else:
        singles = [ctx.upload(cv.fr_to_mont(fixed)) for _ in range(count)]
    nv = index.num_variables
    stride = nv if z_stride is None else z_stride
    both = ctx.alloc(count * stride * 32)
    ctx.dev_zero(both.ptr, count * stride * 32)
    for k, z in enumerate(singles):
        ctx.memcpy_d2d(both.ptr + k * stride * 32, z.ptr, nv * 32)
    ctx.sync()
    return both, stride, singles


def _singles(keys, singles, mask_on_device=False, salt=0):
    """The single prover's proofs and the next draw of each generator after its call."""
    proofs, draws = [], []
    for k, z in enumerate(singles):
        rng = Rng.from_seed(_seed(k, salt), 20)
        proofs.append(DM.prove_native(keys, z, rng, mask_on_device=mask_on_device))
        draws.append(rng.next_u64())
    return proofs, draws


def _batch(keys, both, stride, count, mask_on_device=False, salt=0):
    rngs = [Rng.from_seed(_seed(k, salt), 20) for k in range(count)]
    got = DM.prove_native_batch(keys, both, stride, rngs, mask_on_device=mask_on_device)
    return got, [r.next_u64() for r in rngs]


def _longest_opened(index):
    """The longest polynomial open_combinations divides by X - z: the mask polynomial (3 |H|), h_1 (2 |H| + 1) or h_2 (|B| - |K|)."""
    H, K, B = index.dom_h.size, index.dom_k.size, index.dom_b.size
    return max(3 * H, 2 * H + 1, B - K)


@pytest.mark.parametrize("name,count,mask_on_device,extra_stride", [
    (3, 2, False, 0), (3, 48, False, 0), (13, 3, False, 5), (13, 3, True, 0), (1000, 5, False, 0), (2000, 2, False, 0), ("tiny9", 3, False, 0), ("dense8", 2, False, 0)])
def test_batch_equals_singles(ctx, name, count, mask_on_device, extra_stride):
    """(3, 48) beside the small counts: from some 160 scalar multiplications per step on, the blinding terms are one launch on the
    device instead of tasks on the host's helper threads."""
    index, keys, _, _ = _system(ctx, name)
    if name == "dense8":
        assert index.dom_k.size == 4 * index.dom_h.size and index.num_instance == 8      # the shape the mul-chain never has
    if name == 2000:
        assert _longest_opened(index) > SPAN      # several spans: the three-launch arm of the batched division by X - z
    if name == 13:
        assert _longest_opened(index) < SPAN      # one span: the one-launch arm
    both, stride, singles = _assignments(ctx, name, count, index.num_variables + extra_stride if extra_stride else None)
    want, want_draws = _singles(keys, singles, mask_on_device)
    got, got_draws = _batch(keys, both, stride, count, mask_on_device)
    assert got == want, [k for k in range(count) if got[k] != want[k]]
    assert len(set(got)) == count
    assert got_draws == want_draws


def test_the_oracle_verifier_accepts_a_batch_proof(ctx):
    """Proof 0 of (3, 2) under marlin_full_ref.verify: accepted, and rejected with the first input + 1."""
    import marlin_full_ref as MF
    index, keys, (max_degree, beta, g_k, gg_k), _ = _system(ctx, 3)
    both, stride, singles = _assignments(ctx, 3, 2)
    got, _ = _batch(keys, both, stride, 2)
    zz = cv.fr_from_mont(ctx.download(singles[0], (index.num_variables, 4)))

    class PP:
        pass
    pp = PP()
    pp.beta = beta
    pp.g, pp.gamma_g, pp.h = O.g1_mul(O.G1_GEN, g_k), O.g1_mul(O.G1_GEN, gg_k), O.g2_mul(O.G2_GEN, 5)
    pp.beta_h = O.g2_mul(pp.h, beta)
    info = M.IndexInfo(index.num_constraints, index.num_non_zero, index.num_instance)
    info.num_variables, info.num_constraints, info.num_non_zero = index.num_variables, index.num_constraints, index.num_non_zero
    okeys = MF.Keys(info, pp, max_degree=max_degree, index_comms={l: keys.index_comms[l].comm_aff for l in MF.INDEX_LABELS})
    assert okeys.ivk_bytes() == keys.ivk_bytes()
    pub = zz[1:index.num_instance]
    wrong = [(pub[0] + 1) % O.R_MOD] + pub[1:]
    proof = MF.proof_deserialize(got[0])
    assert MF.verify(okeys, pub, proof) and not MF.verify(okeys, wrong, proof)


def test_the_seam_between_chunks(ctx, monkeypatch):
    """(13, 5) in chunks of 2, 2 and 1: the bytes of the unchunked call and of the singles; twice, over the same scratch."""
    _, keys, _, _ = _system(ctx, 13)
    both, stride, singles = _assignments(ctx, 13, 5, salt=1)
    want, want_draws = _singles(keys, singles, salt=1)
    whole, _ = _batch(keys, both, stride, 5, salt=1)
    monkeypatch.setenv("ZK_MARLIN_BATCH_CHUNK", "2")
    for _ in range(2):
        got, got_draws = _batch(keys, both, stride, 5, salt=1)
        assert got == whole == want
        assert got_draws == want_draws


def test_a_bad_proof_in_the_middle_fails_the_call_and_leaves_the_context_usable(ctx):
    index, keys, _, _ = _system(ctx, 13)
    nv = index.num_variables
    both, stride, singles = _assignments(ctx, 13, 3, salt=2)
    want, _ = _singles(keys, singles, salt=2)
    z1 = ctx.download(singles[1], (nv, 4))
    bad = cv.fr_from_mont(z1)
    bad[4] = (bad[4] + 1) % O.R_MOD                  # one witness element + 1
    broken = ctx.alloc(3 * stride * 32)
    ctx.memcpy_d2d(broken.ptr, both.ptr, 3 * stride * 32)
    ctx.memcpy_d2d(broken.ptr + stride * 32, ctx.upload(cv.fr_to_mont(bad)).ptr, nv * 32)
    ctx.sync()
    with pytest.raises(ZkError, match=r"proof 1: .*sum over H|proof 1: .*divisible"):
        _batch(keys, broken, stride, 3, salt=2)
    got, _ = _batch(keys, both, stride, 3, salt=2)
    assert got == want


def test_arguments(ctx):
    index, keys, _, _ = _system(ctx, 3)
    both, stride, singles = _assignments(ctx, 3, 2)
    with pytest.raises(ZkError, match="error -2"):
        DM.prove_native_batch(keys, both, stride, [])                                     # count = 0
    with pytest.raises(ZkError, match="error -2.*z_stride"):
        _batch(keys, both, index.num_variables - 1, 2)
    d, _keep = DM.native_index(keys)
    slot = ctx.lib.zk_marlin_proof_max_size()
    out, lens = (C.c_uint8 * (2 * slot))(), (C.c_size_t * 2)()
    rngs = [Rng.from_seed(_seed(k), 20) for k in range(2)]
    handles = (C.c_void_p * 2)(*[r.h for r in rngs])
    rc = ctx.lib.zk_marlin_prove_batch(ctx.h, C.byref(d), keys.srs.powers_g.h, keys.srs.powers_gamma_g.h, 2, C.c_void_p(both.ptr), stride, handles, 0, out,
                                       slot - 1, lens)
    assert rc == -2
    # count = 1 is the single prover
    want, want_draws = _singles(keys, singles[:1])
    got, got_draws = _batch(keys, both, stride, 1)
    assert got == want and got_draws == want_draws
