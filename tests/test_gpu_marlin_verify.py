"""GPU: the segmented G1 linear combination (csrc/g1_lincomb.hip) word for word against the host instantiation of the same per-term
source, and zk_marlin_verify_batch against the fixture of oracle verdicts (tests/golden/marlin_verify.json), on batches that fill
a wave, overflow it by one and consist of rejected proofs only; one live proof from zk_marlin_prove confirmed by the oracle."""
import numpy as np
import pytest

import marlin_ref as M
import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from helpers import marlin_test_system
import marlin_verify_cases as MC

pytestmark = pytest.mark.gpu


def test_lincomb_device_equals_host_on_the_seams(ctx):
    points, idx, ks, off, want = MC.lincomb_cases()
    rc_h, host = MC.lincomb(points, idx, ks, off)
    rc_d, dev = MC.lincomb(points, idx, ks, off, ctx)
    assert rc_h == 0 and rc_d == 0
    assert np.array_equal(dev, host), [s for s in range(len(host)) if not np.array_equal(dev[s], host[s])]
    assert cv.g1_array_to_affine(dev) == want


@pytest.mark.parametrize("lens", [[1] * 64, [1] * 65, [64, 1], [40, 40, 40], [63, 2, 64, 0, 1], [33] * 5 + [1]])
def test_lincomb_wave_packing(ctx, lens):
    """Segment lists that fill a wave exactly, spill one lane into the next, would straddle a boundary unless the packing pads,
    and end with a wave that holds a single one-term segment."""
    rng = O.Prng(0x9ac4 + len(lens))
    points, _, _, _, _ = MC.lincomb_cases()
    n = sum(lens)
    idx = np.array([rng.u64() % len(points) for _ in range(n)], dtype=np.uint32)
    ks = np.array([MC.scalar_words(rng.fr() if i % 3 else (rng.u64() << 192) | rng.u64()) for i in range(n)], dtype=np.uint32).reshape(-1, 8)
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    rc_h, host = MC.lincomb(points, idx, ks, off)
    rc_d, dev = MC.lincomb(points, idx, ks, off, ctx)
    assert rc_h == 0 and rc_d == 0
    assert np.array_equal(dev, host)
    s = int(np.argmax(lens))                   # one segment against the oracle as well
    want = None
    pts = cv.g1_array_to_affine(points)
    for t in range(off[s], off[s + 1]):
        k = sum(int(w) << (32 * i) for i, w in enumerate(ks[t]))
        want = O.g1_add(want, O.g1_mul(pts[idx[t]], k % O.R_MOD) if pts[idx[t]] is not None else None)
    assert cv.g1_array_to_affine(dev[s:s + 1])[0] == want


def test_lincomb_device_refuses_65_terms(ctx):
    points, _, _, _, _ = MC.lincomb_cases()
    assert MC.lincomb(points, np.zeros(65, np.uint32), np.ones((65, 8), np.uint32), np.array([0, 65], np.uint32), ctx)[0] == -2


@pytest.mark.parametrize("count", [1, 2, 63, 64, 65])
def test_verify_batch_gives_the_fixture_verdicts(ctx, count):
    """The variants of both systems cycled to `count` proofs (each system under its own key): every verdict is the fixture's."""
    for si, system in enumerate(MC.fixture()["systems"]):
        vk = MC.vk_of(system)
        vs = system["variants"]
        picks = [vs[(3 * si + k) % len(vs)] for k in range(count)]
        args = [MC.variant_args(v) for v in picks]
        got = DM.verify_batch(ctx, vk, np.stack([a[0] for a in args]), [a[1] for a in args])
        want = [a[2] for a in args]
        assert list(got) == want, [(v["name"], int(g), w) for v, g, w in zip(picks, got, want) if g != w]


def test_verify_batch_of_rejected_proofs_only(ctx):
    system = MC.fixture()["systems"][1]
    vk = MC.vk_of(system)
    args = [MC.variant_args(v) for v in system["variants"] if v["verdict"] == 0]
    assert len(args) >= 10
    got = DM.verify_batch(ctx, vk, np.stack([a[0] for a in args]), [a[1] for a in args])
    assert not got.any()
    assert DM.verify_batch(ctx, vk, args[0][0][None], [b""]).tolist() == [0]           # an empty proof is a proof that does not parse


def test_verify_batch_subgroup_test_rejects_cofactor_torsion(ctx):
    """The accepted proof with W_gamma moved by a point of the cofactor's torsion satisfies both pairing equations
    (tests/test_marlin_verify_host.py shows why): the one-term segments r P of the combination launch are what rejects it, and
    only it."""
    system = MC.fixture()["systems"][0]
    good_in, good, _ = MC.variant_args(system["variants"][0])
    inputs, moved = MC.witness_plus_torsion(system)
    got = DM.verify_batch(ctx, MC.vk_of(system), np.stack([good_in, inputs, good_in]), [good, moved, good])
    assert got.tolist() == [1, 0, 1]


def test_verify_batch_timer_names(ctx):
    """With profiling, one batch of one accepted proof leaves exactly these timers, each counted once: the laps by the host's clock,
    the k_ phases by device events (tools/bench_marlin_verify.py reads them by name)."""
    system = MC.fixture()["systems"][0]
    inputs, good, verdict = MC.variant_args(system["variants"][0])
    ctx.set_profiling(True)
    try:
        ctx.timers()
        got_ok = DM.verify_batch(ctx, MC.vk_of(system), inputs[None], [good])
        got = ctx.timers()
    finally:
        ctx.set_profiling(False)
    print(sorted(got.items()))
    assert verdict == 1 and got_ok.tolist() == [1]
    names = ("parse", "decompress", "build", "device", "k_decompress", "k_lincomb", "k_pairing")
    assert {k: c for k, (_, c) in got.items()} == {"marlin_verify." + w: 1 for w in names}


def _raw_batch(ctx, vk, count, inputs, n_inputs, proofs, offsets, ok):
    """zk_marlin_verify_batch as the C ABI has it: the return code, nothing raised."""
    import ctypes as C
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    return ctx.lib.zk_marlin_verify_batch(ctx.h, None if vk is None else C.byref(vk.struct), count, p(inputs), n_inputs, p(proofs), p(offsets), p(ok))


def test_verify_batch_caller_errors(ctx):
    """What is wrong with the call is ZK_ERR_ARG (-2), through the binding as ZkError; ok[] stays untouched and the context usable."""
    from zk_mpc_amd._lib import ZkError
    system = MC.fixture()["systems"][0]
    vk = MC.vk_of(system)
    inputs, proof, _ = MC.variant_args(system["variants"][0])
    with pytest.raises(ZkError, match="error -2"):
        DM.verify_batch(ctx, vk, np.zeros((0, 1, 4), np.uint64), [])                            # count = 0
    with pytest.raises(ZkError, match="error -2"):
        DM.verify_batch(ctx, vk, cv.fr_raw([O.R_MOD])[None], [proof])                           # an input not below r
    k = system["key"]
    bad = DM.VerifierKey.from_parts(bytes.fromhex(k["ivk_bytes"])[:-1], MC._g1(k["g"]), MC._g1(k["gamma_g"]), MC._g2(k["h"]), MC._g2(k["beta_h"]),
                                    MC._g1(k["shift_h"]), MC._g1(k["shift_k"]))
    with pytest.raises(ZkError, match="error -2"):
        DM.verify_batch(ctx, bad, inputs[None], [proof])                                        # ivk_len
    # the batch's own: null pointers, count above 2^20 (checked before anything is read), decreasing offsets
    inp = np.ascontiguousarray(np.stack([inputs, inputs]))
    buf = np.frombuffer(proof + proof, dtype=np.uint8)
    off = np.array([0, len(proof), 2 * len(proof)], dtype=np.uint64)
    ok = np.full(2, 7, dtype=np.int32)
    assert _raw_batch(ctx, vk, 2, inp, 1, buf, off, ok) == 0 and ok.tolist() == [1, 1]
    ok[:] = 7
    assert _raw_batch(ctx, None, 2, inp, 1, buf, off, ok) == -2
    assert _raw_batch(ctx, vk, 2, None, 1, buf, off, ok) == -2
    assert _raw_batch(ctx, vk, 2, inp, 1, None, off, ok) == -2
    assert _raw_batch(ctx, vk, 2, inp, 1, buf, None, ok) == -2
    assert _raw_batch(ctx, vk, 2, inp, 1, buf, off, None) == -2
    assert _raw_batch(ctx, vk, (1 << 20) + 1, inp, 1, buf, off, ok) == -2
    assert _raw_batch(ctx, vk, 2, inp, 1, buf, np.array([0, 2 * len(proof), len(proof)], dtype=np.uint64), ok) == -2
    assert ok.tolist() == [7, 7]
    assert DM.verify_batch(ctx, vk, inputs[None], [proof]).tolist() == [1]                      # the context is as usable as before


def _device_system(ctx, n, seed):
    rng = O.Prng(seed)
    r1cs, z = marlin_test_system(n, rng)
    sq, zz = M.pad_and_square(r1cs, z)
    dix = DM.Index(ctx, sq.num_instance, sq.num_witness, DM.Csr.from_rows(sq.a), DM.Csr.from_rows(sq.b), DM.Csr.from_rows(sq.c))
    return rng, zz, dix


def test_device_prover_reproduces_the_fixture_and_its_key(ctx):
    """n = 3 under the fixture's seeds: zk_marlin_prove writes the fixture's good proof, and the VerifierKey taken from the device's
    index and SRS tables is the fixture's key, field by field; host and device verifiers accept it."""
    from zk_mpc_amd.api import Rng
    system = MC.fixture()["systems"][0]
    assert system["system"] == 3
    rng, zz, dix = _device_system(ctx, 3, system["prng_seed"])
    beta, g_k, gg_k, h_k = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    assert hex(beta) == system["srs"]["beta"] and hex(h_k) == system["srs"]["h_k"]
    keys = DM.IndexKeys(dix, DM.UniversalSrs(ctx, system["max_degree"], beta, g_k, gg_k))
    proof = DM.prove_native(keys, ctx.upload(cv.fr_to_mont(zz)), Rng.from_seed(bytes.fromhex(system["prover_seed"]), 20))
    assert proof.hex() == system["variants"][0]["proof"]
    h = O.g2_mul(O.G2_GEN, h_k)
    vk = DM.VerifierKey(keys, cv.g2_affine_to_array([h])[0], cv.g2_affine_to_array([O.g2_mul(h, beta)])[0])
    assert bytes(vk.struct)[16:] == bytes(MC.vk_of(system).struct)[16:] and vk.ivk == MC.vk_of(system).ivk
    inputs = cv.fr_to_mont(zz[1:dix.num_instance])
    assert DM.verify_host(vk, inputs, proof)
    assert DM.verify_batch(ctx, vk, inputs[None], [proof]).tolist() == [1]


def test_live_proof_at_1000_constraints(ctx):
    """A proof from zk_marlin_prove at n = 1000 is accepted and, with the first input + 1, rejected; the oracle's verifier, on the
    device's index commitments, says the same of both."""
    import marlin_full_ref as MF
    from zk_mpc_amd.api import Rng
    rng, zz, dix = _device_system(ctx, 1000, 0x3e8)
    beta, g_k, gg_k, h_k = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    max_degree = DM.ahp_max_degree(dix) + 5
    keys = DM.IndexKeys(dix, DM.UniversalSrs(ctx, max_degree, beta, g_k, gg_k))
    proof = DM.prove_native(keys, ctx.upload(cv.fr_to_mont(zz)), Rng.from_seed(bytes(range(32)), 20))

    class PP:
        pass
    pp = PP()
    pp.beta = beta
    pp.g, pp.gamma_g, pp.h = O.g1_mul(O.G1_GEN, g_k), O.g1_mul(O.G1_GEN, gg_k), O.g2_mul(O.G2_GEN, h_k)
    pp.beta_h = O.g2_mul(pp.h, beta)
    vk = DM.VerifierKey(keys, cv.g2_affine_to_array([pp.h])[0], cv.g2_affine_to_array([pp.beta_h])[0])
    pub = zz[1:dix.num_instance]
    wrong = [(pub[0] + 1) % O.R_MOD] + pub[1:]
    got = DM.verify_batch(ctx, vk, np.stack([cv.fr_to_mont(pub), cv.fr_to_mont(wrong)]), [proof, proof])
    assert got.tolist() == [1, 0]
    info = M.IndexInfo(dix.num_constraints, dix.num_non_zero, dix.num_instance)
    info.num_variables, info.num_constraints, info.num_non_zero = dix.num_variables, dix.num_constraints, dix.num_non_zero
    okeys = MF.Keys(info, pp, max_degree=max_degree, index_comms={l: keys.index_comms[l].comm_aff for l in MF.INDEX_LABELS})
    assert okeys.ivk_bytes() == keys.ivk_bytes()
    as_oracle = MF.proof_deserialize(proof)
    assert MF.verify(okeys, pub, as_oracle) and not MF.verify(okeys, wrong, as_oracle)
