"""GPU: Marlin::index as one library call (zk_marlin_index_build, csrc/marlin_index.hip) on systems given as the circuit gives them,
against the two earlier implementations -- the oracle's index polynomials (oracle/marlin_ref.py) and the index that
zk_mpc_amd.marlin.Index / IndexKeys build call by call from Python on the oracle-padded system -- and through the provers and
verifiers: the fixture's bytes, the same proof from both indexes, what the call refuses."""
import ctypes as C

import numpy as np
import pytest

import marlin_ref as M
import zkref as O
import zk_mpc_amd.convert as cv
import pyseq.marlin_seq as DM
import zk_mpc_amd.marlin as ZM
from zk_mpc_amd.api import Rng
from helpers import circuit_system
import marlin_index_cases as IC
import marlin_verify_cases as MC

pytestmark = pytest.mark.gpu

PARTS = ("row", "col", "val", "row_col")


def _python_index(ctx, r1cs, z):
    sq, zz = M.pad_and_square(r1cs, z)
    return sq, zz, DM.Index(ctx, sq.num_instance, sq.num_witness, DM.Csr.from_rows(sq.a), DM.Csr.from_rows(sq.b), DM.Csr.from_rows(sq.c))


def _both(ctx, r1cs, z, beta=0x1234567, g_k=3, gg_k=7, extra=3):
    """-> (padded system, padded assignment, IndexKeys built from Python, NativeIndex built by the one call) over one SRS."""
    sq, zz, pix = _python_index(ctx, r1cs, z)
    srs = DM.UniversalSrs(ctx, DM.ahp_max_degree(pix) + extra, beta, g_k, gg_k)
    return sq, zz, DM.IndexKeys(pix, srs), DM.NativeIndex(ctx, IC.host_arrays(r1cs), srs)


def _fr(ctx, ptr, n):
    return ctx.download(ptr, (n, 4))


def _check_parity(ctx, r1cs, z, with_oracle=True):
    sq, zz, pkeys, nix = _both(ctx, r1cs, z)
    pix, view, info = pkeys.index, nix.view, nix.info
    try:
        want_info, _, _, want_zz = IC.oracle_shape(r1cs, z)
        assert info == want_info and want_zz == zz
        H, K, B = info["h_size"], info["k_size"], info["b_size"]
        assert (H, K, B, info["x_size"]) == (pix.dom_h.size, pix.dom_k.size, pix.dom_b.size, pix.dom_x.size)
        assert info["max_degree_needed"] == DM.ahp_max_degree(pix)
        assert (view.num_constraints, view.num_variables, view.num_non_zero, view.num_instance) == \
            (pix.num_constraints, pix.num_variables, pix.num_non_zero, pix.num_instance)
        # the twelve coefficient vectors: the oracle's, coefficient for coefficient, and the Python-built index's, word for word
        oracle = M.Index(sq).polynomials() if with_oracle else None
        python = pix.polynomials()
        for i, label in enumerate(DM.INDEX_LABELS):
            assert view.index_polys[i].n == K
            got = _fr(ctx, view.index_polys[i].ptr, K)
            assert oracle is None or cv.fr_from_mont(got) == oracle[label], label
            assert np.array_equal(got, _fr(ctx, python[label].ptr, K)), label
        for i, m in enumerate("abc"):
            ek, eb = pix.arith[m].evals_on_K, pix.arith[m].evals_on_B
            for part in PARTS:
                if part != "row_col":
                    assert np.array_equal(_fr(ctx, getattr(view.on_k[i], part), K), _fr(ctx, ek[part].ptr, K)), (m, part, "K")
                assert np.array_equal(_fr(ctx, getattr(view.on_b[i], part), B), _fr(ctx, eb[part].ptr, B)), (m, part, "B")
            assert view.on_k[i].row_col is None
        d_w, d_x = pix.w_evals_index()
        assert np.array_equal(ctx.download(view.w_idx, (H,), dtype=np.uint32), ctx.download(d_w, (H,), dtype=np.uint32))
        assert np.array_equal(ctx.download(view.x_idx, (H,), dtype=np.uint32), ctx.download(d_x, (H,), dtype=np.uint32))
        padded = nix.pad_assignment(ctx.upload(cv.fr_to_mont(z)))
        assert np.array_equal(_fr(ctx, padded.ptr, len(zz)), cv.fr_to_mont(zz))
        assert nix.ivk_bytes() == pkeys.ivk_bytes() and view.ivk_len == 24 + 12 * 195
    finally:
        nix.free()


@pytest.mark.parametrize("name", IC.GPU_MARLIN_SYSTEMS + IC.HAND_BUILT)
def test_index_equals_both_earlier_implementations(ctx, name):
    _check_parity(ctx, *IC.system(name))


def test_index_of_a_generated_system_with_three_instance_variables(ctx):
    r1cs, z = circuit_system((9, 2, 2), 4242)
    assert r1cs.num_instance == 3
    _check_parity(ctx, r1cs, z)


def test_index_where_the_transforms_on_k_take_several_passes(ctx):
    """|K| = 2^11: the inverse transforms run four at a time through a scratch buffer, as the forward ones on B do from |B| = 2^11
    on (n = 1000 below has |K| = 2^10, |B| = 2^12).  Against the Python-built index alone: the oracle's would take minutes."""
    r1cs, z = IC.system(2000)
    _check_parity(ctx, r1cs, z, with_oracle=False)


def test_the_c_built_index_reproduces_the_fixture(ctx):
    """n = 3 under the seeds of tests/golden/marlin_verify.json system 0: the fixture's ivk, its good proof byte for byte from
    zk_marlin_prove over zk_marlin_ix_view, its verifier key field by field from zk_marlin_vk_from_index; both verifiers accept."""
    from helpers import marlin_test_system
    system = MC.fixture()["systems"][0]
    assert system["system"] == 3
    rng = O.Prng(system["prng_seed"])
    r1cs, z = marlin_test_system(3, rng)
    beta, g_k, gg_k, h_k = rng.fr(), rng.fr(), rng.fr(), rng.fr()
    assert hex(beta) == system["srs"]["beta"] and hex(h_k) == system["srs"]["h_k"]
    srs = DM.UniversalSrs(ctx, system["max_degree"], beta, g_k, gg_k)
    nix = DM.NativeIndex(ctx, IC.host_arrays(r1cs), srs)
    try:
        want_vk = MC.vk_of(system)
        assert nix.ivk_bytes() == want_vk.ivk
        zpad = nix.pad_assignment(ctx.upload(cv.fr_to_mont(z)))
        proof = DM.prove_native(nix, zpad, Rng.from_seed(bytes.fromhex(system["prover_seed"]), 20))
        assert proof.hex() == system["variants"][0]["proof"]
        h = O.g2_mul(O.G2_GEN, h_k)
        vk = nix.verifier_key(cv.g2_affine_to_array([h])[0], cv.g2_affine_to_array([O.g2_mul(h, beta)])[0])
        assert bytes(vk.struct)[16:] == bytes(want_vk.struct)[16:] and vk.ivk == want_vk.ivk
        _, zz = M.pad_and_square(r1cs, z)
        inputs = cv.fr_to_mont(zz[1:nix.info["num_instance"]])
        assert DM.verify_host(vk, inputs, proof)
        assert DM.verify_batch(ctx, vk, inputs[None], [proof]).tolist() == [1]
    finally:
        nix.free()


@pytest.mark.parametrize("name", ["tiny11", "dense5", 1000])
def test_same_proof_bytes_as_from_the_python_built_index(ctx, name):
    r1cs, z = IC.system(name)
    sq, zz, pkeys, nix = _both(ctx, r1cs, z, extra=5)
    try:
        seed = bytes((11 * i + 5) & 0xff for i in range(32))
        zpad = nix.pad_assignment(ctx.upload(cv.fr_to_mont(z)))
        got = DM.prove_native(nix, zpad, Rng.from_seed(seed, 20))
        want = DM.prove_native(pkeys, ctx.upload(cv.fr_to_mont(zz)), Rng.from_seed(seed, 20))
        assert got == want
        h_k, beta = 0xabcdef, pkeys.srs.beta
        h = O.g2_mul(O.G2_GEN, h_k)
        vk = nix.verifier_key(cv.g2_affine_to_array([h])[0], cv.g2_affine_to_array([O.g2_mul(h, beta)])[0])
        pub = zz[1:sq.num_instance]
        wrong = [(pub[0] + 1) % O.R_MOD] + pub[1:]
        assert DM.verify_batch(ctx, vk, np.stack([cv.fr_to_mont(pub), cv.fr_to_mont(wrong)]), [got, got]).tolist() == [1, 0]
        if name == "tiny11":                # the collaborative prover with a single party reads the same struct
            from zk_mpc_amd import mpc
            party = mpc.Party(ctx, net=mpc.LocalNet.create(1)[0])
            shared = [party.marlin_prove_shared_native(k, zdev, Rng.from_seed(seed, 20))
                      for k, zdev in ((nix, zpad), (pkeys, ctx.upload(cv.fr_to_mont(zz))))]
            assert shared[0] == shared[1]
            assert DM.verify_batch(ctx, vk, cv.fr_to_mont(pub)[None], [shared[0]]).tolist() == [1]
    finally:
        nix.free()


def _raw_build(ctx, host, powers_g, want_out=True):
    out = C.c_void_p()
    rc = ctx.lib.zk_marlin_index_build(ctx.h, None if host is None else C.byref(host), powers_g, C.byref(out) if want_out else None)
    assert rc != 0 or out.value
    return rc, out


def test_refusals_leave_the_context_usable(ctx):
    """Every case the header lists is ZK_ERR_ARG (-2); afterwards a good build and proof succeed on the same context, and build,
    free, build again gives the same bytes."""
    r1cs, z = IC.system(6)
    ni, nw, a, b, c = IC.host_arrays(r1cs)
    sq, zz, pix = _python_index(ctx, r1cs, z)
    need = DM.ahp_max_degree(pix)
    srs = DM.UniversalSrs(ctx, need, 0x77, 3, 7)
    pg = srs.powers_g.h
    good, _k0 = ZM._r1cs_host(ni, nw, a, b, c)
    assert _raw_build(ctx, None, pg)[0] == -2
    assert _raw_build(ctx, good, None)[0] == -2
    assert _raw_build(ctx, good, pg, want_out=False)[0] == -2
    h, _k1 = ZM._r1cs_host(ni, nw, a, b, c)
    h.b_col = None
    assert _raw_build(ctx, h, pg)[0] == -2                                  # a null pointer inside the system
    rp = a[0].copy(); rp[0] = 1
    h, _k2 = ZM._r1cs_host(ni, nw, (rp, a[1], a[2]), b, c)
    assert _raw_build(ctx, h, pg)[0] == -2                                  # row_ptr does not start at 0
    rp = a[0].copy(); rp[2] = rp[1] - 1
    h, _k3 = ZM._r1cs_host(ni, nw, (rp, a[1], a[2]), b, c)
    assert _raw_build(ctx, h, pg)[0] == -2                                  # row_ptr decreases
    col = c[1].copy(); col[0] = ni + nw
    h, _k4 = ZM._r1cs_host(ni, nw, a, b, (c[0], col, c[2]))
    assert _raw_build(ctx, h, pg)[0] == -2                                  # a column that is no variable
    h, _k5 = ZM._r1cs_host(0, ni + nw, a, b, c)
    assert _raw_build(ctx, h, pg)[0] == -2                                  # num_instance = 0
    short = DM.UniversalSrs(ctx, need - 1, 0x77, 3, 7)
    assert _raw_build(ctx, good, short.powers_g.h)[0] == -2                 # IndexTooLarge
    assert b"IndexTooLarge" in ctx.lib.zk_last_error(ctx.h)
    # num_non_zero = 4 = |K|, but balancing hands B the four-entry row of A: seven entries
    from helpers import csr
    wide = (2, 4, csr([[(1, 0), (2, 1), (3, 2), (4, 3)], []]), csr([[(5, 4)], [(6, 1), (7, 2), (8, 3)]]), csr([[(9, 5)], []]))
    h, _k6 = ZM._r1cs_host(*wide)
    big = DM.UniversalSrs(ctx, 64, 0x77, 3, 7)
    assert _raw_build(ctx, h, big.powers_g.h)[0] == -2
    # the context works as before
    seed = bytes(range(32))
    proofs, ivks, polys = [], [], []
    for _ in range(2):
        nix = DM.NativeIndex(ctx, (ni, nw, a, b, c), srs)
        ivks.append(nix.ivk_bytes())
        polys.append(_fr(ctx, nix.view.index_polys[0].ptr, 12 * nix.info["k_size"]).copy())
        proofs.append(DM.prove_native(nix, nix.pad_assignment(ctx.upload(cv.fr_to_mont(z))), Rng.from_seed(seed, 20)))
        nix.free()
    assert ivks[0] == ivks[1] == DM.IndexKeys(pix, srs).ivk_bytes() and np.array_equal(polys[0], polys[1]) and proofs[0] == proofs[1]
