"""CPU: Marlin::verify through the host arithmetic (zk_marlin_verify_host) against the fixture of oracle verdicts
(tests/golden/marlin_verify.json, tools/gen_marlin_verify_golden.py), and the per-term multiplication of the segmented G1 linear
combination (csrc/g1_lincomb.cuh, instantiated for the host by zk_diag_g1_lincomb_host) against the oracle's group law."""
import ctypes as C

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from zk_mpc_amd import _lib
import marlin_verify_cases as MC

ZK_ERR_ARG = -2


def test_err_arg_is_the_headers():
    import os
    import re
    text = open(os.path.join(MC.ROOT, "include", "zkmpc_hip.h")).read()
    assert int(re.search(r"#define ZK_ERR_ARG\s+(-?\d+)", text).group(1)) == ZK_ERR_ARG


@pytest.mark.parametrize("si", [0, 1])
def test_host_verifier_gives_every_fixture_verdict(si):
    system = MC.fixture()["systems"][si]
    vk = MC.vk_of(system)
    verdicts = [v["verdict"] for v in system["variants"]]
    assert verdicts[0] == 1 and 0 in verdicts
    got = {}
    for v in system["variants"]:
        inputs, proof, want = MC.variant_args(v)
        got[v["name"]] = (int(DM.verify_host(vk, inputs, proof)), want)
    assert all(g == w for g, w in got.values()), got


def test_fixture_entries_rederived_with_the_oracle():
    """Two entries live (proof_deserialize + verify on the fixture's key): the fixture cannot rot."""
    system = MC.fixture()["systems"][0]
    keys = MC.oracle_keys(system)
    by_name = {v["name"]: v for v in system["variants"]}
    for name in ("good", "eval_z_b_plus_1"):
        assert MC.oracle_verdict(keys, by_name[name]) == by_name[name]["verdict"], name


def test_caller_errors_are_err_arg():
    system = MC.fixture()["systems"][0]
    lib = _lib.load()
    inputs, proof, _ = MC.variant_args(system["variants"][0])
    buf = np.frombuffer(proof, dtype=np.uint8)
    ok = C.c_int(7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def call(vk, inp=inputs, n=None, pr=p(buf), okp=C.byref(ok)):
        return lib.zk_marlin_verify_host(C.byref(vk.struct) if vk is not None else None, p(inp), inp.shape[0] if n is None else n, pr, len(proof), okp)
    good = MC.vk_of(system)
    assert call(good) == 0 and ok.value == 1
    assert call(None) == ZK_ERR_ARG
    assert call(good, pr=None) == ZK_ERR_ARG
    assert call(good, okp=None) == ZK_ERR_ARG
    k = system["key"]
    parts = [bytes.fromhex(k["ivk_bytes"]), MC._g1(k["g"]), MC._g1(k["gamma_g"]), MC._g2(k["h"]), MC._g2(k["beta_h"]), MC._g1(k["shift_h"]), MC._g1(k["shift_k"])]

    def with_part(i, val):
        q = list(parts)
        q[i] = val
        return DM.VerifierKey.from_parts(*q)
    assert call(with_part(0, parts[0][:-1])) == ZK_ERR_ARG                       # ivk_len
    assert call(with_part(0, parts[0][:24 + 96] + b"\x01" + parts[0][24 + 97:])) == ZK_ERR_ARG      # an index commitment at infinity
    off = parts[1].copy(); off[0] ^= np.uint64(1)
    assert call(with_part(1, off)) == ZK_ERR_ARG                                 # g not on the curve
    assert call(with_part(5, np.zeros(12, np.uint64))) == ZK_ERR_ARG             # a shift power at infinity
    assert call(with_part(3, np.full(24, 0xffffffffffffffff, np.uint64))) == ZK_ERR_ARG     # h not canonical
    big = cv.fr_raw([O.R_MOD])                                                   # the words of r: not below r
    assert call(good, inp=big) == ZK_ERR_ARG
    assert ok.value == 1                                                         # untouched by the refused calls


def test_lincomb_host_matches_the_oracle_on_the_seams():
    points, idx, ks, off, want = MC.lincomb_cases()
    rc, out = MC.lincomb(points, idx, ks, off)
    assert rc == 0
    got = cv.g1_array_to_affine(out)
    bad = [s for s in range(len(want)) if got[s] != want[s]]
    assert not bad, (bad, [int(off[s + 1] - off[s]) for s in bad])
    assert any(w is None for w in want) and sum(w is not None for w in want) > 20


def test_lincomb_refuses_what_it_cannot_take():
    points, idx, ks, off, _ = MC.lincomb_cases()
    one_pt = np.zeros(65, np.uint32)
    k65 = np.ones((65, 8), np.uint32)
    assert MC.lincomb(points, one_pt, k65, np.array([0, 65], np.uint32))[0] == ZK_ERR_ARG       # 65 terms
    assert MC.lincomb(points, one_pt[:64], k65[:64], np.array([0, 64], np.uint32))[0] == 0
    assert MC.lincomb(points, np.array([len(points)], np.uint32), k65[:1], np.array([0, 1], np.uint32))[0] == ZK_ERR_ARG    # index
    assert MC.lincomb(points, one_pt[:2], k65[:2], np.array([0, 2, 1], np.uint32))[0] == ZK_ERR_ARG                         # decreasing
    assert MC.lincomb(points, one_pt[:2], k65[:2], np.array([1, 2], np.uint32))[0] == ZK_ERR_ARG


def test_subgroup_test_is_what_rejects_a_witness_moved_by_cofactor_torsion():
    """W_gamma + T with T of order dividing the cofactor: the pairing cannot see T (e(T, h) = 1, checked here through the host
    pairing), and the witness is in no transcript, so the two equations hold as for the accepted proof -- the verdict 0 is the
    subgroup test's, which the reference's Proof::deserialize makes."""
    from zk_mpc_amd import api
    system = MC.fixture()["systems"][0]
    T = MC.cofactor_torsion_point()
    assert O.ec_mul_raw(T, O.R_MOD, O.FqOps) is not None and (T[1] * T[1] - T[0] ** 3 - 1) % O.Q_MOD == 0
    gt = api.pairing_products_host(cv.g1_affine_to_array([T]), MC._g2(system["key"]["h"])[None], 1)
    assert _lib.load().zk_gt_is_one(gt.ctypes.data_as(C.c_void_p)) == 1
    inputs, proof = MC.witness_plus_torsion(system)
    vk = MC.vk_of(system)
    assert DM.verify_host(vk, *MC.variant_args(system["variants"][0])[:2])
    assert not DM.verify_host(vk, inputs, proof)
