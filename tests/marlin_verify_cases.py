"""Shared by tests/test_marlin_verify_host.py and tests/test_gpu_marlin_verify.py: the fixture tests/golden/marlin_verify.json as
verifier keys and (inputs, proof, verdict) triples, and the seam cases of the segmented G1 linear combination with their
expected sums from the oracle (computed once per session)."""
import ctypes as C
import functools
import json
import os

import numpy as np

import zkref as O
import zk_mpc_amd.convert as cv
import zk_mpc_amd.marlin as DM
from zk_mpc_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = O.R_MOD


@functools.lru_cache(maxsize=None)
def fixture():
    with open(os.path.join(ROOT, "tests", "golden", "marlin_verify.json")) as f:
        return json.load(f)


def _g1(p):
    return cv.g1_affine_to_array([(int(p[0], 16), int(p[1], 16))])[0]


def _g2(p):
    return cv.g2_affine_to_array([((int(p[0][0], 16), int(p[0][1], 16)), (int(p[1][0], 16), int(p[1][1], 16)))])[0]


def vk_of(system) -> DM.VerifierKey:
    k = system["key"]
    return DM.VerifierKey.from_parts(bytes.fromhex(k["ivk_bytes"]), _g1(k["g"]), _g1(k["gamma_g"]), _g2(k["h"]), _g2(k["beta_h"]),
                                     _g1(k["shift_h"]), _g1(k["shift_k"]))


def variant_args(v):
    """(inputs as (n, 4) Montgomery, proof bytes, verdict)"""
    return cv.fr_to_mont([int(x, 16) for x in v["inputs"]]), bytes.fromhex(v["proof"]), v["verdict"]


def oracle_keys(system):
    """The fixture's key as the oracle's verifier takes it (marlin_full_ref.Keys over the recorded index commitments)."""
    import marlin_full_ref as MF
    import marlin_ref as M
    k = system["key"]
    pt = lambda p: (int(p[0], 16), int(p[1], 16))
    pt2 = lambda p: ((int(p[0][0], 16), int(p[0][1], 16)), (int(p[1][0], 16), int(p[1][1], 16)))

    class PP:
        pass
    pp = PP()
    pp.g, pp.gamma_g, pp.h, pp.beta_h, pp.beta = pt(k["g"]), pt(k["gamma_g"]), pt2(k["h"]), pt2(k["beta_h"]), int(system["srs"]["beta"], 16)
    ivk = bytes.fromhex(k["ivk_bytes"])
    nv, nc, nnz = (int.from_bytes(ivk[8 * i:8 * i + 8], "little") for i in range(3))
    info = M.IndexInfo(nc, nnz, system["num_instance"])
    info.num_variables, info.num_constraints, info.num_non_zero = nv, nc, nnz
    comms = {}
    for i, l in enumerate(MF.INDEX_LABELS):
        c = ivk[24 + 195 * i:24 + 195 * (i + 1)]
        comms[l] = (int.from_bytes(c[:48], "little"), int.from_bytes(c[48:96], "little"))
    keys = MF.Keys(info, pp, max_degree=system["max_degree"], index_comms=comms)
    assert keys.ivk_bytes() == ivk
    assert keys.shift_power(keys.bounds["g_1"]) == pt(k["shift_h"]) and keys.shift_power(keys.bounds["g_2"]) == pt(k["shift_k"])
    return keys


def oracle_verdict(keys, v) -> int:
    import marlin_full_ref as MF
    return int(MF.verify(keys, [int(x, 16) for x in v["inputs"]], MF.proof_deserialize(bytes.fromhex(v["proof"]))))


# ---- the segmented linear combination ------------------------------------------------------------------------------------------------

def scalar_words(k: int) -> list:
    assert 0 <= k < 1 << 256
    return [(k >> (32 * i)) & 0xffffffff for i in range(8)]


SEAM_SCALARS = [0, 1, 2, R - 1, R, 1 << 252, (1 << 256) - 1,
                int("7" * 64, 16),                 # every window the largest positive digit
                int("8" * 64, 16),                 # every window -8 with a carry into the next
                int("f" * 64, 16) >> 4,            # all-ones windows under a zero top window
                (1 << 255) + 0x8000_0000_0000_0001]


@functools.lru_cache(maxsize=None)
def lincomb_cases():
    """(points (n, 12) uint64, point_index, scalars (terms, 8) uint32, seg_offsets, expected affine points).  Segments:
    every seam scalar alone on a point; infinity as a term; (P, k) twice (the tree's doubling case); (P, k) and (P, r - k)
    (cancels to infinity); an empty segment; lengths 1, 2, 31, 32, 33, 63, 64; then 40, 40, 40 (would straddle waves unless
    the packing pads) and a final one-term segment."""
    rng = O.Prng(0x11c0b)
    pts = [O.g1_mul(O.G1_GEN, rng.fr()) for _ in range(6)] + [None]
    INF = len(pts) - 1
    segs = [[(0, k)] for k in SEAM_SCALARS]
    segs.append([(INF, 5), (1, 7)])
    segs.append([(INF, R - 1)])
    k = rng.fr()
    segs.append([(2, k), (2, k)])
    segs.append([(2, k), (2, R - k)])
    segs.append([])
    small = lambda: rng.u64() & 0xffff       # short scalars keep the oracle's side of the long segments quick
    for n in (1, 2, 31, 32, 33, 63, 64, 40, 40, 40):
        segs.append([(int(rng.u64() % 6), rng.fr() if i % 16 == 0 else small()) for i in range(n)])
    segs.append([(3, (1 << 256) - 1 - small())])
    idx, ks, off, want = [], [], [0], []
    for s in segs:
        acc = None
        for p, kk in s:
            idx.append(p)
            ks.append(scalar_words(kk))
            acc = O.g1_add(acc, O.g1_mul(pts[p], kk) if pts[p] is not None else None)
        off.append(len(idx))
        want.append(acc)
    return (cv.g1_affine_to_array(pts), np.array(idx, dtype=np.uint32), np.array(ks, dtype=np.uint32).reshape(-1, 8),
            np.array(off, dtype=np.uint32), want)


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def lincomb(points, idx, ks, off, ctx=None):
    """zk_diag_g1_lincomb_host (ctx None) / _dev: (return code, (n_segments, 12) uint64)"""
    points, idx, ks, off = (np.ascontiguousarray(a) for a in (points, idx, ks, off))
    out = np.zeros((len(off) - 1, 12), dtype=np.uint64)
    lib = _lib.load()
    if ctx is None:
        rc = lib.zk_diag_g1_lincomb_host(_p(points), len(points), _p(idx), _p(ks), _p(off), len(off) - 1, _p(out))
    else:
        rc = lib.zk_diag_g1_lincomb_dev(ctx.h, _p(points), len(points), _p(idx), _p(ks), _p(off), len(off) - 1, _p(out))
    return rc, out


OFF_WIT_GAMMA = 901          # the second opening witness inside the 951-byte proof


@functools.lru_cache(maxsize=None)
def cofactor_torsion_point():
    """T = r P for a curve point P outside the prime-order subgroup: on the curve, of order dividing the cofactor."""
    x = 0x5eed
    while True:
        y = O.fq_sqrt((x * x % O.Q_MOD * x + 1) % O.Q_MOD)
        if y is not None:
            T = O.ec_mul_raw((x, y), R, O.FqOps)
            if T is not None:
                return T
        x += 1


def witness_plus_torsion(system):
    """(inputs, proof) of the accepted proof with W_gamma replaced by W_gamma + T.  W_gamma is not absorbed into the transcript and
    the pairing does not see T (e(T, Q) = 1), so both pairing equations still hold: only the subgroup test r P = O rejects it."""
    inputs, proof, verdict = variant_args(system["variants"][0])
    assert verdict == 1
    W = O.g1_deserialize(proof[OFF_WIT_GAMMA:OFF_WIT_GAMMA + 48])
    moved = O.g1_serialize(O.g1_add(W, cofactor_torsion_point()))
    return inputs, proof[:OFF_WIT_GAMMA] + moved + proof[OFF_WIT_GAMMA + 48:]
