#!/usr/bin/env python3
"""Groth16 verification of a 2^10 mul-chain key: the device path (zk_groth16_verify_batch), the host arithmetic
(zk_groth16_verify_host in a loop) and the oracle's verifier (oracle/zkref.py::verify_proof, pure Python), at counts 1, 64 and 1024.

  python tools/bench_verify.py [--out profiles/verify_batch.jsonl] [--host-max 64] [--oracle-max 2]

One JSON line per count: ms per call and per proof for the device path (median of --reps calls after a warm-up call), ms per proof
for the other two (measured on at most --host-max / --oracle-max proofs), and the ratio of the oracle's time per proof to the device's."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import zkref as O          # noqa: E402
import zk_mpc_amd as Z      # noqa: E402
import zk_mpc_amd.convert as cv      # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=64)
    ap.add_argument("--oracle-max", type=int, default=2)
    a = ap.parse_args()
    ctx = Z.Context(0)
    rng = O.Prng(0x5EED)
    mont1 = lambda v: cv.fr_to_mont([v])[0]
    n, m, top = (1 << 10) - 4, (1 << 10) - 1, 1024
    dr = ctx.r1cs_mul_chain(n)
    pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])
    host = np.concatenate([ctx.download(ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr())), (m, 4)) for _ in range(64)])
    host = np.tile(host.reshape(64, m, 4), (top // 64, 1, 1))
    rl, sl = [mont1(rng.fr()) for _ in range(top)], [mont1(rng.fr()) for _ in range(top)]
    proofs = ctx.create_proofs_batch(pk, dr, host, rl, sl)
    inputs = host[:, 1:2, :].copy()
    opk = SimpleNamespace(alpha_g1=cv.g1_array_to_affine(pk.vk_g1(0))[0], beta_g2=cv.g2_array_to_affine(pk.vk_g2(0))[0],
                          gamma_g2=cv.g2_array_to_affine(pk.vk_g2(2))[0], delta_g2=cv.g2_array_to_affine(pk.vk_g2(1))[0],
                          gamma_abc_g1=cv.g1_array_to_affine(pk.download("gamma_abc_g1")))
    g2_of = lambda b: cv.g2_array_to_affine(ctx.bases_deserialize_compressed(b, 1, 2).download())[0]
    rows = []
    for count in (1, 64, 1024):
        assert ctx.groth16_verify_batch(pk, inputs[:count], proofs[:count]).all()        # warm-up, and the verdicts
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            ctx.groth16_verify_batch(pk, inputs[:count], proofs[:count])
            ts.append((time.perf_counter() - t0) * 1e3)
        dev_ms = sorted(ts)[len(ts) // 2]
        nh = min(count, a.host_max)
        t0 = time.perf_counter()
        for k in range(nh):
            assert pk.verify_host(inputs[k], proofs[k])
        host_ms = (time.perf_counter() - t0) * 1e3 / nh
        no = min(count, a.oracle_max)
        t0 = time.perf_counter()
        for k in range(no):
            pr = proofs[k]
            pts = (O.g1_deserialize(pr[:48]), g2_of(pr[48:144]), O.g1_deserialize(pr[144:]))
            assert O.verify_proof(opk, pts, cv.fr_from_mont(inputs[k]))
        oracle_ms = (time.perf_counter() - t0) * 1e3 / no
        rows.append({"circuit": "mul_chain_2p10", "count": count, "device_ms_per_call": round(dev_ms, 3), "device_ms_per_proof": round(dev_ms / count, 4),
                     "host_ms_per_proof": round(host_ms, 3), "host_proofs_timed": nh, "oracle_ms_per_proof": round(oracle_ms, 1),
                     "oracle_proofs_timed": no, "oracle_over_device": round(oracle_ms / (dev_ms / count), 1)})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
