#!/usr/bin/env python3
"""Aggregated Groth16 verification (zk_groth16_verify_aggregate_coeffs: one folded pairing product per batch) against
zk_groth16_verify_batch_checked (one equation per proof, the same subgroup tests), on the proofs of tools/bench_verify.py: a 2^10
mul-chain key, 1024 proofs from zk_groth16_prove_batch, repeated to the larger counts.

  python tools/bench_verify_aggregate.py [--out profiles/verify_aggregate.jsonl] [--counts 1,64,1024,16384,65536] [--reps 5]

The two entry points alternate in one process.  One JSON line per count: the median ms per call of each after a warm-up call, the
spread (max - min) of each over its repetitions, their ratio, and one profiled aggregate call split into its phases (zk_set_profiling: device time by events for the kernels, host
wall-clock for the host parts)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import zkref as O          # noqa: E402
import zk_mpc_amd as Z      # noqa: E402
import zk_mpc_amd.convert as cv      # noqa: E402
from zk_mpc_amd import api      # noqa: E402


def median(ts):
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_aggregate.jsonl"))
    ap.add_argument("--counts", default="1,64,1024,16384,65536")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    counts = [int(c) for c in a.counts.split(",")]
    ctx = Z.Context(0)
    rng = O.Prng(0x5EED)
    mont1 = lambda v: cv.fr_to_mont([v])[0]
    n, m, made = (1 << 10) - 4, (1 << 10) - 1, 1024
    dr = ctx.r1cs_mul_chain(n)
    pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])
    host = np.concatenate([ctx.download(ctx.mul_chain_assignment_dev(n, mont1(rng.fr()), mont1(rng.fr())), (m, 4)) for _ in range(64)])
    host = np.tile(host.reshape(64, m, 4), (made // 64, 1, 1))
    rl, sl = [mont1(rng.fr()) for _ in range(made)], [mont1(rng.fr()) for _ in range(made)]
    made_proofs = b"".join(ctx.create_proofs_batch(pk, dr, host, rl, sl))
    made_inputs = host[:, 1:2, :].copy()
    rows = []
    for count in counts:
        reps = (count + made - 1) // made
        proofs = (made_proofs * reps)[:count * 192]
        inputs = np.tile(made_inputs, (reps, 1, 1))[:count].copy()
        coeffs = api.verify_aggregate_coeffs_from_seed(os.urandom(32), count)
        agg = lambda: ctx.groth16_verify_aggregate(pk, inputs, proofs, coeffs=coeffs)
        chk = lambda: ctx.groth16_verify_batch(pk, inputs, proofs, check_subgroup=True)
        assert agg()[0] is True and chk().all()              # warm-up, and the verdicts
        t_agg, t_chk = [], []
        for _ in range(a.reps):
            for fn, ts in ((agg, t_agg), (chk, t_chk)):
                t0 = time.perf_counter()
                fn()
                ts.append((time.perf_counter() - t0) * 1e3)
        ctx.set_profiling(True)
        ctx.timers()
        agg()
        phases = {k.split(".", 1)[1]: round(v[0], 3) for k, v in ctx.timers().items() if k.startswith("verify_aggregate.")}
        ctx.set_profiling(False)
        rows.append({"circuit": "mul_chain_2p10", "count": count, "aggregate_ms": round(median(t_agg), 3), "checked_batch_ms": round(median(t_chk), 3),
                     "checked_over_aggregate": round(median(t_chk) / median(t_agg), 2), "aggregate_us_per_proof": round(median(t_agg) / count * 1e3, 2),
                     "reps": a.reps, "spread_ms": {"aggregate": round(max(t_agg) - min(t_agg), 3), "checked_batch": round(max(t_chk) - min(t_chk), 3)},
                     "aggregate_phases_ms": phases})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
