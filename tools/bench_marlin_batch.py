#!/usr/bin/env python3
"""Batch Marlin proving (zk_marlin_prove_batch: count proofs of one index in lock-step) against count calls of zk_marlin_prove one
after the other, on the mul-chain family with |H| = |K| = 2^L.

  python tools/bench_marlin_batch.py [--out profiles/marlin_prove_batch.jsonl] [--logs 10,12,14,16] [--counts 1,2,4,16,64] [--rounds 5]

Both run on the same context, index, SRS and assignments (count different assignments), the mask polynomial sampled on the device
as in bench.py's Marlin leg.  After a warm-up of each, a round times the loop and the batch one after the other with a host clock
around calls that return only when their proofs are written; the order rotates from round to round; a timed window repeats its call until it lasts 0.1 s.  A count whose round would
last longer than --budget seconds at the measured loop time is skipped.  One JSON line per (size, count): the median ms per proof of
each, the spread of each over the rounds (min, max), their ratio, and whether the proofs were the same bytes."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zk_mpc_amd as Z      # noqa: E402
from zk_mpc_amd import marlin as DM      # noqa: E402
from zk_mpc_amd.api import Rng      # noqa: E402


def median(ts):
    return sorted(ts)[len(ts) // 2]


def seed(k):
    return bytes((5 * k + i) & 0xff for i in range(32))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_prove_batch.jsonl"))
    ap.add_argument("--logs", default="10,12,14,16")
    ap.add_argument("--counts", default="1,2,4,16,64")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=60.0, help="seconds one (size, count) may take in all")
    a = ap.parse_args()
    ctx = Z.Context(0)
    m = DM.HostField.m
    rows = []
    for log_h in [int(x) for x in a.logs.split(",")]:
        n = (1 << log_h) - 3
        index = DM.Index(ctx, *DM.mul_chain_system(ctx, n))
        keys = DM.IndexKeys(index, DM.UniversalSrs(ctx, DM.ahp_max_degree(index) + 5, 0x1234567, 3, 7))
        nv = index.num_variables
        max_count = max(int(c) for c in a.counts.split(","))
        singles = [ctx.mul_chain_assignment_dev(n, m(3 + 2 * k), m(5 + 11 * k)) for k in range(max_count)]
        both = ctx.alloc(max_count * nv * 32)
        for k, z in enumerate(singles):
            ctx.memcpy_d2d(both.ptr + k * nv * 32, z.ptr, nv * 32)
        ctx.sync()
        ctx.pooling = True
        one_ms = None
        for count in [int(c) for c in a.counts.split(",")]:
            loop = lambda: [DM.prove_native(keys, singles[k], Rng.from_seed(seed(k), 20), mask_on_device=True) for k in range(count)]
            batch = lambda: DM.prove_native_batch(keys, both, nv, [Rng.from_seed(seed(k), 20) for k in range(count)], mask_on_device=True)
            if one_ms is not None and max(one_ms * count, 100.0) * 2.2 * (a.rounds + 1) / 1e3 > a.budget:
                print(json.dumps({"log_h": log_h, "count": count, "skipped": "a run would exceed %.0f s" % a.budget}), flush=True)
                continue
            same = loop() == batch()                                 # warm-up of both, and the contract
            t0 = time.perf_counter()
            loop()
            inner = max(1, int(0.1 / (time.perf_counter() - t0)))    # a timed window lasts 0.1 s at least
            t_loop, t_batch = [], []
            for r in range(a.rounds):
                order = ((loop, t_loop), (batch, t_batch)) if r % 2 == 0 else ((batch, t_batch), (loop, t_loop))
                for fn, ts in order:
                    ctx.sync()
                    t0 = time.perf_counter()
                    for _ in range(inner):
                        fn()
                    ts.append((time.perf_counter() - t0) * 1e3 / (count * inner))
            one_ms = median(t_loop)
            rows.append({"circuit": "mul_chain_2p%d" % log_h, "log_h": log_h, "count": count, "rounds": a.rounds, "calls_per_window": inner, "same_bytes": same,
                         "loop_ms_per_proof": round(median(t_loop), 4), "loop_min_max": [round(min(t_loop), 4), round(max(t_loop), 4)],
                         "batch_ms_per_proof": round(median(t_batch), 4), "batch_min_max": [round(min(t_batch), 4), round(max(t_batch), 4)],
                         "loop_over_batch": round(median(t_loop) / median(t_batch), 3)})
            print(json.dumps(rows[-1]), flush=True)
        ctx.pooling = False
        ctx.drop_pool()
        del index, keys, singles, both
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
