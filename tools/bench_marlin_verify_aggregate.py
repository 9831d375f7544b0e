#!/usr/bin/env python3
"""Aggregated Marlin verification on the device (zk_marlin_verify_aggregate_coeffs: one folded KZG check per batch) against
zk_marlin_verify_batch (two pairing equations per proof), on the four accepted proofs of tests/golden/marlin_aggregate.json under the key
of tests/golden/marlin_verify.json's first system, cycled to the count; and the kernel of the long sum alone in its two modes.

  python tools/bench_marlin_verify_aggregate.py [--out profiles/marlin_verify_aggregate.jsonl] [--counts 1,64,1024,16384] [--reps 5]
                                                [--ab-counts 1024,16384]

The two entry points alternate in one process, through the C ABI with their arguments built once (the wall time of the CALL).  One JSON
line per count: the median ms per call of each after a warm-up call, the min-max spread of each, whether the aggregate is faster by more
than the larger spread (the pass mark at count 1 024), and one profiled aggregate call split into its phases (zk_set_profiling:
device time by events for the k_ phases, host wall-clock for the laps).
Then one line per A/B size: k_g1_term_fold in FULL and GLV mode through zk_diag_g1_term_sum_dev over 13 count + 16 lanes, alternating,
the kernel and its sum-down by device events, median and spread."""
import argparse
import ctypes as C
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
import zk_mpc_amd.marlin as DM      # noqa: E402
from zk_mpc_amd import api      # noqa: E402
import marlin_aggregate_cases as AC      # noqa: E402


def median(ts):
    return sorted(ts)[len(ts) // 2]


def spread(ts):
    return max(ts) - min(ts)


def entry_points(ctx, count, reps):
    vk = AC.vk()
    inputs, proofs = AC.cycled(count)
    n, inp, p_inp, p_buf, p_off, _keep = DM._batch_args(inputs, proofs)
    co = api.verify_aggregate_coeffs_from_seed(os.urandom(32), 2 * count)
    ok_all, each = C.c_int(0), np.zeros(count, dtype=np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)

    def agg():
        rc = ctx.lib.zk_marlin_verify_aggregate_coeffs(ctx.h, C.byref(vk.struct), n, p_inp, inp.shape[1], p_buf, p_off, p(co), C.byref(ok_all), None)
        assert rc == 0 and ok_all.value == 1

    def batch():
        rc = ctx.lib.zk_marlin_verify_batch(ctx.h, C.byref(vk.struct), n, p_inp, inp.shape[1], p_buf, p_off, p(each))
        assert rc == 0 and each.all()
    agg()                                                   # warm-up, and the verdicts
    batch()
    t_agg, t_batch = [], []
    for _ in range(reps):
        for fn, ts in ((agg, t_agg), (batch, t_batch)):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
    ctx.set_profiling(True)
    ctx.timers()
    agg()
    phases = {k.split(".", 1)[1]: round(v[0], 3) for k, v in ctx.timers().items() if k.startswith("marlin_verify_agg.")}
    batch()
    batch_phases = {k.split(".", 1)[1]: round(v[0], 3) for k, v in ctx.timers().items() if k.startswith("marlin_verify.")}
    ctx.set_profiling(False)
    margin = max(spread(t_agg), spread(t_batch))
    return {"bench": "marlin_verify_aggregate", "system": "marlin_verify.json[0]", "count": count, "aggregate_ms": round(median(t_agg), 3),
            "batch_ms": round(median(t_batch), 3), "aggregate_spread_ms": round(spread(t_agg), 3), "batch_spread_ms": round(spread(t_batch), 3),
            "batch_over_aggregate": round(median(t_batch) / median(t_agg), 2), "aggregate_us_per_proof": round(median(t_agg) / count * 1e3, 2),
            "aggregate_faster_beyond_spread": bool(median(t_batch) - median(t_agg) > margin), "reps": reps, "aggregate_phases_ms": phases,
            "batch_phases_ms": batch_phases}


def term_kernel_ab(ctx, count, reps):
    lanes = 13 * count + 16
    rng = O.Prng(0xab1e)
    base = cv.g1_affine_to_array([O.g1_mul(O.G1_GEN, rng.fr()) for _ in range(16)])
    pts = base[np.arange(lanes) % 16]
    gen = np.random.default_rng(7)
    full = gen.integers(0, 1 << 32, size=(lanes, 8), dtype=np.uint64).astype(np.uint32)
    full[:, 7] &= (1 << 28) - 1                             # below 2^252: a reduced scalar, what the entry point feeds
    glv = gen.integers(0, 1 << 32, size=(lanes, 8), dtype=np.uint64).astype(np.uint32)
    glv[:, 3] &= (1 << 31) - 1                              # halves below 2^127, what host64_glv_split gives for k < r
    glv[:, 7] &= (1 << 31) - 1
    modes = (("full", DM.TERM_FULL, full), ("glv", DM.TERM_GLV, glv))
    for _, mode, words in modes:
        DM.diag_g1_term_sum(ctx, pts, words, mode, scaled=False)
    ts = {"full": [], "glv": []}
    ctx.set_profiling(True)
    for _ in range(reps):
        for name, mode, words in modes:
            ctx.timers()
            DM.diag_g1_term_sum(ctx, pts, words, mode, scaled=False)
            ts[name].append(ctx.timers()["diag_term_sum.k_term_fold_" + name][0])
    ctx.set_profiling(False)
    margin = max(spread(ts["full"]), spread(ts["glv"]))
    return {"bench": "k_g1_term_fold_ab", "lanes": lanes, "full_ms": round(median(ts["full"]), 3), "glv_ms": round(median(ts["glv"]), 3),
            "full_spread_ms": round(spread(ts["full"]), 3), "glv_spread_ms": round(spread(ts["glv"]), 3),
            "full_over_glv": round(median(ts["full"]) / median(ts["glv"]), 2),
            "glv_not_slower_beyond_spread": bool(median(ts["glv"]) <= median(ts["full"]) + margin), "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_verify_aggregate.jsonl"))
    ap.add_argument("--counts", default="1,64,1024,16384")
    ap.add_argument("--ab-counts", default="1024,16384")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    ctx = Z.Context(0)
    rows = []
    for count in [int(c) for c in a.counts.split(",") if c]:
        rows.append(entry_points(ctx, count, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    for count in [int(c) for c in a.ab_counts.split(",") if c]:
        rows.append(term_kernel_ab(ctx, count, a.reps))
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
