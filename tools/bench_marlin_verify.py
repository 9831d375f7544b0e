#!/usr/bin/env python3
"""Marlin verification of the fixture's "tiny7" system (|H| = 16, |K| = 32, three public inputs; the verifier's work does not depend on
the system's size): the device path (zk_marlin_verify_batch), the host arithmetic (zk_marlin_verify_host in a loop) and the oracle's
verifier (oracle/marlin_full_ref.py, pure Python) at counts 1, 64 and 1024.  A batch is the fixture's accepted proof repeated with every
eighth replaced by a rejected variant.

  python tools/bench_marlin_verify.py [--out profiles/marlin_verify_batch.jsonl] [--host-max 8] [--reps 5]

One JSON line per count: ms per call and per proof for the device path (median of --reps calls after a warm-up call), the split of one
profiled call (host: parse, the wait for the decompressed points, the equation builders; device: the decompression, the linear-combination
kernel, the pairing kernels), ms per proof for the other two, and the per-proof ratios host / device and oracle / device."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import zk_mpc_amd as Z      # noqa: E402
import zk_mpc_amd.marlin as DM      # noqa: E402
import marlin_verify_cases as MC      # noqa: E402


def oracle_ms(system, v):
    keys = MC.oracle_keys(system)
    t0 = time.perf_counter()
    assert MC.oracle_verdict(keys, v) == 1
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_verify_batch.jsonl"))
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-max", type=int, default=8)
    a = ap.parse_args()
    ctx = Z.Context(0)
    system = MC.fixture()["systems"][1]
    vk = MC.vk_of(system)
    good = MC.variant_args(system["variants"][0])
    bad = MC.variant_args(next(v for v in system["variants"] if v["name"] == "eval_z_b_plus_1"))
    o_ms = oracle_ms(system, system["variants"][0])
    rows = []
    for count in (1, 64, 1024):
        picks = [bad if k % 8 == 7 else good for k in range(count)]
        inputs, proofs, want = np.stack([p[0] for p in picks]), [p[1] for p in picks], [p[2] for p in picks]
        assert DM.verify_batch(ctx, vk, inputs, proofs).tolist() == want        # warm-up, and the verdicts
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            DM.verify_batch(ctx, vk, inputs, proofs)
            ts.append((time.perf_counter() - t0) * 1e3)
        dev_ms = sorted(ts)[len(ts) // 2]
        ctx.set_profiling(True)
        ctx.timers()
        DM.verify_batch(ctx, vk, inputs, proofs)
        split = {k.split(".", 1)[1]: round(v[0], 3) for k, v in ctx.timers().items() if k.startswith("marlin_verify.")}
        ctx.set_profiling(False)
        nh = min(count, a.host_max)
        t0 = time.perf_counter()
        for k in range(nh):
            assert int(DM.verify_host(vk, inputs[k], proofs[k])) == want[k]
        host_ms = (time.perf_counter() - t0) * 1e3 / nh
        rows.append({"system": "tiny7", "count": count, "device_ms_per_call": round(dev_ms, 3), "device_ms_per_proof": round(dev_ms / count, 4),
                     "split_ms": split, "host_ms_per_proof": round(host_ms, 3), "host_proofs_timed": nh, "oracle_ms_per_proof": round(o_ms, 1),
                     "host_over_device": round(host_ms / (dev_ms / count), 1), "oracle_over_device": round(o_ms / (dev_ms / count), 1)})
        print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
