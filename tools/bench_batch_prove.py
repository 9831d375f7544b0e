"""Time per proof of zk_groth16_prove_batch_dev against one context proving the same assignments back to back (create_proof_dev,
each call announcing the next assignment: chained fronts).  Mul-chain keys from zk_groth16_setup; the two forms alternate in one
process, every shape is warmed up first, and every proof's bytes are checked against the single-proof path.  One JSON line per
(size, count) on stdout and appended to profiles/batch_prove.jsonl.

    python tools/bench_batch_prove.py [--sizes 10,12,14,16] [--counts 1,4,16,64] [--reps 5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import zk_mpc_amd as Z  # noqa: E402
import zk_mpc_amd.convert as cv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="10,12,14,16")
    ap.add_argument("--counts", default="1,4,16,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_prove.jsonl"))
    a = ap.parse_args()
    rs = np.random.RandomState(2024)
    mont = lambda: cv.fr_to_mont([int.from_bytes(rs.bytes(31), "little")])[0]
    ctx = Z.Context(0)
    lines = []
    for log_n in [int(x) for x in a.sizes.split(",")]:
        n = (1 << log_n) - 4
        m = n + 3
        dr = ctx.r1cs_mul_chain(n)
        pk = ctx.groth16_setup(dr, *[mont() for _ in range(7)])
        for count in [int(x) for x in a.counts.split(",")]:
            zs = [ctx.mul_chain_assignment_dev(n, mont(), mont()) for _ in range(count)]
            dz = ctx.upload(np.concatenate([ctx.download(z, (m, 4)) for z in zs]))
            rl, sl = [mont() for _ in range(count)], [mont() for _ in range(count)]
            want = [ctx.create_proof_dev(pk, dr, zs[k].ptr, rl[k], sl[k]) for k in range(count)]

            def batch():
                return ctx.create_proofs_batch_dev(pk, dr, dz.ptr, count, rl, sl)

            def queue():
                out = []
                for k in range(count):
                    ctx.groth16_hint_next_dev(zs[k + 1].ptr if k + 1 < count else None)
                    out.append(ctx.create_proof_dev(pk, dr, zs[k].ptr, rl[k], sl[k]))
                return out

            for f in (batch, queue, batch, queue):          # warm-up: graphs, scratch, tables
                assert f() == want
            tb, tq = [], []
            for _ in range(a.reps):
                for f, t in ((batch, tb), (queue, tq)):
                    t0 = time.perf_counter()
                    got = f()
                    t.append((time.perf_counter() - t0) * 1e3 / count)
                    assert got == want, f.__name__
            rec = {"log_n": log_n, "constraints": n, "count": count, "reps": a.reps,
                   "batch_ms_per_proof": round(float(np.median(tb)), 4), "batch_ms_min": round(min(tb), 4),
                   "queue_ms_per_proof": round(float(np.median(tq)), 4), "queue_ms_min": round(min(tq), 4),
                   "speedup": round(float(np.median(tq) / np.median(tb)), 3), "bytes_checked": True}
            print(json.dumps(rec), flush=True)
            lines.append(rec)
            dz.free()
            for z in zs:
                z.free()
        pk.free()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as fh:
        for rec in lines:
            fh.write(json.dumps(rec) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
