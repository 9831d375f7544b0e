#!/usr/bin/env python3
"""Groth16 verification of one batch over SEVERAL keys (zk_groth16_vkeys_verify_aggregate_coeffs: one folded pairing product for all
keys) against the baseline it replaces: the batch split by key and one zk_groth16_vkey_verify_aggregate_coeffs call per key.

  python tools/bench_verify_keys.py [--out profiles/verify_keys.jsonl] [--keys 1,4,16,64,256] [--counts 256,4096,65536] [--reps 3] [--ninp 2]

K keys with --ninp public inputs each (alpha .. delta shared, gamma_abc of their own: what the calls do does not depend on it), the
proofs dealt evenly (proof i belongs to key i mod K), forged from the trapdoor, their points from the fixed-base calls.  The loop is
given its sub-batches ready made: splitting the batch by key is not charged to it.  The several-key call and the loop ALTERNATE in one
process; the call runs under both settings of ZK_VFY_KEYS_MUL (the sum_k (ninp_k + 2) = (ninp + 2) K multiplications of key points on the host's
helper threads, or as one launch); the loop runs with the variable unset, so at K = 1 it is the same call under the library's own
rule.  One JSON line per (K, count): the median ms of each after a warm-up, the spread (max - min) of
each over its repetitions, and one profiled several-key call split into its phases (zk_set_profiling)."""
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
from zk_mpc_amd import api      # noqa: E402
import groth16_verify_cases as G      # noqa: E402

R = O.R_MOD
POOL = 16      # distinct proofs per key; a longer sub-batch repeats them


def median(ts):
    return sorted(ts)[len(ts) // 2]


def fixed_base(ctx, scalars, group, gen_k):
    d = ctx.upload(cv.fr_to_mont([s % R for s in scalars]))
    tb = ctx.fixed_base(d.ptr, len(scalars), group, cv.fr_to_mont([gen_k])[0])
    return tb, d


def make_keys(ctx, base, n_keys, NINP, rng):
    """n_keys resident keys with base's alpha .. delta and gamma_abc[j] = k_j G, and gamma_abc's logs as G.forge reads them"""
    keys = []
    for _ in range(n_keys):
        ks = [G.nonzero(rng) for _ in range(NINP + 1)]
        tb, d = fixed_base(ctx, ks, 1, 1)
        vk = dict(base.vk, gamma_abc_g1=tb.download())
        tb.free()
        d.free()
        keys.append(SimpleNamespace(vkey=ctx.vkey_upload(**vk), pks=SimpleNamespace(gamma_abc=[k * G.inv(base.td.g1_k) % R for k in ks])))
    return keys


def make_pool(ctx, base, keys, NINP, rng):
    """POOL valid proofs per key -> inputs (K, POOL, NINP, 4), proofs (K, POOL, 192)"""
    xs, abcs = [], []
    for k in keys:
        for _ in range(POOL):
            x = [rng.fr() for _ in range(NINP)]
            xs.append(x)
            abcs.append(G.forge(k.pks, base.td, x, rng)[0])
    cols = []
    for which, group, gen_k in ((0, 1, base.td.g1_k), (1, 2, base.td.g2_k), (2, 1, base.td.g1_k)):
        tb, d = fixed_base(ctx, [abc[which] for abc in abcs], group, gen_k)
        cols.append(np.frombuffer(tb.serialize(compressed=True), dtype=np.uint8).reshape(len(abcs), 48 * group))
        tb.free()
        d.free()
    proofs = np.ascontiguousarray(np.concatenate(cols, axis=1)).reshape(len(keys), POOL, 192)
    return G.inputs_mont(xs).reshape(len(keys), POOL, NINP, 4), proofs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_keys.jsonl"))
    ap.add_argument("--keys", default="1,4,16,64,256")
    ap.add_argument("--counts", default="256,4096,65536")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--ninp", type=int, default=2)
    a = ap.parse_args()
    n_keys = [int(c) for c in a.keys.split(",")]
    counts = [int(c) for c in a.counts.split(",")]
    ctx = Z.Context(0)
    rng = O.Prng(0x4B455953)
    base = G.host_key(2)
    NINP = a.ninp
    keys = make_keys(ctx, base, max(n_keys), NINP, rng)
    pool_in, pool_pr = make_pool(ctx, base, keys, NINP, rng)
    rows = []
    for count in counts:
        for K in n_keys:
            if K > count:
                continue
            key_of = np.arange(count, dtype=np.uint32) % K
            nth = np.arange(count) // K % POOL                       # which pool proof of its key
            inputs = np.ascontiguousarray(pool_in[key_of, nth]).reshape(-1, 4)
            proofs = np.ascontiguousarray(pool_pr[key_of, nth]).tobytes()
            coeffs = api.verify_aggregate_coeffs_from_seed(os.urandom(32), count)
            vkeys = [k.vkey for k in keys[:K]]
            subs = []
            for k in range(K):
                rows_k = np.nonzero(key_of == k)[0]
                subs.append((vkeys[k], np.ascontiguousarray(pool_in[k, nth[rows_k]]), np.ascontiguousarray(pool_pr[k, nth[rows_k]]).tobytes(),
                             np.ascontiguousarray(coeffs[rows_k])))

            def several(mode):
                os.environ["ZK_VFY_KEYS_MUL"] = mode
                return ctx.verify_keys_aggregate(vkeys, key_of, inputs, proofs, coeffs=coeffs)

            def loop():
                os.environ.pop("ZK_VFY_KEYS_MUL", None)      # the single-key calls as a caller gets them: the rule decides
                return all([ctx.groth16_verify_aggregate(v, i, p, coeffs=c)[0] for v, i, p, c in subs])

            assert several("host")[0] is True and several("dev")[0] is True and loop() is True      # warm-up, and the verdicts
            ts = {"host": [], "dev": [], "loop": []}
            for _ in range(a.reps):
                for name in ("host", "loop", "dev"):
                    t0 = time.perf_counter()
                    (loop if name == "loop" else lambda: several(name))()
                    ts[name].append((time.perf_counter() - t0) * 1e3)
            phases = {}
            for mode in ("host", "dev"):
                ctx.set_profiling(True)
                ctx.timers()
                several(mode)
                phases[mode] = {k.split(".", 1)[1]: round(v[0], 3) for k, v in ctx.timers().items() if k.startswith("verify_aggregate.")}
                ctx.set_profiling(False)
            os.environ.pop("ZK_VFY_KEYS_MUL", None)
            med = {k: median(v) for k, v in ts.items()}
            rows.append({"keys": K, "count": count, "ninp": NINP, "key_mul_terms": (NINP + 2) * K, "reps": a.reps,
                         "several_keys_mul_host_ms": round(med["host"], 3), "several_keys_mul_dev_ms": round(med["dev"], 3),
                         "loop_of_single_key_ms": round(med["loop"], 3),
                         "spread_ms": {k: round(max(v) - min(v), 3) for k, v in ts.items()},
                         "loop_over_several_keys": round(med["loop"] / min(med["host"], med["dev"]), 2),
                         "phases_ms": phases})
            print(json.dumps(rows[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
