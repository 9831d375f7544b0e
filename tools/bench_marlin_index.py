#!/usr/bin/env python3
"""Marlin::index on one GPU, two ways on one box: the path through Python (zk_mpc_amd.marlin.Index + IndexKeys on the padded
system: gathers, scales and products call by call, twelve inverse and twelve forward transforms one at a time, one MSM batch) and the
library's one call (zk_marlin_index_build on the system as the circuit gives it: NativeIndex).

Systems: the mul-chain filling |H| = 2^16 and 2^20 (|K| = |H|), and a circuit-shaped system with |K| = 4 |H| at |H| = 2^16.  The two
paths alternate; after a warm-up pair the median of --reps builds of each is reported, with the split of the C call (host wall-clock
per phase, the device's work included: zk_set_profiling) from one more build.  One JSON line per system; --out appends them to a file.

  python tools/bench_marlin_index.py [--systems chain16,chain20,circuit16] [--reps 5] [--out profiles/marlin_index.jsonl]
"""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    sys.path.insert(0, p)
import zk_mpc_amd.marlin as DM  # noqa: E402
from zk_mpc_amd.api import Context  # noqa: E402


def chain(log_h):
    """The mul-chain whose padded square form fills |H| = 2^log_h, as the circuit gives it: (ni, nw, a, b, c)."""
    n = (1 << log_h) - 3
    idx = lambda j: np.where(j <= n, 2 + j, 1).astype(np.uint32)
    i = np.arange(n, dtype=np.int64)
    rp = np.arange(n + 1, dtype=np.uint32)
    ones = np.tile(DM.HostField.m(1), (n, 1))
    return 2, n + 1, (rp, idx(i), ones), (rp, idx(i + 1), ones), (rp, idx(i + 2), ones)


def circuit(log_h, seed=16):
    import synth_r1cs as S
    from helpers import csr
    ni, nw, a, b, c, _ = S.sized_for_domain(log_h, seed)
    return ni, nw, csr(a), csr(b), csr(c)


def padded(ni, nw, a, b, c):
    """The same system padded and square, as Index takes it (what oracle/marlin_ref.py::pad_and_square does, on the arrays)."""
    extra = DM._next_pow2(ni) - ni
    nc = len(a[0]) - 1
    size = max(nc, ni + extra + nw)

    def one(m):
        rp, col, co = m
        col = np.where(col < ni, col, col + extra).astype(np.uint32)
        rp = np.concatenate([rp, np.full(size - nc, rp[-1], dtype=np.uint32)])
        return DM.Csr(rp, col, co)
    return ni + extra, size - ni - extra, one(a), one(b), one(c)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", default="chain16,chain20,circuit16")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = Context(0)
    for name in args.systems.split(","):
        log_h = int(name[-2:])
        host = chain(log_h) if name.startswith("chain") else circuit(log_h)
        sq = padded(*host)
        info = DM.shape_info(*host)
        srs = DM.UniversalSrs(ctx, info["max_degree_needed"], 0x5eed, 1, 7)
        ctx.sync()

        def python_path():
            t0 = time.perf_counter()
            index = DM.Index(ctx, *sq)
            index.w_evals_index()
            keys = DM.IndexKeys(index, srs)
            ivk = keys.ivk_bytes()
            ctx.sync()
            dt = time.perf_counter() - t0
            index.r1cs.free()
            index.r1cs_t.free()
            return dt, ivk

        def c_path():
            t0 = time.perf_counter()
            nix = DM.NativeIndex(ctx, host, srs)
            ivk = nix.ivk_bytes()
            dt = time.perf_counter() - t0
            nix.free()
            return dt, ivk

        times = {"python": [], "c": []}
        for rep in range(args.reps + 1):
            for label, fn in (("python", python_path), ("c", c_path)):
                dt, ivk = fn()
                gc.collect()
                if rep:
                    times[label].append(dt)
                times[label + "_ivk"] = ivk
        assert times["python_ivk"] == times["c_ivk"], "the two paths disagree on the index verifier key"
        ctx.set_profiling(True)
        c_path()
        split = {k.split(".", 1)[1]: round(v[0], 3) for k, v in ctx.timers().items() if k.startswith("marlin_index.")}
        ctx.set_profiling(False)
        med = {k: statistics.median(times[k]) for k in ("python", "c")}
        line = {"system": name, "h_size": info["h_size"], "k_size": info["k_size"], "b_size": info["b_size"], "reps": args.reps,
                "python_index_s": round(med["python"], 4), "c_index_s": round(med["c"], 4), "factor": round(med["python"] / med["c"], 2),
                "python_all_s": [round(x, 4) for x in times["python"]], "c_all_s": [round(x, 4) for x in times["c"]],
                "c_split_ms": split}
        print(json.dumps(line), flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(json.dumps(line) + "\n")
        del srs
        gc.collect()
    ctx.close()


if __name__ == "__main__":
    main()
