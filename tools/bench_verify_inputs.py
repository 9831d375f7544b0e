#!/usr/bin/env python3
"""Groth16 verification against the number of public inputs: zk_groth16_verify_batch and zk_groth16_verify_aggregate_coeffs of this
tree's library against another build of the library (the parent commit's), in ONE process, alternating the two.

  python tools/bench_verify_inputs.py --parent-lib /path/to/parent/libzkmpc_hip.so [--out profiles/verify_inputs.jsonl]
         [--ninps 1,8,64,512,4096] [--counts 1,64,4096] [--reps 3]

Per (ninp, count) the order is parent, branch, parent: the two parent figures show the spread of the call itself.  A figure is the
median of --reps calls after a warm-up call (one call where the warm-up took more than --slow-ms).  The key is groth16_verify_cases'
system with ninp + 1 instance variables, set up from its trapdoor by each library; the proofs are forged from the trapdoor (valid:
the verdicts are asserted), one proof repeated count times.  One JSON line per cell; the last line has the key load times."""
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
from zk_mpc_amd import _lib, api      # noqa: E402
from helpers import csr, mont1, td_mont      # noqa: E402
import groth16_verify_cases as G      # noqa: E402


def context_on(path):
    """a Context whose calls go to the library at `path` (symbols that library lacks are left without prototypes)"""
    lib = C.CDLL(path)
    for name, (res, args) in _lib.PROTOTYPES.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = res, args
    _lib._lib = lib
    return Z.Context(0)


def timed(fn, reps, slow_ms):
    t0 = time.perf_counter()
    fn()
    first = (time.perf_counter() - t0) * 1e3
    ts = []
    for _ in range(1 if first > slow_ms else reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_inputs.jsonl"))
    ap.add_argument("--ninps", default="1,8,64,512,4096")
    ap.add_argument("--counts", default="1,64,4096")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slow-ms", type=float, default=500.0)
    a = ap.parse_args()
    ctxs = {"branch": context_on(_lib.LIB_PATH), "parent": context_on(a.parent_lib)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    out = open(a.out, "w")

    def emit(row):
        print(json.dumps(row), flush=True)
        out.write(json.dumps(row) + "\n")
        out.flush()

    for ninp in [int(v) for v in a.ninps.split(",")]:
        k = G.host_key(ninp + 1)
        rng = O.Prng(0xBE7C + ninp)
        x = [rng.fr() for _ in range(ninp)]
        abc, _ = G.forge(k.pks, k.td, x, rng)
        proof = np.frombuffer(G.proof_bytes(k.td, abc), dtype=np.uint8)
        pks, first_ms = {}, {}
        for name, ctx in ctxs.items():
            dr = ctx.r1cs_upload(k.r1cs.num_instance, k.r1cs.num_witness, csr(k.r1cs.a), csr(k.r1cs.b), csr(k.r1cs.c))
            pks[name] = ctx.groth16_setup(dr, *td_mont(k.td))
            one = G.inputs_mont([x])
            t0 = time.perf_counter()
            assert ctx.groth16_verify_batch(pks[name], one, proof.tobytes()).tolist() == [1]
            first_ms[name] = round((time.perf_counter() - t0) * 1e3, 3)      # (branch: with the key's vkey and its window table)
        vk_bytes = O.vk_serialize(k.opk)
        t0 = time.perf_counter()
        ctxs["branch"].vkey_deserialize(vk_bytes).free()
        load_ms = (time.perf_counter() - t0) * 1e3
        emit({"ninp": ninp, "first_verify_ms": first_ms, "vkey_load_ms": round(load_ms, 3), "vkey_load_ms_per_input": round(load_ms / ninp, 4)})
        for count in [int(v) for v in a.counts.split(",")]:
            inp = np.ascontiguousarray(np.broadcast_to(G.inputs_mont([x]), (count, ninp, 4)))
            blob = np.tile(proof, count).tobytes()
            coeffs = api.verify_aggregate_coeffs_from_seed(bytes(range(32)), count)
            row = {"ninp": ninp, "count": count}
            for run, name in (("parent_1", "parent"), ("branch", "branch"), ("parent_2", "parent")):
                ctx, pk = ctxs[name], pks[name]
                assert ctx.groth16_verify_batch(pk, inp, blob).all() and ctx.groth16_verify_aggregate(pk, inp, blob, coeffs=coeffs)[0]
                row[run + "_batch_ms"] = round(timed(lambda: ctx.groth16_verify_batch(pk, inp, blob), a.reps, a.slow_ms), 3)
                row[run + "_aggregate_ms"] = round(timed(lambda: ctx.groth16_verify_aggregate(pk, inp, blob, coeffs=coeffs), a.reps, a.slow_ms), 3)
            for form in ("batch", "aggregate"):
                row[form + "_parent_over_branch"] = round(min(row["parent_1_%s_ms" % form], row["parent_2_%s_ms" % form]) / row["branch_%s_ms" % form], 2)
            emit(row)
        for name in ctxs:
            pks[name].free()
    out.close()
    for ctx in ctxs.values():
        ctx.close()


if __name__ == "__main__":
    main()
