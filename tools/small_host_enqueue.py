#!/usr/bin/env python3
"""One context, a hinted queue of small proofs with the phase timers on: host.enqueue per proof and the sha of all proof bytes."""
import hashlib, json, os, sys, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
L, K = int(sys.argv[1]), int(sys.argv[2])
n = (1 << L) - 2
mont = lambda v: cv.fr_to_mont([v])[0]
ctx = Z.Context(0)
dr = ctx.r1cs_mul_chain(n)
pk = ctx.groth16_setup(dr, *[mont(1000 + i) for i in range(1, 8)])
zs = [ctx.mul_chain_assignment_dev(n, mont(100 + 10 * q), mont(101 + 10 * q)) for q in range(4)]
rs = (mont(200), mont(201))
h = hashlib.sha256()
for i in range(8):
    ctx.create_proof_dev(pk, dr, zs[i % 4].ptr, *rs)
ctx.set_profiling(True)
ctx.timers()
t0 = time.perf_counter()
for i in range(K):
    ctx.groth16_hint_next_dev(zs[(i + 1) % 4].ptr)
    h.update(ctx.create_proof_dev(pk, dr, zs[i % 4].ptr, *rs))
dt = time.perf_counter() - t0
t = ctx.timers()
ctx.set_profiling(False)
ctx.groth16_hint_next_dev(None)
ms, cnt = t.get("host.enqueue", (0.0, 0))
print(json.dumps({"groth16_log": L, "proofs": K, "host_enqueue_ms_per_proof": round(ms / max(cnt, 1), 5), "host_enqueue_count": cnt,
                  "profiled_ms_per_proof": round(dt / K * 1e3, 4), "proof_sha": h.hexdigest()[:16]}))
pk.free()
ctx.close()
