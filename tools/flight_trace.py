#!/usr/bin/env python3
"""Every way the Groth16 pipeline starts work ahead of a proof, once each on one context: the workload of a rocprofv3 --kernel-trace
run whose per-queue kernel sequence (tools/kernel_seq.py) is compared across a change that must not move a launch.
  rocprofv3 --kernel-trace -d DIR -o t --output-format csv -- python3 tools/flight_trace.py
Prints one sha per leg so that two runs can also be compared by their bytes."""
import hashlib
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import zk_mpc_amd as Z  # noqa: E402
import zk_mpc_amd.convert as cv  # noqa: E402

mont = lambda v: cv.fr_to_mont([v])[0]


def main():
    ctx = Z.Context(0)
    td = [mont(1000 + i) for i in range(1, 8)]
    legs = {}

    def key(n):
        dr = ctx.r1cs_mul_chain(n)
        return dr, ctx.groth16_setup(dr, *td), [ctx.mul_chain_assignment_dev(n, mont(100 + q), mont(201 + q)) for q in range(4)]

    def queue(name, dr, pk, zs, rounds=2):
        h = hashlib.sha256()
        for i in range(4 * rounds):
            ctx.groth16_hint_next_dev(zs[(i + 1) % 4].ptr if i + 1 < 4 * rounds else None)
            h.update(ctx.create_proof_dev(pk, dr, zs[i % 4].ptr, mont(7 + i % 4), mont(9 + i % 4)))
        legs[name] = h.hexdigest()[:16]

    def ahead(name, dr, pk, zs, D):
        hq = ctx.alloc(D * 32)
        ctx.witness_map_dev(dr, zs[0].ptr, hq.ptr)
        h = hashlib.sha256()
        for start in (ctx.groth16_msms_presort_dev, ctx.groth16_msms_begin_dev):
            start(pk, dr, zs[0].ptr)
            g1, g2 = ctx.groth16_msms_dev(pk, dr, zs[0].ptr, hq.ptr)
            h.update(g1.tobytes() + g2.tobytes())
        legs[name] = h.hexdigest()[:16]
        hq.free()

    for n, D, tag in (((1 << 10) - 2, 1 << 10, "2^10"), ((1 << 16) + 50, 1 << 17, "2^16+50"), ((1 << 20) - 2, 1 << 20, "2^20-2")):
        dr, pk, zs = key(n)
        if D == 1 << 10:
            ctx.groth16_chain_fronts(True)
            queue("queue %s chained" % tag, dr, pk, zs)
            ctx.groth16_chain_fronts(False)
            queue("queue %s unchained" % tag, dr, pk, zs)
            ctx.groth16_chain_fronts(True)
        else:
            queue("queue %s" % tag, dr, pk, zs, rounds=1)
        if D <= 1 << 17:
            ahead("presort, begin -> msms %s" % tag, dr, pk, zs, D)
        pk.free()
        dr.free()
        for z in zs:
            z.free()
    ctx.close()
    print(json.dumps(legs))


if __name__ == "__main__":
    main()
