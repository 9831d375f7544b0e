#!/usr/bin/env python3
"""Collaborative Marlin in batches (zk_marlin_prove_shared_batch / _spdz_batch: count proofs of one index in lock-step, the exchanges of
one proof per chunk) against count calls of zk_marlin_prove_shared[_spdz] one after the other, on the mul-chain family with
|H| = |K| = 2^L.

  python tools/bench_marlin_shared_batch.py [--out profiles/marlin_shared_batch.jsonl] [--logs 10,12,14] [--counts 1,2,4,16,64]
                                            [--modes additive,spdz] [--parties 1,3] [--rounds 5] [--budget 40] [--append]

The parties are threads of this process, each with a context of its own on device 0, over LocalNet.  The loop and the batch run on the
same contexts, index, SRS and shares (party 0 holds the assignments, the others shares of zero: the work does not depend on the
values), the mask polynomial sampled on the device.  After a warm-up of each, a round times the loop and the batch one after the other
with a host clock at party 0 around calls that return only when their proofs are written; the order rotates from round to round; a
timed window repeats its call until it lasts 0.1 s.  What the parties must agree on (calls per window, a skipped cell) is party 0's
and travels over the same net.  A cell whose run would last longer than --budget seconds at the measured loop time is skipped.  One
JSON line per (mode, parties, size, count): the median ms per proof of each, the spread of each over the rounds (min, max), their
ratio, whether the batch is faster by more than the loop's own spread, and whether the proofs were the same bytes.

--laps LOG,COUNT,MODE,PARTIES adds one line for that cell from the library's host laps of one batch call at party 0: the share of the
call inside exchanges (small opens, vector opens, the Beaver product with its two opens) and, of the small opens, the part that is not
the transport's -- validating and summing what the peers sent."""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import zk_mpc_amd as Z      # noqa: E402
from zk_mpc_amd import marlin as DM      # noqa: E402
from zk_mpc_amd import mpc      # noqa: E402
from zk_mpc_amd.api import Rng      # noqa: E402


def median(ts):
    return sorted(ts)[len(ts) // 2]


def seed(p, k):
    return bytes((5 * k + 29 * p + i) & 0xff for i in range(32))


def party_main(p, n_parties, net, a, spdz, rows, errors):
    ctx = Z.Context(0, p, n_parties)
    try:
        party = (mpc.SpdzParty if spdz else mpc.Party)(ctx, net=net)
        m = DM.HostField.m
        counts = [int(c) for c in a.counts.split(",")]
        agree = lambda v: net.exchange(v)[0]              # party 0's value, at every party
        for log_h in [int(x) for x in a.logs.split(",")]:
            n = (1 << log_h) - 3
            index = DM.Index(ctx, *DM.mul_chain_system(ctx, n))
            keys = DM.IndexKeys(index, DM.UniversalSrs(ctx, DM.ahp_max_degree(index) + 5, 0x1234567, 3, 7))
            nv = index.num_variables
            both = ctx.alloc(max(counts) * nv * 32)
            ctx.dev_zero(both.ptr, max(counts) * nv * 32)
            for k in range(max(counts) if p == 0 else 0):
                z = ctx.mul_chain_assignment_dev(n, m(3 + 2 * k), m(5 + 11 * k))
                ctx.memcpy_d2d(both.ptr + k * nv * 32, z.ptr, nv * 32)
            ctx.sync()
            ctx.pooling = True
            z_of = lambda k: both.ptr + k * nv * 32
            one_ms = None
            for count in counts:
                rngs = lambda: [Rng.from_seed(seed(p, k), 20) for k in range(count)]
                if spdz:            # MAC key 1: the MAC lane of a value is a sharing of the value itself
                    loop = lambda: [party.marlin_prove_shared_spdz_native(keys, (z_of(k), z_of(k)), r, mask_on_device=True) for k, r in enumerate(rngs())]
                    batch = lambda: party.marlin_prove_shared_spdz_batch_native(keys, (both, both), nv, rngs(), mask_on_device=True)
                else:
                    loop = lambda: [party.marlin_prove_shared_native(keys, z_of(k), r, mask_on_device=True) for k, r in enumerate(rngs())]
                    batch = lambda: party.marlin_prove_shared_batch_native(keys, both, nv, rngs(), mask_on_device=True)
                cell = {"mode": "spdz" if spdz else "additive", "parties": n_parties, "circuit": "mul_chain_2p%d" % log_h, "log_h": log_h, "count": count}
                skip = agree(one_ms is not None and max(one_ms * count, 100.0) * 2.2 * (a.rounds + 1) / 1e3 > a.budget)
                if skip:
                    if p == 0:
                        rows.append(dict(cell, skipped="a run would exceed %.0f s" % a.budget))
                        print(json.dumps(rows[-1]), flush=True)
                    continue
                same = loop() == batch()                                 # warm-up of both, and the contract
                t0 = time.perf_counter()
                loop()
                inner = agree(max(1, int(0.1 / (time.perf_counter() - t0))))    # a timed window lasts 0.1 s at least
                t_loop, t_batch = [], []
                for r in range(a.rounds):
                    order = ((loop, t_loop), (batch, t_batch)) if r % 2 == 0 else ((batch, t_batch), (loop, t_loop))
                    for fn, ts in order:
                        ctx.sync()
                        net.barrier()
                        t0 = time.perf_counter()
                        for _ in range(inner):
                            fn()
                        ts.append((time.perf_counter() - t0) * 1e3 / (count * inner))
                one_ms = agree(median(t_loop))
                if p == 0:
                    rows.append(dict(cell, rounds=a.rounds, calls_per_window=inner, same_bytes=same,
                                     loop_ms_per_proof=round(median(t_loop), 4), loop_min_max=[round(min(t_loop), 4), round(max(t_loop), 4)],
                                     batch_ms_per_proof=round(median(t_batch), 4), batch_min_max=[round(min(t_batch), 4), round(max(t_batch), 4)],
                                     loop_over_batch=round(median(t_loop) / median(t_batch), 3),
                                     faster_beyond_spread=bool(median(t_loop) - median(t_batch) > max(t_loop) - min(t_loop))))
                    print(json.dumps(rows[-1]), flush=True)
                if a.laps == "%d,%d,%s,%d" % (log_h, count, "spdz" if spdz else "additive", n_parties):
                    gather, in_gather = net.all_gather_small, [0.0]

                    def timed_gather(*args, **kw):
                        t = time.perf_counter()
                        try:
                            return gather(*args, **kw)
                        finally:
                            in_gather[0] += (time.perf_counter() - t) * 1e3
                    net.all_gather_small = timed_gather
                    ctx.set_profiling(True)
                    ctx.timers()                                          # (drop what earlier calls left)
                    net.barrier()
                    t0 = time.perf_counter()
                    batch()
                    call_ms = (time.perf_counter() - t0) * 1e3
                    tm = {k: v for k, v in ctx.timers().items() if k.startswith("marlin_shared.")}
                    ctx.set_profiling(False)
                    net.all_gather_small = gather
                    if p == 0:
                        ms = lambda k: float(tm[k][0]) if k in tm and isinstance(tm[k], (tuple, list)) else float(tm.get(k, 0.0))
                        small, vec, beaver = ms("marlin_shared.small_open"), ms("marlin_shared.vec_open"), ms("marlin_shared.beaver")
                        rows.append(dict(cell, laps=True, call_ms=round(call_ms, 3), small_open_ms=round(small, 3), vec_open_ms=round(vec, 3),
                                         beaver_ms=round(beaver, 3), gather_callbacks_ms=round(in_gather[0], 3),
                                         share_in_exchanges=round((small + vec + beaver) / call_ms, 3),
                                         share_validating_peers=round(max(small - in_gather[0], 0.0) / call_ms, 3)))
                        print(json.dumps(rows[-1]), flush=True)
            ctx.pooling = False
            ctx.drop_pool()
            del index, keys, both
    except Exception as e:      # a party that stops must not leave the others waiting
        import traceback
        errors.append("party %d: %s\n%s" % (p, e, traceback.format_exc()))
        try:
            net.sh.barrier.abort()
        except Exception:
            pass
    finally:
        ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "marlin_shared_batch.jsonl"))
    ap.add_argument("--logs", default="10,12,14")
    ap.add_argument("--counts", default="1,2,4,16,64")
    ap.add_argument("--modes", default="additive,spdz")
    ap.add_argument("--parties", default="1,3")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--budget", type=float, default=40.0, help="seconds one cell may take in all")
    ap.add_argument("--append", action="store_true", help="add to --out instead of writing it anew")
    ap.add_argument("--laps", default="10,64,spdz,3", help="LOG,COUNT,MODE,PARTIES: the cell whose host laps are reported (empty: none)")
    a = ap.parse_args()
    rows, errors = [], []
    for mode in a.modes.split(","):
        for n_parties in [int(x) for x in a.parties.split(",")]:
            nets = mpc.LocalNet.create(n_parties)
            ts = [threading.Thread(target=party_main, args=(p, n_parties, nets[p], a, mode == "spdz", rows, errors)) for p in range(n_parties)]
            [t.start() for t in ts]
            [t.join() for t in ts]
            if errors:
                sys.exit("\n".join(errors))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a" if a.append else "w") as f:
        for r in rows:
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
