"""Time per proof of the collaborative batch prover (zk_groth16_prove_shared_batch) against a loop of count single calls
(zk_groth16_prove_shared) over the same shares.  Parties are threads on one GPU over mpc.LocalNet -- its exchange is a Python barrier
between threads, not a network: what the batch saves on a real mesh (count - 1 round trips of every exchange) is NOT in these
figures, only the device and host time.  Mul-chain keys from zk_groth16_setup; the two forms alternate in one process, every shape
is warmed up by one round of each, the median of `reps` rounds is taken (the loop's fastest round is kept beside it), and the
batch's bytes are checked against the loop's.  One JSON line per (parties, size, count): ms per proof, exchanges per call and
bytes_sent, both ways -- on stdout and appended to profiles/shared_batch.jsonl.

    python tools/bench_shared_batch.py [--parties 1,3] [--sizes 10,12,14] [--counts 1,8,64] [--reps 5] [--timeout 300]

Every (parties, size) is a child process of its own under a time limit; the run stops at the first one that fails.
"""
import argparse
import json
import os
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def share_of(ctx, p, n_parties, dz, m, ni, seed):
    """Party p's additive share of the assignment at dz (input generation): the instance on the leader, the witness as pseudo-random
    residues on parties 0 .. N-2 (every party derives them from the seed) and the difference on the last."""
    import numpy as np
    z = ctx.download(dz, (m, 4))

    def rnd(q):
        t = np.random.RandomState((seed * 1000 + q) & 0x7FFFFFFF).randint(0, 1 << 62, size=(m - ni, 4), dtype=np.int64).astype(np.uint64)
        t[:, 3] &= np.uint64((1 << 60) - 1)          # < 2^252 < r: a valid residue
        return t
    mine = np.zeros((m, 4), dtype=np.uint64)
    if p < n_parties - 1:
        mine[ni:] = rnd(p)
    else:
        acc = ctx.upload(np.ascontiguousarray(z[ni:]))
        for q in range(n_parties - 1):
            s = ctx.upload(rnd(q))
            ctx.fr_vec_op_dev(2, acc.ptr, s.ptr, acc.ptr, m - ni)
            ctx.sync()
            s.free()
        mine[ni:] = ctx.download(acc, (m - ni, 4))
        acc.free()
    if p == 0:
        mine[:ni] = z[:ni]
    return mine


def run_cell(n_parties, log_n, counts, reps):
    """One (parties, size): every count, one JSON line each on stdout."""
    import numpy as np
    import zk_mpc_amd as Z
    import zk_mpc_amd.convert as cv
    from zk_mpc_amd import mpc

    n = (1 << log_n) - 4
    m = n + 3
    rs = np.random.RandomState(2024 + log_n)
    rnd = lambda: int.from_bytes(rs.bytes(31), "little")
    td = cv.fr_to_mont([rnd() for _ in range(7)])
    top = max(counts)
    ws = [(cv.fr_to_mont([rnd()])[0], cv.fr_to_mont([rnd()])[0]) for _ in range(top)]
    rsv = [(rnd(), rnd()) for _ in range(top)]
    nets = mpc.LocalNet.create(n_parties)
    sync = threading.Barrier(n_parties)
    recs, err = {}, []

    def work(p):
        ctx = Z.Context(0, p, n_parties)
        try:
            party = mpc.Party(ctx, net=nets[p])
            dr = ctx.r1cs_mul_chain(n)
            pk = ctx.groth16_setup(dr, *[td[i] for i in range(7)])
            shares, rl, sl = [], [], []
            for k in range(top):                     # input generation: this party's share of every assignment and scalar
                dz = ctx.mul_chain_assignment_dev(n, *ws[k])
                shares.append(share_of(ctx, p, n_parties, dz, m, 2, 100 + k))
                r_k, s_k = party.share_scalars(rsv[k], 500 + k)
                rl.append(r_k)
                sl.append(s_k)
                dz.free()
            calls = {"small": 0, "vec": 0}
            gather, open_vec = nets[p].all_gather_small, party.be.open_vec

            def counted_gather(*a, **kw):
                calls["small"] += 1
                return gather(*a, **kw)

            def counted_open(*a, **kw):
                calls["vec"] += 1
                return open_vec(*a, **kw)
            nets[p].all_gather_small, party.be.open_vec = counted_gather, counted_open
            for count in counts:
                dzs = ctx.upload(np.concatenate(shares[:count]))

                def batch():
                    return party.create_proofs_shared_native(pk, dr, dzs.ptr, rl[:count], sl[:count])

                def loop():
                    return [party.create_proof_shared_native(pk, dr, dzs.ptr + k * m * 32, rl[k], sl[k]) for k in range(count)]

                def timed(f):
                    calls.update(small=0, vec=0)
                    sent0 = party.bytes_sent
                    sync.wait()
                    t0 = time.perf_counter()
                    got = f()
                    ms = (time.perf_counter() - t0) * 1e3 / count
                    return got, ms, calls["small"] + calls["vec"], party.bytes_sent - sent0

                want = timed(loop)[0]                # warm-up: graphs, scratch, tables
                assert timed(batch)[0] == want, "batch bytes differ from the loop's"
                tb, tl = [], []
                for _ in range(reps):
                    for f, t in ((batch, tb), (loop, tl)):
                        got, ms, exchanges, sent = timed(f)
                        assert got == want, f.__name__
                        t.append((ms, exchanges, sent))
                if p == 0:
                    med = lambda t: round(float(np.median([x[0] for x in t])), 4)
                    recs[count] = {"parties": n_parties, "log_n": log_n, "constraints": n, "count": count, "reps": reps,
                                   "batch_ms_per_proof": med(tb), "batch_ms_min": round(min(x[0] for x in tb), 4),
                                   "loop_ms_per_proof": med(tl), "loop_ms_min": round(min(x[0] for x in tl), 4),
                                   "speedup": round(med(tl) / med(tb), 3),
                                   "batch_exchanges_per_call": tb[0][1], "loop_exchanges_per_call": tl[0][1] // count,
                                   "loop_exchanges_total": tl[0][1], "batch_bytes_sent": tb[0][2], "loop_bytes_sent": tl[0][2],
                                   "transport": "LocalNet (threads, Python barrier)", "bytes_checked": True}
                dzs.free()
        except Exception as e:
            import traceback
            err.append("party %d: %s\n%s" % (p, e, traceback.format_exc()))
            sync.abort()
            try:
                nets[p].sh.barrier.abort()
            except Exception:
                pass
        finally:
            ctx.close()

    ts = [threading.Thread(target=work, args=(p,)) for p in range(n_parties)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if err:
        sys.exit("\n".join(err))
    for count in counts:
        print(json.dumps(recs[count]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parties", default="1,3")
    ap.add_argument("--sizes", default="10,12,14")
    ap.add_argument("--counts", default="1,8,64")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--timeout", type=int, default=300, help="seconds for one (parties, size)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_batch.jsonl"))
    ap.add_argument("--cell", default=None, help="internal: parties,log_n of the one cell this process runs")
    a = ap.parse_args()
    counts = [int(x) for x in a.counts.split(",")]
    if a.cell:
        n_parties, log_n = [int(x) for x in a.cell.split(",")]
        return run_cell(n_parties, log_n, counts, a.reps)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for n_parties in [int(x) for x in a.parties.split(",")]:
        for log_n in [int(x) for x in a.sizes.split(",")]:
            cmd = [sys.executable, os.path.abspath(__file__), "--cell", "%d,%d" % (n_parties, log_n), "--counts", a.counts, "--reps", str(a.reps)]
            try:
                r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=a.timeout)
            except subprocess.TimeoutExpired:
                sys.exit("P = %d, 2^%d: no result within %d s; stopping" % (n_parties, log_n, a.timeout))
            if r.returncode != 0:
                sys.exit("P = %d, 2^%d: exit status %d; stopping" % (n_parties, log_n, r.returncode))
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            with open(a.out, "a") as fh:
                fh.write(r.stdout)


if __name__ == "__main__":
    main()
