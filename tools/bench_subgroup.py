#!/usr/bin/env python3
"""Subgroup membership on the device (csrc/subgroup.hip) against what there was before it.

  python tools/bench_subgroup.py [--out profiles/subgroup_check.jsonl] [--log-n 16] [--key-log 20] [--reps 5] [--only tables]
  rocprofv3 --kernel-trace --stats -d DIR -o sg --output-format csv -- python tools/bench_subgroup.py --only tables --out /dev/null
  python tools/bench_subgroup.py --kernel-stats DIR/.../sg_kernel_stats.csv        # appends the kernel line to --out; no device

One JSON line per measurement, the median of --reps after a warm-up, the two sides of a comparison alternating:
  g1_table      2^log_n G1 points.  check_ms: zk_bases_subgroup_check on the resident table (one launch of k_subgroup, a 4-byte copy
                back).  The parent's only device route to the same verdict is one-term segments with the scalar r through
                zk_diag_g1_lincomb_dev (how zk_marlin_verify_batch tests its points); it has no resident form, so the two are also
                timed as whole calls from host points (upload + check against the lincomb call, which moves a scalar and an index
                per point in and a point per point out besides).
  g1_kernels    the per-point comparison the pass mark is about, from the kernel trace of a run of this script: device time per launch
                of k_subgroup<G1> and of k_g1_lincomb over the same 2^log_n points (--kernel-stats)
  g2_table      2^log_n G2 points: the kernel (there was no device route), beside the host form's time per point
  verify        zk_groth16_verify_batch against _checked at count 1, 64 and 1024 on the D = 8 key of tests/golden/groth16.json with the
                oracle's predicted proofs (verification does not depend on the circuit's size: one public input, three pairings)
  pk_check      zk_pk_check_subgroups on the 2^key_log mul-chain key beside zk_pk_deserialize of the same key's uncompressed bytes
                (--key-log 0 skips it)
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle")):
    sys.path.insert(0, p)


def med(ts):
    return sorted(ts)[len(ts) // 2]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def alternate(reps, *fns):
    """each fn once as a warm-up, then reps rounds of all of them in turn -> the medians (ms)"""
    for f in fns:
        f()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for k, f in enumerate(fns):
            ts[k].append(timed(f))
    return [med(t) for t in ts]


def kernel_line(path, log_n):
    """the g1_kernels line from a rocprofv3 kernel-stats csv of a `--only tables` run"""
    rows = {}
    for r in csv.DictReader(open(path)):
        name = r["Name"]
        if "k_subgroup<zk::FqField" in name:
            rows["new"] = r
        elif "k_subgroup<zk::Fq2Field" in name:
            rows["g2"] = r
        elif "k_g1_lincomb" in name:
            rows["old"] = r
    n = 1 << log_n
    us = lambda r: float(r["AverageNs"]) / 1e3
    return {"what": "g1_kernels", "points": n, "k_subgroup_g1_us_per_launch": round(us(rows["new"]), 1), "k_subgroup_g1_launches": int(rows["new"]["Calls"]),
            "k_g1_lincomb_us_per_launch": round(us(rows["old"]), 1), "k_g1_lincomb_launches": int(rows["old"]["Calls"]),
            "lincomb_over_subgroup": round(us(rows["old"]) / us(rows["new"]), 2),
            "k_subgroup_g2_us_per_launch": round(us(rows["g2"]), 1), "k_subgroup_g2_launches": int(rows["g2"]["Calls"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "subgroup_check.jsonl"))
    ap.add_argument("--log-n", type=int, default=16)
    ap.add_argument("--key-log", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="tables: the two table measurements alone")
    ap.add_argument("--kernel-stats", default="", help="append the g1_kernels line from this rocprofv3 kernel-stats csv and stop")
    a = ap.parse_args()
    if a.kernel_stats:
        row = kernel_line(a.kernel_stats, a.log_n)
        print(json.dumps(row))
        with open(a.out, "a") as f:
            f.write(json.dumps(row) + "\n")
        return

    import zkref as O
    import zk_mpc_amd as Z
    import zk_mpc_amd.convert as cv
    import zk_mpc_amd.serialize as S
    from zk_mpc_amd import api
    ctx = Z.Context(0)
    rng = O.Prng(0x5B6B)
    mont1 = lambda v: cv.fr_to_mont([v])[0]
    rows = []

    def emit(row):
        rows.append(row)
        print(json.dumps(row), flush=True)

    n = 1 << a.log_n
    # ---- tables: multiples of the generators made on the device
    scal = ctx.alloc(n * 32)
    ctx.fr_powers_dev(mont1(rng.fr()), mont1(rng.fr()), n, scal.ptr)
    t1, t2 = ctx.fixed_base(scal.ptr, n, 1, mont1(1)), ctx.fixed_base(scal.ptr, n, 2, mont1(1))
    pts1 = t1.download()
    r_words = np.tile(np.array([(O.R_MOD >> (32 * i)) & 0xFFFFFFFF for i in range(8)], dtype=np.uint32), (n, 1))
    idx, off = np.arange(n, dtype=np.uint32), np.arange(n + 1, dtype=np.uint32)
    out = np.zeros((n, 12), dtype=np.uint64)
    vp = lambda x: x.ctypes.data_as(C.c_void_p)

    def lincomb():
        assert ctx.lib.zk_diag_g1_lincomb_dev(ctx.h, vp(pts1), n, vp(idx), vp(r_words), vp(off), n, vp(out)) == 0

    def upload_check():
        b = ctx.bases_upload(pts1, 1)
        assert ctx.bases_subgroup_check(b)[1] == 0
        b.free()

    def check1():
        assert ctx.bases_subgroup_check(t1)[1] == 0

    (new_kernel,) = alternate(a.reps, check1)
    new_whole, old_whole, after_lincomb = alternate(a.reps, upload_check, lincomb, check1)
    assert not out.any()                                      # r P = O everywhere: the same verdict
    emit({"what": "g1_table", "points": n, "check_ms": round(new_kernel, 3), "check_points_per_s": round(n / new_kernel * 1e3),
          "check_ms_right_after_a_lincomb_call": round(after_lincomb, 3),
          "upload_and_check_call_ms": round(new_whole, 3), "lincomb_by_r_call_ms": round(old_whole, 3),
          "lincomb_call_over_upload_and_check_call": round(old_whole / new_whole, 2)})

    def check2():
        assert ctx.bases_subgroup_check(t2)[1] == 0

    (g2_ms,) = alternate(a.reps, check2)
    nh = 64
    p1h, p2h = pts1[:nh], t2.download(0, nh)
    h1, h2 = alternate(a.reps, lambda: api.in_subgroup_host(p1h, 1), lambda: api.in_subgroup_host(p2h, 2))
    emit({"what": "g2_table", "points": n, "check_ms": round(g2_ms, 3), "check_points_per_s": round(n / g2_ms * 1e3),
          "host_ms_per_point_g2": round(h2 / nh, 4), "host_ms_per_point_g1": round(h1 / nh, 4), "host_points_timed": nh})
    t1.free(); t2.free(); scal.free()

    if a.only != "tables":
        # ---- verification: the golden D = 8 key from the oracle's bytes, the oracle's predicted proofs
        ih = lambda x: int(x, 16)
        j = json.load(open(os.path.join(ROOT, "tests", "golden", "groth16.json")))["mul_chain_5"]
        rows_of = lambda m: [[(ih(c), k) for c, k in row] for row in m]
        r1cs = O.R1CS(j["num_instance"], j["num_witness"], rows_of(j["a"]), rows_of(j["b"]), rows_of(j["c"]))
        t = j["trapdoor"]
        td = O.Trapdoor(*[ih(t[k]) for k in ("alpha", "beta", "gamma", "delta", "tau", "g1_k", "g2_k")])
        ps = O.ProvingKeyScalars(r1cs, td)
        pk, _, _ = S.proving_key_from_bytes(ctx, O.pk_serialize(O.ProvingKey(ps), False))
        z = [ih(v) for v in j["z"]]
        distinct = [O.proof_serialize(*O.predict_proof(r1cs, ps, z, rng.fr(), rng.fr())) for _ in range(8)]
        top = 1024
        proofs = [distinct[k % 8] for k in range(top)]
        inputs = np.tile(cv.fr_to_mont(z[1:j["num_instance"]]).reshape(1, -1, 4), (top, 1, 1))
        for count in (1, 64, 1024):
            assert ctx.groth16_verify_batch(pk, inputs[:count], proofs[:count], check_subgroup=True).all()
            plain, checked = alternate(a.reps, lambda: ctx.groth16_verify_batch(pk, inputs[:count], proofs[:count]),
                                       lambda: ctx.groth16_verify_batch(pk, inputs[:count], proofs[:count], check_subgroup=True))
            emit({"what": "verify", "circuit": "mul_chain_5 (D = 8)", "count": count, "unchecked_ms_per_call": round(plain, 3),
                  "checked_ms_per_call": round(checked, 3), "checked_over_unchecked": round(checked / plain, 3)})
        pk.free()

        # ---- the key check, beside the load of the same key
        if a.key_log:
            nk = (1 << a.key_log) - 2
            dr = ctx.r1cs_mul_chain(nk)
            pk = ctx.groth16_setup(dr, *[mont1(rng.fr()) for _ in range(7)])

            def key_check():
                assert all(v == (0, None) for v in pk.check_subgroups().values())

            (ms,) = alternate(a.reps, key_check)
            g1 = sum(pk.query_len(q) for q in ("a_query", "b_g1_query", "h_query", "l_query", "gamma_abc_g1"))
            g2 = pk.query_len("b_g2_query")
            data = S.proving_key_bytes(ctx, pk, False)
            pk.free()
            t0 = time.perf_counter()
            pk2, _, _ = S.proving_key_from_bytes(ctx, data)
            load_ms = (time.perf_counter() - t0) * 1e3
            pk2.free(); dr.free()
            emit({"what": "pk_check", "circuit": "mul_chain_2p%d" % a.key_log, "g1_points": g1, "g2_points": g2,
                  "check_ms": round(ms, 1), "pk_deserialize_uncompressed_ms": round(load_ms, 1)})

    if a.out != "/dev/null":
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
