"""GPU: the MSM kernels where additions degenerate -- doubling, cancellation, infinity -- on every kernel path, exactly.

Every table is small multiples of one point (msm_degenerate_cases.py), so every stage of an MSM -- the accumulate chains, the folds of
split buckets, the row / column / bit sums of the grid reduce, the host's Horner chain -- adds points that are equal, opposite or
at infinity all the time, and the result is one scalar multiplication in the oracle.  One case per kernel path; each case asserts,
from the record the dispatch code leaves (Context.msm_plans), that the job went where the case is for.  The shapes are the smallest
that reach their path with the dispatch constants of csrc/msm.hip, csrc/msm_batch.hip, csrc/msm_g2pair.hip and
csrc/fixed_base.hip; if those move, the record says so and the shape has to move with them.
"""
import time

import numpy as np
import pytest

import zk_mpc_amd.convert as cv
import msm_degenerate_cases as D

pytestmark = pytest.mark.gpu


def _affine(group, out):
    return (cv.g1_projective_to_affine if group == 1 else cv.g2_projective_to_affine)(out)


def _check_record(case, rec, plan):
    want = case["want"]
    got = {k: rec[k] for k in want}
    assert got == want, "%s: the job took another path: %r, wanted %r (whole record: %r)" % (case["id"], got, want, rec)
    # the windows the CPU model counted events for (test_msm_degenerate_model.py) are the job's own
    assert (rec["c"], rec["W"], rec["off"], rec["NB"]) == (plan["c"], plan["W"], plan["off"], plan["NB"]), (rec, plan)


@pytest.mark.parametrize("case", [pytest.param(c, id=c["id"]) for c in D.CASES])
def test_msm_over_small_multiples(ctx, case):
    """Every scalar set at full length, and the uniform one at (off, m) = (3, n - 3), equal the closed form; the record of every
    full-length job names the path of the case.  The certain set is built from the record of the first job."""
    group, n, jobs, vectors = case["group"], case["n"], case["jobs"], case["vectors"]
    t0 = time.time()
    ms, arr, P = D.table(group, n, 31 * n + group)
    bases = ctx.bases_upload(arr, group)
    try:
        if case["layout"]:
            bases.precompute(case["layout"])
        ctx.msm_plans()                                              # forget what earlier tests left
        model = D.case_plan(case)
        seed = 1000 + n
        first = D.uniform_scalars(n, seed + 1)
        bufs = {}

        def keep(name, a):                                           # (a device buffer lives as long as its entry here)
            bufs[name] = ctx.upload(a)
            return bufs[name]

        def dev(name, sc):
            return keep(name, D.to_mont(sc))

        def one(sc, off=0, m=n):
            return _affine(group, ctx.msm_dev(bases, off, dev("one", sc).ptr, m))

        if vectors > 1:
            # one job of `vectors` scalar vectors, n + 2 elements apart: the record of a first call gives the windows
            stride = n + 2
            probe = np.zeros((vectors * stride, 4), dtype=np.uint64)
            probe[:n] = D.to_mont(first)
            ctx.msm_multi_dev(bases, 0, keep("probe", probe).ptr, n, stride, vectors)
            (rec,) = ctx.msm_plans()
            sets = list(D.scalar_sets(rec, ms, seed).items()) + [("uniform2", D.uniform_scalars(n, seed + 9))]
            assert len(sets) == vectors
            flat = np.zeros((vectors * stride, 4), dtype=np.uint64)
            for k, (_, sc) in enumerate(sets):
                flat[k * stride:k * stride + n] = D.to_mont(sc)
            dflat = keep("flat", flat)
            outs = ctx.msm_multi_dev(bases, 0, dflat.ptr, n, stride, vectors)
            (rec,) = ctx.msm_plans()
            _check_record(case, rec, model)
            for k, (name, sc) in enumerate(sets):
                assert _affine(group, outs[k]) == D.expected(group, P, ms, sc), (case["id"], name)
            # ... and over the table from entry 3 on
            outs = ctx.msm_multi_dev(bases, 3, dflat.ptr, n - 3, stride, vectors)
            for k, (name, sc) in enumerate(sets):
                assert _affine(group, outs[k]) == D.expected(group, P, ms, sc, 3, n - 3), (case["id"], name, "offset")
        elif jobs > 1:
            # a group of `jobs` jobs over one table through the batch call, one scalar vector each
            probe = ctx.msm_batch_dev([(bases, 0, dev("p%d" % k, first).ptr, n) for k in range(jobs)])
            recs = ctx.msm_plans()
            assert len(recs) == jobs
            assert all(_affine(group, o) == D.expected(group, P, ms, first) for o in probe)
            runs = [(name, sc, 0, n) for name, sc in D.scalar_sets(recs[0], ms, seed).items()] + [("uniform-offset", first, 3, n - 3)]
            while len(runs) % jobs:
                runs.append(runs[3])                                 # (the certain set again: a full group every time)
            for g0 in range(0, len(runs), jobs):
                grp = runs[g0:g0 + jobs]
                outs = ctx.msm_batch_dev([(bases, off, dev("g%d" % k, sc).ptr, m) for k, (_, sc, off, m) in enumerate(grp)])
                recs = ctx.msm_plans()
                assert len(recs) == jobs
                for rec in recs:
                    _check_record(case, rec, model)
                for (name, sc, off, m), o in zip(grp, outs):
                    assert _affine(group, o) == D.expected(group, P, ms, sc, off, m), (case["id"], name)
        else:
            assert one(first) == D.expected(group, P, ms, first), (case["id"], "uniform")
            (rec,) = ctx.msm_plans()
            _check_record(case, rec, model)
            for name, sc in D.scalar_sets(rec, ms, seed).items():
                if name != "uniform":
                    assert one(sc) == D.expected(group, P, ms, sc), (case["id"], name)
            for rec in ctx.msm_plans():
                _check_record(case, rec, model)
            assert one(first, 3, n - 3) == D.expected(group, P, ms, first, 3, n - 3), (case["id"], "uniform-offset")
    finally:
        ctx.sync()
        bases.free()
    print("%s: %.2f s" % (case["id"], time.time() - t0))


def test_msm_plans_ring_keeps_the_latest(ctx):
    """The record ring drops the oldest: after more jobs than it holds, one call returns the last ZK_MSM_PLAN_RING of them, oldest
    first, and the next call returns none."""
    from zk_mpc_amd import _lib
    ms, arr, _ = D.table(1, 64, 5)
    bases = ctx.bases_upload(arr, 1)
    try:
        sc = ctx.upload(D.to_mont(D.uniform_scalars(64, 6)))
        ctx.msm_plans()
        lens = [8 + (k % 50) for k in range(_lib.MSM_PLAN_RING + 7)]
        for m in lens:
            ctx.msm_dev(bases, 0, sc.ptr, m)
        recs = ctx.msm_plans()
        assert [r["n"] for r in recs] == lens[-_lib.MSM_PLAN_RING:]
        assert all(r["group"] == 1 and r["table"] == "plain" and r["vectors"] == 1 and len(r["off"]) == r["W"] + 1 for r in recs)
        assert ctx.msm_plans() == []
    finally:
        bases.free()
