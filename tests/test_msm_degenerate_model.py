"""CPU: the inputs of test_gpu_msm_degenerate.py do what they are for.

The closed form (sum s_i m_i mod r) * P equals the oracle's naive MSM on every scalar set, and an integer model of the accumulate
kernel's chains (msm_degenerate_cases.count_events) counts how often an addition meets a doubling or a cancellation: at least 100
of each on an accumulator that is not fresh, for every shape of the GPU test and every order the sort may leave a bucket in.  That
is a condition on the inputs: a shape that falls short gets other inputs, not another bound."""
import numpy as np
import pytest

import zkref as O
import msm_degenerate_cases as D

ORDERS = ("ascending", "descending", "shuffled")


@pytest.mark.parametrize("group,n,merged", [(1, 96, False), (1, 96, True), (1, 33, False), (2, 40, False), (2, 40, True)])
def test_closed_form_equals_naive_msm(group, n, merged):
    """Every scalar set over a table of small multiples, whole and at (off, m) = (3, n - 3), against O.msm_naive."""
    ms, arr, P = D.table(group, n, 1000 + n)
    assert arr.shape == (n, 12 * group) and (ms == 0).any() and set(np.unique(ms)) <= set(range(-D.J, D.J + 1))
    assert not arr[ms == 0].any() and arr[ms != 0].any(axis=1).all()
    pts = D.table_points(group, ms, P)
    ops = O.FqOps if group == 1 else O.Fq2Ops
    plan = D.model_plan(n, merged)
    for name, sc in D.scalar_sets(plan, ms, 7 * n).items():
        assert all(0 <= s < O.R_MOD for s in sc) and len(sc) == n
        assert D.expected(group, P, ms, sc) == O.msm_naive(pts, sc, ops), name
        assert D.expected(group, P, ms, sc, 3, n - 3) == O.msm_naive(pts[3:], sc[:n - 3], ops), name
    assert D.expected(group, P, ms, [0] * n) is None


def test_to_mont_is_fr_to_mont():
    import zk_mpc_amd.convert as cv
    sc = D.uniform_scalars(50, 3) + [0, 1, O.R_MOD - 1]
    assert (D.to_mont(sc) == cv.fr_to_mont(sc)).all()


def test_plan_digits_recompose_the_scalar():
    """sum_w digit_w 2^off[w] == s for the model's windows, plain and merged, and every digit is in its signed range."""
    for n, merged in ((300, False), (24576, False), (512, True), (65536, True)):
        plan = D.model_plan(n, merged)
        sc = D.uniform_scalars(64, n) + [0, 1, O.R_MOD - 1]
        dg = D.plan_digits(plan, sc)
        off = plan["off"]
        assert off[-1] >= 255 and len(off) == plan["W"] + 1
        for s, row in zip(sc, dg):
            assert sum(int(d) << off[w] for w, d in enumerate(row)) == s
            assert all(-(1 << (off[w + 1] - off[w] - 1)) <= d < 1 << (off[w + 1] - off[w] - 1) for w, d in enumerate(row))


def _model_shapes():
    seen, out = set(), []
    for c in D.CASES:
        key = (c["n"], c["layout"] != 0, c["vectors"])
        if key not in seen:
            seen.add(key)
            out.append(pytest.param(c, id="n%d-%s-v%d" % (c["n"], "merged" if key[1] else "plain", c["vectors"])))
    return out


@pytest.mark.parametrize("case", _model_shapes())
def test_special_branches_are_hit(case):
    """Per shape (the plan of one vector; the segment length of the whole job) and per order: doublings and cancellations on an
    accumulator that is not fresh, summed over the scalar sets the GPU test runs on that shape, >= 100 each; and the certain set
    delivers what it is laid out for in EVERY order -- a cancellation per neg_pair and neg_triple bucket (the latter not fresh), a
    doubling per dbl_pair bucket and for a third of the dbl_triple buckets (not fresh)."""
    n = case["n"]
    plan = D.case_plan(case)
    ms = D.multiples(n, 11)
    sets = D.scalar_sets(plan, ms, 5)
    buckets, _ = D.certain_layout(plan, ms, 5 + 4)
    per_kind = {k: sum(1 for b in buckets if b[0] == k) for k in D.KINDS}
    k = D.certain_count(n)
    assert k >= 12 and all(v == k for v in per_kind.values()), per_kind
    assert len({b[1] for b in buckets}) == len(buckets)                       # a bucket of its own each
    for kind, (w, d), idx in buckets:                                         # ... whose entries are the multiples it is named for
        vals = sorted(int(ms[i]) for i in idx)
        if kind == "dbl_pair":
            assert len(vals) == 2 and vals[0] == vals[1] != 0
        elif kind == "neg_pair":
            assert len(vals) == 2 and vals[0] == -vals[1] != 0
        else:
            assert len(vals) == 3 and 0 not in vals and len({abs(v) for v in vals}) == 3
            by_pos = [int(ms[i]) for i in sorted(idx)]
            assert (sum(by_pos) == 0) if kind == "neg_triple" else (max(by_pos, key=abs) == sum(by_pos) - max(by_pos, key=abs))
    # the six index orders of the dbl_triple buckets in equal shares: where the largest multiple sits among the three, by table index
    last = [sorted(idx).index(max(idx, key=lambda i: abs(int(ms[i])))) for kind, _, idx in buckets if kind == "dbl_triple"]
    assert [last.count(p) for p in range(3)] == [k // 3] * 3
    for order in ORDERS:
        tot = dict(dbl_deep=0, neg_deep=0)
        for name, sc in sets.items():
            ev = D.count_events(plan, ms, sc, order, seed=17)
            for key in tot:
                tot[key] += ev[key]
            if name == "certain":
                # the dbl_triple buckets: a + b comes last in exactly a third of them when the bucket keeps the table order either
                # way round; a shuffle puts it last with probability 1 / 3 per bucket (binomial: four standard deviations below k / 3)
                third = k // 3 if order != "shuffled" else max(0, int(k / 3 - 4 * (2 * k / 9) ** 0.5))
                assert ev["neg"] >= 2 * k and ev["neg_deep"] >= k, (order, ev)
                assert ev["dbl"] >= k + third and ev["dbl_deep"] >= third, (order, ev)
            assert ev["inf_entry"] > 0 and ev["restart"] > 0, (order, name, ev)
        assert tot["dbl_deep"] >= 100 and tot["neg_deep"] >= 100, (order, tot)
