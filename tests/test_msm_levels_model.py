"""Shifted window multiples (msm_digits.cuh: level_bucket; msm.hip: msm_set_sum) as a pure-Python model, checked exhaustively.

A signed digit of magnitude d in [1, 2^(c-1)] with v trailing zero bits takes its point from level m = min(v, M) -- the table entry
2^m P -- and goes to the bucket labelled d >> m.  The labels that occur are [1, D] and the odd ones in (D, 2^(c-1)], D = 2^(c-1-M);
numbered compactly they are 2^M + 1 windows of Nw = D / 2 buckets.  The reduce leaves, per window w, T_w = sum_i S_i and
U_w = sum_i (i + 1) S_i, and the host combines them with a weight pair (a_w, s_w).  Here P = 1: a bucket sum is an integer."""
import pytest


def level_bucket(d, M, c):
    """(compact bucket index, level) of digit magnitude d"""
    if M == 0:
        return d - 1, 0
    D = 1 << (c - 1 - M)
    v = 0
    while v < M and not (d >> v) & 1:
        v += 1
    label = d >> v
    return (label - 1 if label <= D else D + (label - D - 1) // 2), v


def window_weights(M, c):
    """[(a_w, s_w)]: bucket i of window w carries the label a_w + s_w (i + 1)"""
    if M == 0:
        return [(0, 1)]
    Nw = 1 << (c - 2 - M)
    D = 2 * Nw
    return [(0, 1), (Nw, 1)] + [(D + 2 * (w - 2) * Nw - 1, 2) for w in range(2, (1 << M) + 1)]


def combine_as_the_host_does(T, U, M, c):
    """msm_set_sum's arrangement of sum_w (a_w T_w + s_w U_w): doublings and a running sum only"""
    if M == 0:
        return U[0]
    R, log_nb = (1 << M) + 1, c - 2 - M
    u = U[0] + U[1] + 2 * sum(U[2:])
    run = tot = 0
    for w in range(R - 1, 1, -1):
        run += T[w]
        tot += run
    return u + ((T[1] + 2 * tot) << log_nb) - run


@pytest.mark.parametrize("c", [6, 8])
@pytest.mark.parametrize("M", [0, 1, 2, 3])
def test_labels_indices_and_weights_exhaustively(c, M):
    half = 1 << (c - 1)
    Nw = 1 << (c - 2 - M) if M else half
    R = (1 << M) + 1 if M else 1
    NB = R * Nw
    assert NB == ((1 << (c - 2)) + (1 << (c - 2 - M)) if M else half)
    weights = window_weights(M, c)
    assert len(weights) == R
    # every digit alone: its bucket's label times its level's multiple is the digit, and the index is inside the compact range
    seen = {}
    for d in range(1, half + 1):
        idx, lvl = level_bucket(d, M, c)
        assert 0 <= idx < NB and 0 <= lvl <= M
        w, i = divmod(idx, Nw)
        a, s = weights[w]
        assert (a + s * (i + 1)) << lvl == d, (d, idx, lvl)
        seen.setdefault(idx, set()).add(d >> lvl)
    assert sorted(seen) == list(range(NB))                    # every compact bucket is used ...
    assert all(len(v) == 1 for v in seen.values())            # ... by one label
    # all digits at once, each with a different multiplicity (and sign): sum_w (a_w T_w + s_w U_w) == sum_d mult_d * d
    S = [0] * NB
    want = 0
    for d in range(1, half + 1):
        mult = (d * 2654435761 % 1009) - 504                  # the number of points with this digit, signs folded in
        idx, lvl = level_bucket(d, M, c)
        S[idx] += mult << lvl                                 # the bucket receives mult entries of level lvl: mult * 2^lvl * P
        want += mult * d
    T = [sum(S[w * Nw:(w + 1) * Nw]) for w in range(R)]
    U = [sum((i + 1) * S[w * Nw + i] for i in range(Nw)) for w in range(R)]
    assert sum(a * T[w] + s * U[w] for w, (a, s) in enumerate(weights)) == want
    assert combine_as_the_host_does(T, U, M, c) == want


@pytest.mark.parametrize("c,M,expect", [(20, 3, 3), (20, 1, 1), (13, 3, 3), (10, 3, 2), (10, 2, 2), (9, 3, 1), (8, 3, 0), (8, 1, 0), (20, 7, 3)])
def test_clamp(c, M, expect):
    """zk_msm_mul_levels_clamp (host code of the library): at most three levels, and a reduce window keeps 2^6 buckets: c - 2 - M >= 6"""
    import zk_mpc_amd
    assert zk_mpc_amd.load().zk_msm_mul_levels_clamp(c, M) == expect
