"""Boundary cases of the lazy-domain field arithmetic (fp29.cuh, frlazy.cuh, msm_g2pair.hip, she.hip), shared by the host-build tests
(test_abi.py) and the device tests (test_gpu_lazy_domain.py): raw 29-bit limb layouts, the range ends each file states, the values
just below them and operands whose low limbs are all at 2^29 - 1."""
import json
import os
import random

import zkref as O

M29 = (1 << 29) - 1

# ---- Fq (BLS12-377 base field): 13 limbs, Montgomery radix RI = 2^406 inside the kernels ----------------------------------------
Q = O.Q_MOD
RI14 = 1 << (29 * 14)
EPS = 1 << 354


def _limbs_wide(v):
    """13 limbs: 12 of 29 bits and a top limb holding the rest (< 2^32)."""
    assert 0 <= v < (1 << (29 * 12 + 32))
    return [(v >> (29 * i)) & M29 for i in range(12)] + [v >> (29 * 12)]


def _val(a):
    return sum(int(x) << (29 * i) for i, x in enumerate(a))


def _normalised(a, top_bits=29):
    return all(int(x) < (1 << 29) for x in a[:12]) and int(a[12]) < (1 << top_bits)


def below(end, n_low):
    """The largest value below `end`, and the largest one below it whose n_low low limbs are all 2^29 - 1 (when there is one)."""
    out = [end - 1]
    mask = (1 << (29 * n_low)) - 1
    v = ((end - 1) & ~mask) | mask
    if v >= end:
        v -= 1 << (29 * n_low)
    if v >= 0:
        out.append(v)
    return out


# the range ends fp29.cuh / ec.cuh / msm_g2pair.hip state for Fq lazy values
FQ_RANGE_ENDS = [Q, Q + EPS, 2 * Q, 3 * Q + EPS, 5 * Q + EPS, 7 * Q + EPS, 7 * Q + 2 * EPS]
FQ_ENDS = [0, 1, Q - 1, Q, Q + EPS - 1, 2 * Q, 3 * Q + EPS, 5 * Q + EPS - 1, 7 * Q + EPS - 1, 7 * Q + 2 * EPS - 1]


def fq_below_ends(limit=None):
    """Every value just below an Fq range end (the end itself excluded), below `limit` if given."""
    vals = sorted({v for e in FQ_RANGE_ENDS for v in below(e, 12)})
    return [v for v in vals if limit is None or v < limit]


def fq_ends(limit):
    """FQ_ENDS and the below-end values, restricted to [0, limit)."""
    return sorted({v for v in FQ_ENDS + fq_below_ends() if v < limit})


def neg5_cases(rnd, n_random=3000):
    """Operands of fp_neg5_almost at its quotient boundaries j q / 5, at the top-limb boundaries and at random (all < q)."""
    q = Q
    ptop = q >> 348
    cases = [0, 1, 2, q - 1, q - 2, ptop << 348, (ptop << 348) - 1, (ptop - 1) << 348, (1 << 348) - 1, 1 << 348]
    for j in range(1, 6):
        t = ((j * q) // 5) >> 348
        cases += [v for v in [(j * q) // 5 + d for d in range(-3, 4)] if 0 <= v < q]
        cases += [v for v in [((t + dt) << 348) + low for dt in (-1, 0, 1) for low in (0, (1 << 348) - 1)] if 0 <= v < q]
    return cases + [rnd.randrange(q) for _ in range(n_random)]


# operands whose low limbs are zero: the first product columns are clear and the first Montgomery digit is 2^29
FQ_SPARSE = [1 << (29 * k) for k in (1, 2, 5, 12)] + [3 << 87, (Q >> 58) << 58, ((7 * Q) >> 29) << 29, 1 << 376]


def worst_columns(tops, split_top=False):
    """Worst-case column sums (in the order the kernels accumulate them) of the product scanning with every low limb at
    2^29 - 1, the given top limbs per operand ((a, b) or (a, b, c, d)) and every Montgomery digit at its maximum (2^29 for the
    first one, fp29.cuh::fp_redc_column).  The m_i p_0 terms stand for the "+ 1" carries the kernels never add: an upper bound."""
    L, LR = 13, 14
    pl = [(Q >> (29 * i)) & M29 for i in range(13)]
    mmax = M29
    ops = [[M29] * 12 + [t] for t in tops]
    carry, cols = 0, []
    for k in range(LR + L - 1):
        col, up = carry, 0
        for i in range(L):
            j = k - i
            if 0 <= j < L:
                col += ops[0][i] * ops[1][j]
                if len(ops) == 4:
                    t = ops[2][i] * ops[3][j]
                    if split_top and k == 2 * L - 2:
                        col += t & M29
                        up = t >> 29
                    else:
                        col += t
        for i in range(LR):
            if 0 <= k - i < L:
                col += (mmax + 1 if i == 0 else mmax) * pl[k - i]
        cols.append(col)
        carry = (col >> 29) + up
    return cols


# ---- Fr (BLS12-377 scalar field): 9 limbs of any u32 width, RI = 2^261 -------------------------------------------------------------
RR = O.R_MOD
RI9 = 1 << 261

# range ends of frlazy.cuh: stage inputs < 2.1 r, sub<2|3|5> subtrahends < 1.03 r / 2.1 r / 4.2 r, reduce inputs < 8.4 r, last-stage
# outputs < 9.2 r, product operands < 2^261
FR_RANGE_ENDS = [RR, 103 * RR // 100, 21 * RR // 10, 42 * RR // 10, 84 * RR // 10, 92 * RR // 10, RI9]
FR_ENDS = [0, 1, RR - 1, RR, 2 * RR, 21 * RR // 10, 42 * RR // 10, 84 * RR // 10, 92 * RR // 10 - 1, 16 * RR, 438 * RR, RI9 - 1]


def _l9(v):
    assert 0 <= v < RI9
    return [(v >> (29 * i)) & M29 for i in range(9)]


def _spread(v, rnd, limb_cap):
    """The same value with limbs pushed above 29 bits where the value allows: limb i borrows from limb i + 1."""
    l = _l9(v)
    for i in range(8):
        k = min(l[i + 1], (limb_cap - l[i]) >> 29)
        k = rnd.randrange(k + 1) if k > 0 else 0
        l[i] += k << 29
        l[i + 1] -= k
    assert sum(x << (29 * i) for i, x in enumerate(l)) == v and all(0 <= x < (1 << 32) for x in l)
    return l


def spread_max(v, limb_cap):
    """v with every limb pushed as high as limb_cap allows (the worst limb spread), from the top limb down."""
    l = _l9(v)
    for i in range(7, -1, -1):
        k = min(l[i + 1], (limb_cap - l[i]) >> 29)
        if k > 0:
            l[i] += k << 29
            l[i + 1] -= k
    for i in range(8):                       # a second pass lets a limb that received from above pass it further down
        k = min(l[i + 1], (limb_cap - l[i]) >> 29)
        if k > 0:
            l[i] += k << 29
            l[i + 1] -= k
    assert sum(x << (29 * i) for i, x in enumerate(l)) == v and all(0 <= x <= limb_cap for x in l)
    return l


def fr_below_ends():
    return sorted({v for e in FR_RANGE_ENDS for v in below(e, 8)})


# ---- the SHE field (MNT4-753 base field): 26 limbs of 29 bits, RI = 2^754 -----------------------------------------------------------
def q753():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return int(json.load(open(os.path.join(root, "tests", "golden", "ref_constants.json")))["mnt4_753_fq"]["MODULUS"]["value"])


RI26 = 1 << 754


def l26(v):
    assert 0 <= v < (1 << (29 * 25 + 32))
    return [(v >> (29 * i)) & M29 for i in range(25)] + [v >> (29 * 25)]


def she_range_ends(q):
    """she.hip's ends: red's output 2.01 q, f7l_sub<3>'s subtrahend 2.26 q, a product 1.89 q, red's input 7.9 q."""
    return [q, 189 * q // 100, 2 * q, 201 * q // 100, 226 * q // 100, 79 * q // 10]


def she_below_ends(q):
    return sorted({v for e in she_range_ends(q) for v in below(e, 25)})


def rng(seed):
    return random.Random(seed)
