"""GPU: the lazy-domain field arithmetic as the DEVICE code object runs it, at the ends of the ranges its comments state.

fp29.cuh / frlazy.cuh / ec.cuh (Fq, Fr: against the host build word for word, and against big integers), msm_g2pair.hip (the G2
lane-pair Fq2 products and additions), ec_dual.cuh on lane pairs and quads, and she.hip (the lazy field of the MNT4-753 transforms):
congruent to the exact result, inside the stated range, limbs normalised -- through the diag.hip test hooks, each op in one launch."""
import ctypes as C

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd as Z
from lazy_cases import (EPS, FQ_SPARSE, FR_ENDS, M29, Q, RI14, RI26, RI9, RR, _l9, _limbs_wide, _normalised, _spread, _val, below,
                        fq_ends, fr_below_ends, l26, neg5_cases, q753, rng, she_below_ends, spread_max)

pytestmark = pytest.mark.gpu

N = 12000          # random cases per primitive op
NP = 3000          # random cases per point op
INV14 = pow(RI14, -1, Q)
INV9 = pow(RI9, -1, RR)
WIDE = 7 * Q + 2 * EPS


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev(ctx, fn, op, rows, n_out, words):
    inp = np.ascontiguousarray(np.array(rows, dtype=np.uint32))
    out = np.zeros((len(rows), n_out * words), dtype=np.uint32)
    ctx._ck(getattr(ctx.lib, fn)(ctx.h, op, _p(inp), _p(out), len(rows)))
    return inp, out.reshape(len(rows), n_out, words)


def _host(fn, op, inp, n_out, words):
    f = getattr(Z.load(), fn)
    out = np.zeros((len(inp), n_out * words), dtype=np.uint32)
    for i in range(len(inp)):
        assert f(op, _p(inp[i]), _p(out[i])) == 0
    return out.reshape(len(inp), n_out, words)


# ---- field models on the kernels' Montgomery residues (x RI14) and the XYZZ formulas ---------------------------------------------
class Fm:
    """Fq on residues."""
    z = 0
    one = RI14 % Q
    zero = staticmethod(lambda a: a % Q == 0)
    add = staticmethod(lambda a, b: (a + b) % Q)
    sub = staticmethod(lambda a, b: (a - b) % Q)
    mul = staticmethod(lambda a, b: a * b * INV14 % Q)
    red = staticmethod(lambda a: a % Q)


class F2m:
    """Fq2 (u^2 = -5: oracle/zkref.py::fq2_mul) on residues, components as pairs."""
    z = (0, 0)
    one = (RI14 % Q, 0)
    zero = staticmethod(lambda a: a[0] % Q == 0 and a[1] % Q == 0)
    add = staticmethod(lambda a, b: ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q))
    sub = staticmethod(lambda a, b: ((a[0] - b[0]) % Q, (a[1] - b[1]) % Q))
    red = staticmethod(lambda a: (a[0] % Q, a[1] % Q))

    @staticmethod
    def mul(a, b):
        c = O.fq2_mul((a[0] % Q, a[1] % Q), (b[0] % Q, b[1] % Q))
        return (c[0] * INV14 % Q, c[1] * INV14 % Q)


def _dbl_affine_formula(F, q):
    """mdbl-2008-s-1 (ec.cuh::xyzz_dbl_affine, msm_g2pair.hip::dbl_affine_p)"""
    u = F.add(q[1], q[1])
    if F.zero(u):
        return [F.z] * 4
    v = F.mul(u, u)
    w, s = F.mul(u, v), F.mul(q[0], v)
    xx = F.mul(q[0], q[0])
    m = F.add(F.add(xx, xx), xx)
    x3 = F.sub(F.mul(m, m), F.add(s, s))
    return [x3, F.sub(F.mul(m, F.sub(s, x3)), F.mul(w, q[1])), v, w]


def _dbl_formula(F, a):
    """dbl-2008-s-1 (ec.cuh::xyzz_dbl)"""
    if F.zero(a[2]):
        return list(a)
    x3, y3, v, w = _dbl_affine_formula(F, a[:2])
    if F.zero(v):
        return [F.z] * 4
    return [x3, y3, F.mul(v, a[2]), F.mul(w, a[3])]


def _madd_formula(F, acc, q):
    """madd-2008-s with the special cases as the kernels take them (acc infinity = zz = 0; P = 0: doubling or infinity by R)"""
    x1, y1, zz1, zzz1 = acc
    if F.zero(zz1):
        return [q[0], q[1], F.one, F.one]
    p, r = F.sub(F.mul(q[0], zz1), x1), F.sub(F.mul(q[1], zzz1), y1)
    if F.zero(p):
        return _dbl_affine_formula(F, q) if F.zero(r) else [F.z] * 4
    pp = F.mul(p, p)
    ppp, qq = F.mul(pp, p), F.mul(pp, x1)
    x3 = F.sub(F.sub(F.mul(r, r), ppp), F.add(qq, qq))
    y3 = F.sub(F.mul(r, F.sub(qq, x3)), F.mul(ppp, y1))
    return [x3, y3, F.mul(zz1, pp), F.mul(zzz1, ppp)]


def _add_formula(F, a, b):
    """add-2008-s with the kernels' special cases"""
    if F.zero(a[2]):
        return list(b)
    if F.zero(b[2]):
        return list(a)
    u1, u2 = F.mul(a[0], b[2]), F.mul(b[0], a[2])
    s1, s2 = F.mul(a[1], b[3]), F.mul(b[1], a[3])
    p, r = F.sub(u2, u1), F.sub(s2, s1)
    if F.zero(p):
        return _dbl_formula(F, [F.red(c) for c in a]) if F.zero(r) else [F.z] * 4
    pp = F.mul(p, p)
    ppp, qq = F.mul(pp, p), F.mul(pp, u1)
    x3 = F.sub(F.sub(F.mul(r, r), ppp), F.add(qq, qq))
    y3 = F.sub(F.mul(r, F.sub(qq, x3)), F.mul(ppp, s1))
    return [x3, y3, F.mul(F.mul(a[2], b[2]), pp), F.mul(F.mul(a[3], b[3]), ppp)]


def _check_point_out(F, vals, want, ranges, what):
    """lazy coordinates (vals[:4]) congruent to the formula and inside `ranges`; canonical ones (vals[4:]) equal to it"""
    assert [F.red(x) for x in vals[:4]] == [F.red(x) for x in want], what
    assert list(vals[4:]) == [F.red(x) for x in want], what
    for x, hi in zip(vals[:4], ranges):
        assert all(c < hi for c in (x if isinstance(x, tuple) else (x,))), (what, hex(hi))


def _acc_ends(ranges):
    """the top four values of fq_ends below each coordinate's range end; zz, zzz without the multiples of q (a non-zero zz is never
    congruent to 0: infinity is all-zero words)"""
    return [[v for v in fq_ends(h) if k < 2 or v % Q][-4:] for k, h in enumerate(ranges)]


# ---- Fq (fp29.cuh, ec.cuh) ----------------------------------------------------------------------------------------------------------
FQ_NOUT = {10: 8, 12: 8}
G1_RANGES = (5 * Q + EPS, Q + EPS, Q + EPS, Q + EPS)     # ec.cuh::xyzz_madd_lazy / xyzz_add_lazy: x, y, zz, zzz


def _fq_run(ctx, op, cases):
    rows = [[l for v in c for l in _limbs_wide(v)] for c in cases]
    n_out = FQ_NOUT.get(op, 1)
    inp, dev = _dev(ctx, "zk_diag_fq_lazy_dev", op, rows, n_out, 13)
    host = _host("zk_fq_lazy_raw", op, inp, n_out, 13)
    bad = np.nonzero((dev != host).any(axis=(1, 2)))[0]
    assert len(bad) == 0, "op %d: device != host build on %d cases, first %r" % (op, len(bad), [hex(v) for v in cases[bad[0]]])
    return [[_val(e) for e in o] for o in dev], dev


def test_fq_lazy_primitives_device_matches_host_and_big_integers(ctx):
    """ops 0 - 9 and 11 of zk_fq_lazy_raw on the device: word for word the host build's output, and congruent / exact / in range
    by big integers, for every range end, the values just below it (also with all twelve low limbs at 2^29 - 1) and random."""
    rnd = rng(1)
    wide = fq_ends(WIDE)
    # 0 mul_l, 1 sqr_l: operands up to 7q + 2 eps -> < q + eps
    cases = [(a, b) for a in wide for b in wide] + [(a, b) for a in FQ_SPARSE + [0] for b in FQ_SPARSE + [0, 1, Q]]
    cases += [(rnd.randrange(WIDE), rnd.randrange(WIDE)) for _ in range(N)]
    res, dev = _fq_run(ctx, 0, cases)
    for (a, b), (r,), w in zip(cases, res, dev):
        assert r % Q == a * b * INV14 % Q and r < Q + EPS and _normalised(w[0]), (hex(a), hex(b))
    cases = [(a,) for a in wide + FQ_SPARSE] + [(rnd.randrange(WIDE),) for _ in range(N)]
    res, dev = _fq_run(ctx, 1, cases)
    for (a,), (r,), w in zip(cases, res, dev):
        assert r % Q == a * a * INV14 % Q and r < Q + EPS and _normalised(w[0]), hex(a)
    # 2 mul2 (the operand mixes of test_abi.py's column model), 11 mul2 with the split top column (four operands up to 7q + 2 eps)
    for op, shapes in ((2, [(7, 7, 1, 7), (3, 7, 2, 2), (5, 7, 5, 7), (5, 5, 5, 5)]), (11, [(7, 7, 7, 7)])):
        cases = []
        for sh in shapes:
            lim = [k * Q + 2 * EPS for k in sh]
            ends = [fq_ends(h)[-6:] for h in lim]
            cases += [tuple(e[(i + j) % len(e)] for j, e in enumerate(ends)) for i in range(36)] + [tuple(h - 1 for h in lim)]
            cases += [tuple(rnd.randrange(h) for h in lim) for _ in range(N // len(shapes))]
        res, dev = _fq_run(ctx, op, cases)
        for (a, b, c, d), (r,), w in zip(cases, res, dev):
            t = a * b + c * d
            assert r % Q == t * INV14 % Q and r * RI14 <= t + Q * RI14 and r < Q + 2 * EPS and _normalised(w[0]), (op, hex(a))
    # 3..5 sub_kp<2|4|6>(a, b) = a + K q - b exactly: a a product (< q + 2 eps), b <= K q
    for op, K in ((3, 2), (4, 4), (5, 6)):
        bvals = sorted({0, 1, Q, K * Q} | set(below(K * Q, 12)) | set(fq_ends(K * Q)))
        cases = [(a, b) for a in fq_ends(Q + 2 * EPS) for b in bvals]
        cases += [(rnd.randrange(Q + 2 * EPS), rnd.randrange(K * Q + 1)) for _ in range(N)]
        res, dev = _fq_run(ctx, op, cases)
        for (a, b), (r,), w in zip(cases, res, dev):
            assert r == a + K * Q - b and _normalised(w[0], 32), (op, hex(a), hex(b))
    # 6 x3_l(rr, ppp, qq) = rr + 4q - ppp - 2qq exactly, < 5q + eps: three products below q + eps
    ends = fq_ends(Q + EPS)
    cases = [(a, b, c) for a in ends for b in ends for c in ends] + [tuple(rnd.randrange(Q + EPS) for _ in range(3)) for _ in range(N)]
    res, dev = _fq_run(ctx, 6, cases)
    for (rr, ppp, qq), (r,), w in zip(cases, res, dev):
        assert r == rr + 4 * Q - ppp - 2 * qq and r < 5 * Q + EPS and _normalised(w[0], 32)
    # 7 canon (a < 8q), 8 kp_minus<1> (y <= q), 9 neg5_almost (any a < 8q: 0 < V <= q (1 + 2e-7))
    eight = sorted(set(fq_ends(8 * Q) + below(8 * Q, 12)))
    cases = [(a,) for a in eight] + [(rnd.randrange(8 * Q),) for _ in range(N)]
    res, dev = _fq_run(ctx, 7, cases)
    assert all(r == a % Q and _normalised(w[0]) for (a,), (r,), w in zip(cases, res, dev))
    cases = [(y,) for y in [0, 1, Q - 1, Q] + below(Q, 12)] + [(rnd.randrange(Q + 1),) for _ in range(N)]
    res, dev = _fq_run(ctx, 8, cases)
    assert all(r == Q - y and _normalised(w[0]) for (y,), (r,), w in zip(cases, res, dev))
    cases = [(a,) for a in eight + neg5_cases(rnd, N)] + [(rnd.randrange(8 * Q),) for _ in range(N)]
    res, dev = _fq_run(ctx, 9, cases)
    for (a,), (v,), w in zip(cases, res, dev):
        assert (v + 5 * a) % Q == 0 and 0 < v <= Q + (Q >> 22) and _normalised(w[0]), hex(a)


def test_fq_lazy_point_additions_device_matches_host_and_formula(ctx):
    """10: ec.cuh::xyzz_madd_lazy, 12: xyzz_add_lazy, operands anywhere in their ranges (x < 5q + eps, y, zz, zzz < q + eps; the
    affine q: x reduced, y <= q) and at infinity: device == host build, canonical output == the formula, lazy outputs in range."""
    rnd = rng(2)
    ends = _acc_ends(G1_RANGES)
    cases = [tuple(e[(i + k) % len(e)] for k, e in enumerate(ends)) + (Q - 1 - i, Q - i % 3) for i in range(16)]
    cases += [tuple(rnd.randrange(h) for h in G1_RANGES) + (rnd.randrange(Q), rnd.randrange(Q + 1)) for _ in range(NP)]
    cases += [(0, 0, 0, 0, rnd.randrange(Q), rnd.randrange(Q + 1)) for _ in range(4)]
    res, _ = _fq_run(ctx, 10, cases)
    for c, r in zip(cases, res):
        _check_point_out(Fm, r, _madd_formula(Fm, list(c[:4]), [c[4], c[5] % Q]), G1_RANGES, ("madd", c))
    cases = [tuple(e[(i + k) % len(e)] for k, e in enumerate(ends)) * 2 for i in range(8)]
    cases += [tuple(rnd.randrange(h) for h in G1_RANGES) * 1 + tuple(rnd.randrange(h) for h in G1_RANGES) for _ in range(NP)]
    cases += [(0, 0, 0, 0) + c[4:] for c in cases[:4]] + [c[:4] + (0, 0, 0, 0) for c in cases[:4]]
    res, _ = _fq_run(ctx, 12, cases)
    for c, r in zip(cases, res):
        _check_point_out(Fm, r, _add_formula(Fm, list(c[:4]), list(c[4:])), G1_RANGES, ("add", c))


# ---- Fr (frlazy.cuh) --------------------------------------------------------------------------------------------------------------------
FR_NOUT = {7: 4, 8: 4, 9: 2}


def _fr_run(ctx, op, cases):
    rows = [[l for e in c for l in e] for c in cases]
    n_out = FR_NOUT.get(op, 1)
    inp, dev = _dev(ctx, "zk_diag_fr_lazy_dev", op, rows, n_out, 9)
    host = _host("zk_fr_lazy_raw", op, inp, n_out, 9)
    bad = np.nonzero((dev != host).any(axis=(1, 2)))[0]
    assert len(bad) == 0, "op %d: device != host build on %d cases, first %r" % (op, len(bad), cases[bad[0]])
    return [[_val(e) for e in o] for o in dev], dev


def test_fr_lazy_primitives_device_matches_host_and_big_integers(ctx):
    """ops 0 - 6 and 10 of zk_fr_lazy_raw on the device: the host build's output word for word; exact where the op is exact,
    congruent and in range where it reduces; operands at frlazy.cuh's range ends, with limbs spread as wide as allowed."""
    rnd = rng(3)
    vals = sorted(set(FR_ENDS + fr_below_ends()))
    # 0 reduce (< 1.13 r), 6 canon: any limbs up to 2^32 - 2^10;  1 norm (exact): limbs up to 2^32 - 16
    for op in (0, 6, 1):
        cap = (1 << 32) - (1 << 10) if op != 1 else (1 << 32) - 16
        src = vals + [rnd.randrange(RI9) for _ in range(N // 2)] + [rnd.randrange(10 * RR) for _ in range(N // 2)]
        limbs = [_l9(v) for v in src] + [spread_max(v, cap) for v in vals] + [_spread(v, rnd, cap) for v in src[:N // 2]]
        res, dev = _fr_run(ctx, op, [(l,) for l in limbs])
        for l, (r,), w in zip(limbs, res, dev):
            v = _val(l)
            ok = {0: r % RR == v % RR and r < 113 * RR // 100, 6: r == v % RR, 1: r == v}[op]
            assert ok and (w <= M29).all(), (op, l)
    # 10 mul32: v < 2^256 -> 32 v mod r
    src = [v for v in vals if v < (1 << 256)] + [rnd.randrange(1 << 256) for _ in range(N)]
    res, dev = _fr_run(ctx, 10, [(_l9(v),) for v in src])
    assert all(r == 32 * v % RR and (w <= M29).all() for v, (r,), w in zip(src, res, dev))
    # 2..4 sub<2|3|5>(a, b) = a + K r - b exactly: operands < 1.03 r / 2.1 r / 4.2 r with limbs < 2^29, 2^29, 2^30
    for op, K, bmax, blimb in ((2, 2, 103 * RR // 100, 1 << 29), (3, 3, 21 * RR // 10, 1 << 29), (4, 5, 42 * RR // 10, 1 << 30)):
        ends = [v for v in vals if v < bmax] + below(bmax, 8)
        lim = (lambda v: spread_max(v, blimb - 1)) if blimb > (1 << 29) else _l9
        cases = [(lim(a), lim(b)) for a in ends for b in ends]
        for _ in range(N):
            a, b = rnd.randrange(bmax), rnd.randrange(bmax)
            cases.append((_spread(a, rnd, blimb - 1), _spread(b, rnd, blimb - 1)) if blimb > (1 << 29) else (_l9(a), _l9(b)))
        res, dev = _fr_run(ctx, op, cases)
        for (la, lb), (r,), w in zip(cases, res, dev):
            assert r == _val(la) + K * RR - _val(lb) and (w < 2 ** 31.34).all(), op
    # 5 mul(a, w): a < 2^261 with limbs up to 2^31.33, w a table entry (< r) -> < r (1 + a / 2^261)
    cap = int(2 ** 31.33)
    cases = [(spread_max(a, cap), _l9(t)) for a in vals for t in (0, 1, RR - 1)]
    cases += [(_spread(rnd.randrange(RI9), rnd, cap), _l9(rnd.choice([RR - 1, rnd.randrange(RR)]))) for _ in range(N)]
    res, dev = _fr_run(ctx, 5, cases)
    for (la, lw), (r,), w in zip(cases, res, dev):
        a, t = _val(la), _val(lw)
        assert r % RR == a * t * INV9 % RR and r * RI9 <= RR * (RI9 + a) and (w <= M29).all()


def test_fr_lazy_butterflies_device_matches_host(ctx):
    """7 / 8 radix4<true|false>, 9 radix2 (the sequences ntt.hip runs): inputs anywhere below 2.1 r including its end, against the
    DIF levels of radix2/fft.rs on big integers; outputs back in range (< 2.1 r, or < 9.2 r with wide limbs in a last stage)."""
    rnd = rng(4)
    hi = 21 * RR // 10
    ends = [0, RR - 1, RR] + below(hi, 8)
    tw = [RR - 1, 1, 0]
    quads = [(a, b, c, d) for a in ends for b in ends for c in ends[:3] for d in ends[2:]]
    cases = [tuple(_l9(x) for x in xs) + tuple(_l9(t) for t in (tw[i % 3], tw[(i + 1) % 3], RR - 1)) for i, xs in enumerate(quads)]
    cases += [tuple(_l9(rnd.randrange(hi)) for _ in range(4)) + tuple(_l9(rnd.randrange(RR)) for _ in range(3)) for _ in range(N // 2)]
    m = lambda a, w: a * w * INV9 % RR
    for op in (7, 8):
        res, dev = _fr_run(ctx, op, cases)
        for c, ys, w in zip(cases, res, dev):
            xs = [_val(e) for e in c[:4]]
            wa, wb, wc = [_val(e) for e in c[4:]]
            d0, d1 = m(xs[0] - xs[2], wa), m(xs[1] - xs[3], wb)
            if op == 7:
                want = [sum(xs) % RR, m(xs[0] + xs[2] - xs[1] - xs[3], wc), (d0 + d1) % RR, m(d0 - d1, wc)]
                assert [y % RR for y in ys] == want and all(y < hi for y in ys) and (w <= M29).all()
            else:
                want = [sum(xs) % RR, (xs[0] + xs[2] - xs[1] - xs[3]) % RR, (d0 + d1) % RR, (d0 - d1) % RR]
                assert [y % RR for y in ys] == want and all(y < 92 * RR // 10 for y in ys) and (w < 2 ** 31.34).all()
    cases2 = [c[:2] + c[4:5] for c in cases]
    res, dev = _fr_run(ctx, 9, cases2)
    for c, ys, w in zip(cases2, res, dev):
        x0, x1, wa = [_val(e) for e in c]
        assert [y % RR for y in ys] == [(x0 + x1) % RR, m(x0 - x1, wa)] and all(y < 113 * RR // 100 for y in ys) and (w <= M29).all()


# ---- G2 lane pairs (msm_g2pair.hip), the dual forms of ec_dual.cuh (G2 quads, G1 pairs) --------------------------------------------
PAIR_NOUT = {0: 1, 1: 1, 2: 1, 3: 8, 4: 4, 5: 8, 6: 8, 7: 8, 8: 8}
PAIR_RANGES = (5 * Q + EPS, 3 * Q + EPS, Q + EPS, Q + EPS)      # madd_p_lazy / ec_dual.cuh: x, y, zz, zzz


def _pair_run(ctx, op, cases):
    """cases: tuples of Fq2 elements (c0, c1) for ops 0 - 6, of Fq values for 7, 8"""
    if op <= 6:
        rows = [[l for e in c for comp in e for l in _limbs_wide(comp)] for c in cases]
        _, out = _dev(ctx, "zk_diag_fq2_pair_dev", op, rows, PAIR_NOUT[op], 26)
        return [[(_val(e[:13]), _val(e[13:])) for e in o] for o in out], out
    rows = [[l for v in c for l in _limbs_wide(v)] for c in cases]
    _, out = _dev(ctx, "zk_diag_fq2_pair_dev", op, rows, PAIR_NOUT[op], 13)
    return [[_val(e) for e in o] for o in out], out


def _host_lazy(op, *vals):
    inp = np.array([l for v in vals for l in _limbs_wide(v)], dtype=np.uint32)
    out = np.zeros(13, dtype=np.uint32)
    assert Z.load().zk_fq_lazy_raw(op, _p(inp), _p(out)) == 0
    return out


def _mulp_l_host(a, b, split):
    """msm_g2pair.hip::mulp_l composed from the host build's primitives the way the lanes compose them (prep: the even lane's c
    operand is fp_neg5_almost(a1)): even a0 b0 + (-5 a1) b1, odd a0 b1 + a1 b0 -> each lane's raw limbs"""
    n5 = _val(_host_lazy(9, a[1]))
    op = 11 if split else 2
    return _host_lazy(op, a[0], b[0], n5, b[1]), _host_lazy(op, a[0], b[1], a[1], b[0])


def test_g2_pair_products_device_matches_the_lane_model(ctx):
    """0 mulp (reduced operands -> reduced result), 1 mulp_l<false> (left < 5p + eps, right < 7p + eps: R (Q - X3) and everything
    smaller), 2 mulp_l<true> (both up to 7p + 2 eps: P^2): fq2_mul on the residues; every range end on either lane and on both; the
    lazy forms word for word against the host build's fp_mul2_lazy / fp_neg5_almost composed lane by lane, and below (a b + c d) / RI + p."""
    rnd = rng(5)
    for op, la, lb in ((0, Q, Q), (1, 5 * Q + EPS, 7 * Q + EPS), (2, WIDE, WIDE)):
        ea, eb = fq_ends(la), fq_ends(lb)
        lefts = [(x, 0) for x in ea] + [(0, x) for x in ea] + [(x, x) for x in ea] + [(x, ea[-1]) for x in ea]
        cases = [(a, b) for a in lefts for b in [(eb[-1], 0), (0, eb[-1]), (eb[-1], eb[-2]), (1, 1), (eb[-2], eb[-1])]]
        cases += [((rnd.randrange(la), rnd.randrange(la)), (rnd.randrange(lb), rnd.randrange(lb))) for _ in range(N // 4)]
        res, out = _pair_run(ctx, op, cases)
        for k, ((a, b), (r,), w) in enumerate(zip(cases, res, out)):
            assert F2m.red(r) == F2m.mul(a, b), (op, a, b)
            if op == 0:
                assert r == F2m.mul(a, b)
                continue
            assert _normalised(w[0][:13]) and _normalised(w[0][13:])
            if k < 800 or k % 8 == 0:
                ev, od = _mulp_l_host(a, b, op == 2)
                assert (w[0][:13] == ev).all() and (w[0][13:] == od).all(), ("device != host lanes", op, a, b)
            t0, t1 = a[0] * b[0] + (Q + (Q >> 22)) * b[1], a[0] * b[1] + a[1] * b[0]
            assert r[0] * RI14 <= t0 + Q * RI14 and r[1] * RI14 <= t1 + Q * RI14, (op, a, b)
            assert max(r) < Q + (EPS if op == 1 else 2 * EPS), (op, a, b)


def _madd_special_cases(rnd, g2):
    """Accumulators with zz = 1 and X1 = U2 + (k q, d) or (d, k q), U2 the lazy value the device computes for q.x zz: P = U2 + 6q - X1
    then has one component a multiple of q (the general path must be taken) or both (then Y1 = S2 + j q or S2 + 1 decides doubling
    or infinity).  g2: Fq2 cases (the lanes disagree on "maybe a multiple of q"); otherwise G1."""
    one = RI14 % Q
    cases = []
    for _ in range(4):
        if g2:
            qx, qy, zz, zzz = (rnd.randrange(Q), rnd.randrange(Q)), (rnd.randrange(Q + 1), rnd.randrange(Q + 1)), (one, 0), (rnd.randrange(Q), 0)
            u2 = tuple(_val(x) for x in _mulp_l_host(qx, zz, False))
            s2 = tuple(_val(x) for x in _mulp_l_host(qy, zzz, False))
        else:
            qx, qy, zz, zzz = rnd.randrange(Q), rnd.randrange(Q + 1), one, rnd.randrange(Q)
            u2, s2 = _val(_host_lazy(0, qx, zz)), _val(_host_lazy(0, qy, zzz))
        for k in range(6):
            for d in (0, 1, Q - 1):
                for j in (0, 1, 2):
                    if g2:
                        y1 = (s2[0] + j * Q, s2[1] + j * Q) if j < 2 else (s2[0] + 1, s2[1])
                        for x1 in ((u2[0] + k * Q, u2[1] + d), (u2[0] + d, u2[1] + k * Q)):
                            if max(x1) < PAIR_RANGES[0] and max(y1) < PAIR_RANGES[1]:
                                cases.append(((x1, y1, zz, zzz), (qx, qy)))
                    else:
                        x1, y1 = u2 + k * Q + d, (s2 + j * Q if j < 2 else s2 + 1)
                        if x1 < PAIR_RANGES[0] and y1 < PAIR_RANGES[1]:
                            cases.append(((x1, y1, zz, zzz), (qx, qy)))
    return cases


@pytest.mark.parametrize("op", [3, 6])
def test_g2_pair_madd_device_matches_the_formula(ctx, op):
    """3: madd_p_lazy on lane pairs, 6: xyzz_madd_dual<G2QuadBase> on lane quads: lazy outputs in madd_p_lazy's ranges, canonical
    outputs equal to madd-2008-s on the residues (its doubling / infinity cases where P = 0 in Fq2); range ends put on one lane and
    not the other, the equal-x boundary cases above, random operands, the accumulator at infinity."""
    rnd = rng(6)
    ends = _acc_ends(PAIR_RANGES)
    cases = _madd_special_cases(rnd, True)
    for i in range(32):
        acc = tuple((ends[c][i % 4], ends[c][(i // 4) % 4] if i % 2 else 0) for c in range(4))
        cases.append((acc if i % 3 else tuple((b, a) for a, b in acc), ((Q - 1, i), (Q - i, Q))))
    cases += [(tuple((rnd.randrange(h), rnd.randrange(h)) for h in PAIR_RANGES), ((rnd.randrange(Q), rnd.randrange(Q)),
               (rnd.randrange(Q + 1), rnd.randrange(Q + 1)))) for _ in range(NP)]
    cases.append((((0, 0),) * 4, ((5, 6), (7, 8))))
    # P near 7q on BOTH lanes (X1 small, U2 = q.x zz near q): P^2's odd lane is P0 P1 + P1 P0 with four operands whose top limbs
    # overflow one 64-bit column unless the product splits it (mulp_l<true>, fp_mul2_lazy's TOPSPLIT)
    one = RI14 % Q
    for i in range(400):
        qx = (Q - 1 - rnd.randrange(Q >> 6), Q - 1 - rnd.randrange(Q >> 6)) if i else (Q - 1, Q - 1)
        x1 = (rnd.randrange(Q >> 6), rnd.randrange(Q >> 6)) if i else (0, 0)
        acc = (x1, (rnd.randrange(PAIR_RANGES[1]), rnd.randrange(PAIR_RANGES[1])), (one, 0), (rnd.randrange(Q), rnd.randrange(Q)))
        cases.append((acc, (qx, (rnd.randrange(Q + 1), rnd.randrange(Q + 1)))))
    res, _ = _pair_run(ctx, op, [acc + q for acc, q in cases])
    paths = set()
    for (acc, q), r in zip(cases, res):
        want = _madd_formula(F2m, list(acc), [q[0], F2m.red(q[1])])
        _check_point_out(F2m, r, want, PAIR_RANGES, (op, acc, q))
        p = F2m.sub(F2m.mul(q[0], acc[2]), acc[0])
        paths.add((p[0] == 0) + (p[1] == 0) if not F2m.zero(acc[2]) else -1)
    assert paths == {-1, 0, 1, 2}


def test_g2_pair_dbl_affine_device_matches_the_formula(ctx):
    rnd = rng(7)
    cases = [((rnd.randrange(Q), rnd.randrange(Q)), (rnd.randrange(Q), rnd.randrange(Q))) for _ in range(NP)]
    cases += [((Q - 1, Q - 1), (Q - 1, 0)), ((0, 1), (0, 0)), ((1, 0), (0, Q - 1)), ((Q - 1, 0), (0, 0))]
    res, _ = _pair_run(ctx, 4, cases)
    for q, r in zip(cases, res):
        assert r == _dbl_affine_formula(F2m, list(q)), q


@pytest.mark.parametrize("op", [5, 7])
def test_dual_add_device_matches_the_formula(ctx, op):
    """5: xyzz_add_dual<G2QuadOps> on lane quads, 7: xyzz_add_dual<G1DualOps> on lane pairs: operands anywhere in ec_dual.cuh's
    ranges (x < 5p + eps, y < 3p + eps, zz, zzz < p + eps), at their ends and at infinity, against add-2008-s on the residues."""
    rnd = rng(8)
    F = F2m if op == 5 else Fm
    ends = _acc_ends(PAIR_RANGES)
    if op == 5:
        r_, e_ = (lambda h: (rnd.randrange(h), rnd.randrange(h))), (lambda c, i: (ends[c][i % 4], ends[c][(i + 1) % 4] if i % 2 else 0))
    else:
        r_, e_ = (lambda h: rnd.randrange(h)), (lambda c, i: ends[c][i % 4])
    cases = [tuple(e_(c, i) for c in range(4)) + tuple(e_(c, i + 2) for c in range(4)) for i in range(16)]
    cases += [tuple(r_(h) for h in PAIR_RANGES) + tuple(r_(h) for h in PAIR_RANGES) for _ in range(NP)]
    z = (F.z,) * 4
    cases += [z + c[4:] for c in cases[:3]] + [c[:4] + z for c in cases[:3]] + [z + z]
    res, _ = _pair_run(ctx, op, cases)
    for c, r in zip(cases, res):
        _check_point_out(F, r, _add_formula(F, list(c[:4]), list(c[4:])), PAIR_RANGES, (op, c))


def test_g1_dual_madd_device_matches_the_formula(ctx):
    """8: xyzz_madd_dual<G1DualOps> (the small-job G1 accumulate) at the equal-x boundary cases and on random operands."""
    rnd = rng(9)
    cases = _madd_special_cases(rnd, False)
    cases += [(tuple(rnd.randrange(h) for h in PAIR_RANGES), (rnd.randrange(Q), rnd.randrange(Q + 1))) for _ in range(NP)]
    cases.append(((0, 0, 0, 0), (5, 6)))
    res, _ = _pair_run(ctx, 8, [acc + q for acc, q in cases])
    for (acc, q), r in zip(cases, res):
        _check_point_out(Fm, r, _madd_formula(Fm, list(acc), [q[0], q[1] % Q]), PAIR_RANGES, (acc, q))


# ---- chains over points of the curves: the accumulator stays in its lazy ranges between steps -------------------------------------
def _curve(g2):
    if g2:
        return F2m, O.g2_add, O.g2_mul, O.g2_neg, O.G2_GEN, O.fq2_inv, O.fq2_mul
    return Fm, O.g1_add, O.g1_mul, O.g1_neg, O.G1_GEN, (lambda v: pow(v, -1, Q)), (lambda a, b: a * b % Q)


def _to_int(g2, v):
    return tuple(t * RI14 % Q for t in v) if g2 else v * RI14 % Q


def _affine(g2, c):
    F, _, _, _, _, inv, mul = _curve(g2)
    x, y, zz, zzz = [F.red(v) for v in c]
    if F.zero(zz):
        return None
    frm = (lambda v: tuple(t * INV14 % Q for t in v)) if g2 else (lambda v: v * INV14 % Q)
    return (mul(frm(x), inv(frm(zz))), mul(frm(y), inv(frm(zzz))))


@pytest.mark.parametrize("op", [3, 6, 8, 10])
def test_madd_chains_land_on_the_group_law(ctx, op):
    """Chains of mixed additions over oracle points (G2: 3 madd_p_lazy, 6 the quad form; G1: 8 the pair form, 10 ec.cuh), 64
    independent chains per launch, the accumulator left in its lazy ranges between steps: P + Q, P + P, P + (-P), the accumulator at
    infinity (all-zero words, as the kernels keep it), negated table points given as q - y."""
    g2 = op in (3, 6)
    F, add, mul, neg, gen, _, _ = _curve(g2)
    prng = O.Prng(4242 + op)
    pts = [mul(gen, prng.fr()) for _ in range(10)]
    ranges = G1_RANGES if op == 10 else PAIR_RANGES
    n_ch, steps = 64, ["pt", "dbl", "pt", "neg", "pt", "pt", "negpt", "dbl", "pt", "neg", "pt", "dbl"]
    acc_pt = [pts[i % 10] for i in range(n_ch)]
    acc = [[_to_int(g2, p[0]), _to_int(g2, p[1]), F.one, F.one] for p in acc_pt]
    neg_y = (lambda y: tuple(Q - t for t in y)) if g2 else (lambda y: Q - y)      # kp_minus<1> per component
    for s, step in enumerate(steps):
        qs, qpts = [], []
        for i in range(n_ch):
            p = pts[(3 * i + s) % 10]
            if step in ("dbl", "neg") and acc_pt[i] is not None:
                x, y = _to_int(g2, acc_pt[i][0]), _to_int(g2, acc_pt[i][1])
                qs.append((x, y) if step == "dbl" else (x, neg_y(y)))
                qpts.append(acc_pt[i] if step == "dbl" else neg(acc_pt[i]))
            elif step == "negpt":
                qs.append((_to_int(g2, p[0]), neg_y(_to_int(g2, p[1]))))
                qpts.append(neg(p))
            else:
                qs.append((_to_int(g2, p[0]), _to_int(g2, p[1])))
                qpts.append(p)
        cases = [tuple(a) + q for a, q in zip(acc, qs)]
        res = (_fq_run(ctx, 10, cases) if op == 10 else _pair_run(ctx, op, cases))[0]
        for i in range(n_ch):
            acc_pt[i] = add(acc_pt[i], qpts[i])
            assert _affine(g2, res[i][4:]) == acc_pt[i], (op, step, i)
            for x, h in zip(res[i][:4], ranges):
                assert all(c < h for c in (x if g2 else (x,))), (op, step, i)
            acc[i] = res[i][:4] if acc_pt[i] is not None else [F.z] * 4


@pytest.mark.parametrize("op", [5, 7, 12])
def test_add_chains_land_on_the_group_law(ctx, op):
    """xyzz_add_dual (G2 quads: 5, G1 pairs: 7) and ec.cuh::xyzz_add_lazy (12) over oracle points in XYZZ form with random Z:
    P + Q, P + P, P + (-P), infinity on either side; the accumulator stays lazy between steps."""
    g2 = op == 5
    F, add, mul, neg, gen, _, fmul = _curve(g2)
    prng = O.Prng(777 + op)
    rnd = rng(op)
    pts = [mul(gen, prng.fr()) for _ in range(8)]
    ranges = G1_RANGES if op == 12 else PAIR_RANGES

    def xyzz(pt):
        if pt is None:
            return [F.z] * 4
        lam = (rnd.randrange(1, Q), rnd.randrange(Q)) if g2 else rnd.randrange(1, Q)
        zz = fmul(lam, lam)
        zzz = fmul(zz, lam)
        return [_to_int(g2, fmul(pt[0], zz)), _to_int(g2, fmul(pt[1], zzz)), _to_int(g2, zz), _to_int(g2, zzz)]

    n_ch, steps = 32, ["pt", "same", "pt", "neg", "pt", "inf", "pt", "same", "pt"]
    acc_pt = [pts[i % 8] for i in range(n_ch)]
    acc = [xyzz(p) for p in acc_pt]
    for s, step in enumerate(steps):
        bpts = []
        for i in range(n_ch):
            a = acc_pt[i]
            bpts.append({"same": a, "neg": None if a is None else neg(a), "inf": None}.get(step, pts[(5 * i + s) % 8]))
        cases = [tuple(a) + tuple(xyzz(b)) for a, b in zip(acc, bpts)]
        res = (_fq_run(ctx, 12, cases) if op == 12 else _pair_run(ctx, op, cases))[0]
        for i in range(n_ch):
            acc_pt[i] = add(acc_pt[i], bpts[i])
            assert _affine(g2, res[i][4:]) == acc_pt[i], (op, step, i)
            for x, h in zip(res[i][:4], ranges):
                assert all(c < h for c in (x if g2 else (x,))), (op, step, i)
            acc[i] = res[i][:4]


# ---- the SHE field (she.hip) ----------------------------------------------------------------------------------------------------------
F7_NOUT = {6: 2, 7: 2}


def _v26(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def _f7_run(ctx, op, cases):
    rows = [[l for e in c for l in e] for c in cases]
    _, out = _dev(ctx, "zk_diag_f7l_dev", op, rows, F7_NOUT.get(op, 1), 26)
    return [[_v26(e) for e in o] for o in out], out


def _spread26(v, rnd, wide):
    """v as 26 limbs with the lower ones pushed up to `wide` bits where v allows (all the way when rnd is None)"""
    limbs = l26(v)
    for i in range(24, -1, -1):
        room = min(((1 << wide) - 1 - limbs[i]) >> 29, limbs[i + 1])
        if room > 0:
            mv = rnd.randint(0, room) if rnd else room
            limbs[i] += mv << 29
            limbs[i + 1] -= mv
    assert _v26(limbs) == v
    return limbs


def test_she_lazy_field_at_its_range_ends(ctx):
    """f7l_red / add / sub<2|3> / mul / canon, the two butterflies and the negation of the pointwise product on the device, at the
    ends test_abi.py::test_she_lazy_domain_bounds proves the ranges for: congruent mod q, inside 2.01 q / 1.89 q, limbs < 2^29."""
    rnd = rng(10)
    q = q753()
    inv = pow(RI26, -1, q)
    ends = sorted(set(she_below_ends(q) + [0, 1, q - 1, q, 2 * q]))
    ok29 = lambda w: (w < (1 << 29)).all()
    r201, r189, r226 = 201 * q // 100, 189 * q // 100, 226 * q // 100
    # 0 red: any a < 7.9 q with limbs < 2^31 -> [0, 2.01 q)
    src = [v for v in ends if v < 79 * q // 10] + [rnd.randrange(79 * q // 10) for _ in range(N)]
    cases = [(l26(v),) for v in src] + [(_spread26(v, None, 31),) for v in src[:60]] + [(_spread26(v, rnd, 31),) for v in src[60:N // 2]]
    res, out = _f7_run(ctx, 0, cases)
    for (l,), (r,), w in zip(cases, res, out):
        v = _v26(l)
        assert r % q == v % q and r < r201 and ok29(w[0]), hex(v)
    # 1 add, 2 sub<2> (b < 1.89 q), 3 sub<3> (b < 2.26 q): exact, no limb wraps; a < 2.01 q
    for op, K, bmax in ((1, 0, r226), (2, 2, r189), (3, 3, r226)):
        bs = [v for v in ends if v < bmax] + below(bmax, 25)
        cases = [(l26(a), l26(b)) for a in ends if a < r201 for b in bs]
        cases += [(l26(rnd.randrange(r201)), l26(rnd.randrange(bmax))) for _ in range(N)]
        res, _ = _f7_run(ctx, op, cases)
        for (la, lb), (r,) in zip(cases, res):
            a, b = _v26(la), _v26(lb)
            assert r == (a + b if op == 1 else a + K * q - b), (op, hex(a), hex(b))
    # 4 mul: x < 2.26 q by a reduced y -> < 2 q; x < 2.01 q by a reduced y -> < 1.89 q; both < 2.01 q (the pointwise product) ->
    # < 2.79 q (its top limb may pass 29 bits: f7l_red takes it); never above (x y + q RI) / RI (the Montgomery digits are never 0)
    for amax, bmax, bound in ((r226, q, 2 * q), (r201, q, r189), (r201, r201, 279 * q // 100)):
        ea, eb = [v for v in ends if v < amax] + below(amax, 25), [v for v in ends if v < bmax] + below(bmax, 25)
        cases = [(l26(a), l26(b)) for a in ea for b in eb] + [(l26(rnd.randrange(amax)), l26(rnd.randrange(bmax))) for _ in range(N // 2)]
        res, out = _f7_run(ctx, 4, cases)
        for (la, lb), (r,), w in zip(cases, res, out):
            a, b = _v26(la), _v26(lb)
            assert r % q == a * b * inv % q and r * RI26 <= a * b + q * RI26 and r < bound, (hex(a), hex(b))
            assert ok29(w[0][:25]) and (ok29(w[0][25:]) or bound > r226), (hex(a), hex(b))
    # 5 canon (a < 2.01 q), 8 negation of the pointwise product (v < 2.01 q)
    src = [v for v in ends if v < r201] + [rnd.randrange(r201) for _ in range(N)]
    res, _ = _f7_run(ctx, 5, [(l26(v),) for v in src])
    assert all(r == v % q for v, (r,) in zip(src, res))
    res, out = _f7_run(ctx, 8, [(l26(v),) for v in src])
    for v, (r,), w in zip(src, res, out):
        assert (r + v) % q == 0 and r < r201 and ok29(w[0]), hex(v)
    # 6 forward butterfly (U < 2.01 q, V = x S < 1.89 q), 7 inverse (U, V < 2.01 q, S reduced)
    eu, ev = [v for v in ends if v < r201], [v for v in ends if v < r189]
    cases = [(l26(u), l26(v)) for u in eu for v in ev] + [(l26(rnd.randrange(r201)), l26(rnd.randrange(r189))) for _ in range(N)]
    res, out = _f7_run(ctx, 6, cases)
    for (lu, lv), (lo, hi), w in zip(cases, res, out):
        u, v = _v26(lu), _v26(lv)
        assert lo % q == (u + v) % q and hi % q == (u - v) % q and lo < r201 and hi < r201 and ok29(w), (hex(u), hex(v))
    cases = [(l26(u), l26(v), l26(s)) for u in eu for v in eu for s in (0, 1, q - 1)]
    cases += [(l26(rnd.randrange(r201)), l26(rnd.randrange(r201)), l26(rnd.randrange(q))) for _ in range(N)]
    res, out = _f7_run(ctx, 7, cases)
    for (lu, lv, ls), (lo, hi), w in zip(cases, res, out):
        u, v, s = _v26(lu), _v26(lv), _v26(ls)
        assert lo % q == (u + v) % q and hi % q == (u - v) * s * inv % q and lo < r201 and hi < r189 and ok29(w), (hex(u), hex(v))


def test_hooks_reject_bad_arguments(ctx):
    """An unknown op, a null pointer or an empty batch is ZK_ERR_ARG, never a launch."""
    buf = np.zeros(64 * 26 * 8, dtype=np.uint32)
    for fn, bad_op in (("zk_diag_fq_lazy_dev", 13), ("zk_diag_fr_lazy_dev", 11), ("zk_diag_fq2_pair_dev", 9), ("zk_diag_f7l_dev", 9)):
        f = getattr(ctx.lib, fn)
        for op, a, b, n in ((bad_op, buf, buf, 1), (-1, buf, buf, 1), (0, None, buf, 1), (0, buf, None, 1), (0, buf, buf, 0)):
            assert f(ctx.h, op, _p(a), _p(b), n) == -2, (fn, op, n)          # ZK_ERR_ARG
