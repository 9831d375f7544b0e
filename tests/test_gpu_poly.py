"""GPU parity: dense-polynomial kernels and KZG10 commit / open against the oracle."""
import numpy as np
import pytest

import marlin_ref as M
import ntt_cases as NC
import zkref as O
import zk_mpc_amd.convert as cv
from helpers import mont1

pytestmark = pytest.mark.gpu


def up(ctx, vals):
    return ctx.upload(cv.fr_to_mont(vals) if len(vals) else np.zeros((1, 4), dtype=np.uint64))


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 4096, 4097, 70000])
def test_evaluate_and_divide_by_linear(ctx, n):
    rng = O.Prng(3000 + n)
    c = [rng.fr() for _ in range(n)]
    d = up(ctx, c)
    for z in (rng.fr(), 0, 1, O.R_MOD - 1):
        assert cv.fr_from_mont(ctx.poly_evaluate_dev(d.ptr, n, mont1(z)).reshape(1, 4)) == [O.poly_evaluate(c, z)]
        q = ctx.alloc(max(n - 1, 1) * 32)
        rem = ctx.poly_divide_by_linear_dev(d.ptr, n, mont1(z), q.ptr)
        wq, wr = O.poly_divide_with_q_and_r(c, [(-z) % O.R_MOD, 1])
        assert cv.fr_from_mont(rem.reshape(1, 4)) == [O.poly_evaluate(c, z)]
        if n > 1:
            assert cv.fr_from_mont(ctx.download(q, (n - 1, 4))) == wq
            assert wr == [O.poly_evaluate(c, z)]


def test_evaluate_batch(ctx):
    """zk_poly_evaluate_batch_dev: pairs of different lengths (incl. empty, one coefficient, spans that end on a block edge,
    more than 256 spans so that the join folds several per thread) and different points, one call."""
    rng = O.Prng(3100)
    sizes = [0, 1, 15, 16, 17, 4095, 4096, 4097, 8192, 70001, (1 << 20) + 4097 + 5]
    polys, cs, pts = [], [], []
    keep = []
    for n in sizes:
        c = [rng.fr() for _ in range(min(n, 70001))]
        if n > len(c):                      # long one: a short random head, zeros, a random tail (Horner in python stays cheap)
            c = c[:300] + [0] * (n - 600) + c[300:600]
        d = up(ctx, c)
        keep.append(d)
        polys.append((d.ptr, n))
        cs.append(c)
        pts.append(rng.fr() if n != 16 else 0)
    out = ctx.poly_evaluate_batch_dev(polys, cv.fr_to_mont(pts))
    got = cv.fr_from_mont(out)

    def horner(c, z):
        acc, i = 0, len(c)
        nz = [(j, v) for j, v in enumerate(c) if v]
        return sum(v * pow(z, j, O.R_MOD) for j, v in nz) % O.R_MOD
    assert got == [horner(c, z) for c, z in zip(cs, pts)]
    assert ctx.poly_evaluate_batch_dev([], np.zeros((0, 4), dtype=np.uint64)).shape == (0, 4)


def test_divide_by_linear_beyond_256_spans(ctx):
    """More than 256 spans of 4096 coefficients: the one-block suffix scan of the spans folds two per thread."""
    rng = O.Prng(3200)
    n = (1 << 20) + 4097 + 3
    c = [rng.fr() for _ in range(2000)] + [0] * (n - 4000) + [rng.fr() for _ in range(2000)]
    z = rng.fr()
    d, q = up(ctx, c), ctx.alloc(n * 32)
    rem = ctx.poly_divide_by_linear_dev(d.ptr, n, mont1(z), q.ptr)
    want, acc = [0] * (n - 1), 0
    for i in range(n - 1, 0, -1):
        acc = (c[i] + acc * z) % O.R_MOD
        want[i - 1] = acc
    assert cv.fr_from_mont(ctx.download(q, (n - 1, 4))) == want
    assert cv.fr_from_mont(rem.reshape(1, 4)) == [(c[0] + acc * z) % O.R_MOD]


def test_divide_by_root_of_domain(ctx):
    """z inside the evaluation domain (where an evaluate-and-interpolate division would divide by zero)."""
    rng = O.Prng(31)
    n = 300
    c = [rng.fr() for _ in range(n)]
    z = O.Domain(512).element(5)
    d, q = up(ctx, c), ctx.alloc(n * 32)
    ctx.poly_divide_by_linear_dev(d.ptr, n, mont1(z), q.ptr)
    assert cv.fr_from_mont(ctx.download(q, (n - 1, 4))) == O.poly_divide_with_q_and_r(c, [(-z) % O.R_MOD, 1])[0]


@pytest.mark.parametrize("n,log_dom", [(5, 3), (8, 3), (9, 3), (100, 5), (1000, 8), (3000, 10), (5000, 0), (5001, 1), (100000, 2), (70000, 15)])
def test_divide_by_vanishing(ctx, n, log_dom):
    rng = O.Prng(3100 + n)
    c = [rng.fr() for _ in range(n)]
    N = 1 << log_dom
    d, q, r = up(ctx, c), ctx.alloc(max(n, 1) * 32), ctx.alloc(N * 32)
    ctx.poly_divide_by_vanishing_dev(d.ptr, n, log_dom, q.ptr, r.ptr)
    wq, wr = M.divide_by_vanishing(c, N)       # O(n); cross-checked against the generic long division in test_oracle.py
    if n <= 1000 and n > N:
        assert (wq, wr) == O.poly_divide_with_q_and_r(c, [O.R_MOD - 1] + [0] * (N - 1) + [1])
    nq = max(n - N, 0)
    assert cv.fr_from_mont(ctx.download(r, (N, 4))) == (wr + [0] * N)[:N]
    if nq:
        assert cv.fr_from_mont(ctx.download(q, (nq, 4))) == wq


def test_batch_inversion_and_powers(ctx):
    rng = O.Prng(32)
    n = 5000
    v = [rng.fr() for _ in range(n)]
    v[0], v[17], v[n - 1] = 0, 0, 1
    d = up(ctx, v)
    ctx.batch_inversion_dev(d.ptr, n)
    assert cv.fr_from_mont(ctx.download(d, (n, 4))) == O.batch_inversion(v)
    b, s = rng.fr(), rng.fr()
    out = ctx.alloc(1000 * 32)
    ctx.fr_powers_dev(mont1(b), mont1(s), 1000, out.ptr)
    assert cv.fr_from_mont(ctx.download(out, (1000, 4))) == [s * pow(b, i, O.R_MOD) % O.R_MOD for i in range(1000)]


@pytest.mark.parametrize("na,nb", [(1, 1), (3, 5), (64, 64), (100, 29)])
def test_poly_mul(ctx, na, nb):
    rng = O.Prng(3200 + na)
    a, b = [rng.fr() for _ in range(na)], [rng.fr() for _ in range(nb)]
    da, db, out = up(ctx, a), up(ctx, b), ctx.alloc((na + nb) * 32)
    ctx.poly_mul_dev(da.ptr, na, db.ptr, nb, out.ptr)
    assert cv.fr_from_mont(ctx.download(out, (na + nb - 1, 4))) == O.poly_mul(a, b)


R = O.R_MOD
R2 = NC.MONT * NC.MONT % R          # a residue x R inverts to x^-1 R = (x R)^-1 R^2


def inv_chunk(n):
    """Elements per lane of zk_fr_batch_inverse_dev: 8 / 16 / 32 while <= 2048 chunk totals go to the host, 32 in k_batch_inverse."""
    ch = 8
    while ch < 32 and (n + ch - 1) // ch > 2048:
        ch *= 2
    return ch


@pytest.mark.parametrize("n", [1, 7, 8, 9, 16384, 16385, 32768, 32769, 65536, 65537, (1 << 20) + 3])
def test_batch_inversion_dispatch_seams(ctx, n):
    """zk_fr_batch_inverse_dev on both sides of each of its four paths (host-inverted chunk totals with 8, 16, 32 elements per
    lane up to 16 384 / 32 768 / 65 536 elements, the one-kernel form above), with zeros where the chunk walk could trip: none,
    all, one whole chunk, the whole (partial) last chunk, the first and last slot of a chunk, index 0 and n - 1.  The values 1,
    -1 and the residue r - 1 are in every vector.  Reference: pow(x, -1, r), zeros left zero (from 2^20 on Montgomery's trick in
    python, held to x * inv == 1 on every element)."""
    ch = inv_chunk(n)
    v = NC.uniform(np.random.RandomState(4000 + n % 1000), n)
    special = NC.limbs([NC.MONT, R - NC.MONT, R - 1])
    for k in range(min(3, n - 1)):
        v[n // 3 + k] = special[k]
    xs = NC.ints(v)
    assert all(xs)
    if n <= 1 << 17:
        inv = [pow(x, -1, R) * R2 % R for x in xs]
    else:
        pre, run = [], 1
        for x in xs:
            pre.append(run)
            run = run * x % R
        acc, inv = pow(run, -1, R), [0] * n
        for i in range(n - 1, -1, -1):
            inv[i] = acc * pre[i] % R * R2 % R
            acc = acc * xs[i] % R
    assert all(x * y % R == R2 for x, y in zip(xs, inv))
    want = NC.limbs(inv)
    mid = (((n + ch - 1) // ch) // 2) * ch
    mid_end = min(n, mid + ch)
    last = ((n - 1) // ch) * ch
    patterns = {"none": [], "all": range(n), "chunk": range(mid, mid_end), "last_chunk": range(last, n),
                "chunk_edges": [mid, mid_end - 1], "ends": [0, n - 1]}
    for name, zeros in patterns.items():
        zeros = np.array(list(zeros), dtype=np.int64)
        a, w = v.copy(), want.copy()
        a[zeros] = 0
        w[zeros] = 0
        d = ctx.upload(a)
        ctx.batch_inversion_dev(d.ptr, n)
        bad = NC.mismatch(ctx.download(d, (n, 4)), w)
        d.free()
        assert bad is None, "zeros '%s', %d elements per lane: %s" % (name, ch, bad)


@pytest.mark.parametrize("n", [1, 8, 9, 65536, 65537, (1 << 20) + 5])
def test_powers_dispatch_seam(ctx, n):
    """zk_fr_powers_dev on both sides of its switch from 8 to 32 powers per lane (n = 2^16) and at lane ends, for the bases
    0, 1, -1, a 2^10-th root of unity (the sequence has to cycle exactly) and random, from the starts 0, 1 and random."""
    rng = O.Prng(4100 + n % 1000)
    root = O.Domain(1 << 10).group_gen
    out = ctx.alloc(n * 32)
    for base in (0, 1, R - 1, root, rng.fr()):
        for start in (0, 1, rng.fr()):
            ctx.fr_powers_dev(mont1(base), mont1(start), n, out.ptr)
            got = ctx.download(out, (n, 4))
            bad = NC.mismatch(got, NC.geometric(NC.mont(start), base, n))
            assert bad is None, "base %x start %x: %s" % (base, start, bad)
            if base == root and n > 1024:
                assert np.array_equal(got[1024:], got[:-1024])
    out.free()


def horner(c, z):
    acc = 0
    for x in reversed(c):
        acc = (acc * z + x) % R
    return acc


@pytest.mark.parametrize("na,nb", [(600, 425), (600, 426), (2500, 1597), (2500, 1598), ((1 << 19) + 7, (1 << 19) - 6),
                                   ((1 << 19) + 7, (1 << 19) - 5)])
def test_poly_mul_pass_seams(ctx, na, nb):
    """zk_poly_mul_dev with na + nb - 1 on both sides of 2^10 (one-pass -> two-pass transforms), 2^12 and 2^20 (two -> three
    passes).  Operands, all as residues x R:
      random x random -- against the schoolbook product O.poly_mul up to 2^12; above, a(z) b(z) == out(z) at two random z by
        Horner in python (a wrong product passes one point with probability at most degree / r < 2^-230);
      sparse x dense -- a has five non-zero terms (both ends among them), so the product is five shifted multiples of b;
      all r - 1 x all r - 1 -- maximal residues: out[k] = c^2 * #{(i, j): i + j = k}."""
    nout = na + nb - 1
    rs = np.random.RandomState(na + nb)
    rinv = pow(NC.MONT, -1, R)

    def product(a, b):
        da, db, out = ctx.upload(a), ctx.upload(b), ctx.alloc((nout + 1) * 32)
        ctx.poly_mul_dev(da.ptr, na, db.ptr, nb, out.ptr)
        got = ctx.download(out, (nout, 4))
        for buf in (da, db, out):
            buf.free()
        assert NC.below_r(got).all()
        return got

    # random x random
    a, b = NC.uniform(rs, na), NC.uniform(rs, nb)
    ai, bi = NC.ints(a), NC.ints(b)
    got = product(a, b)
    if nout <= 1 << 13:
        assert NC.mismatch(got, NC.limbs(x * rinv % R for x in O.poly_mul(ai, bi))) is None
    else:
        gi = NC.ints(got)
        for z in (O.Prng(na).fr(), O.Prng(nb).fr()):
            assert horner(ai, z) * horner(bi, z) % R == horner(gi, z) * NC.MONT % R
    # sparse x dense
    terms = {0: ai[0], 1: R - 1, na // 2: NC.MONT, na - 2: ai[na - 2], na - 1: R - NC.MONT}
    sp = np.zeros((na, 4), dtype=np.uint64)
    want = [0] * nout
    for pos, c in terms.items():
        sp[pos] = NC.limbs([c])[0]
        cr = c * rinv % R
        for j, y in enumerate(bi):
            want[pos + j] += cr * y
    bad = NC.mismatch(product(sp, b), NC.limbs(x % R for x in want))
    assert bad is None, "sparse x dense: %s" % bad
    # all r - 1
    top = NC.limbs([R - 1])[0]
    k = np.arange(nout, dtype=np.int64)
    count = np.minimum(np.minimum(k + 1, nout - k), min(na, nb))
    c2 = (R - 1) * (R - 1) * rinv % R
    want = NC.limbs(c2 * m % R for m in count.tolist())
    bad = NC.mismatch(product(np.tile(top, (na, 1)), np.tile(top, (nb, 1))), want)
    assert bad is None, "all r - 1: %s" % bad


def test_kzg10_commit_open_check(ctx):
    """KZG10 with and without hiding: commitments / proofs equal the oracle's and satisfy the pairing check."""
    rng = O.Prng(33)
    deg = 40
    beta = rng.fr()
    pp = O.KzgParams(deg, beta, g_k=rng.fr(), gg_k=rng.fr(), h_k=rng.fr())
    pg = ctx.bases_upload(cv.g1_affine_to_array(pp.powers_of_g), 1)
    pgg = ctx.bases_upload(cv.g1_affine_to_array(pp.powers_of_gamma_g), 1)
    coeffs = [rng.fr() for _ in range(deg + 1)]
    blind = [rng.fr() for _ in range(3)]
    dc, dbl = up(ctx, coeffs), up(ctx, blind)
    z = rng.fr()
    v = O.poly_evaluate(coeffs, z)
    # no hiding
    c0 = cv.g1_projective_to_affine(ctx.kzg_commit_dev(pg, dc.ptr, deg + 1))
    assert c0 == O.kzg_commit(pp, coeffs)
    w0, _ = ctx.kzg_open_dev(pg, dc.ptr, deg + 1, mont1(z))
    w0 = cv.g1_projective_to_affine(w0)
    assert w0 == O.kzg_open(pp, coeffs, z)[0]
    assert O.kzg_check(pp, c0, z, v, w0)
    assert not O.kzg_check(pp, c0, z, (v + 1) % O.R_MOD, w0)
    # hiding bound 2 (blinding polynomial of degree 2)
    c1 = cv.g1_projective_to_affine(ctx.kzg_commit_dev(pg, dc.ptr, deg + 1, pgg, dbl.ptr, 3))
    assert c1 == O.kzg_commit(pp, coeffs, blind)
    w1, rv = ctx.kzg_open_dev(pg, dc.ptr, deg + 1, mont1(z), pgg, dbl.ptr, 3)
    w1, rv = cv.g1_projective_to_affine(w1), cv.fr_from_mont(rv.reshape(1, 4))[0]
    ow, orv = O.kzg_open(pp, coeffs, z, blind)
    assert (w1, rv) == (ow, orv)
    assert O.kzg_check(pp, c1, z, v, w1, rv)
