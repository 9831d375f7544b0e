"""GPU parity, exact: the SHE ring kernels (csrc/she.hip) against the references of she_cases.py at every transform size, every
row layout and the ends of the operand range.  No tolerance anywhere: every check is bit equality of 12 x u64 Montgomery words
with the words of the canonical reference value, which also proves the device's outputs reduced.

What a size reaches (TILE = 1024 elements in LDS, 10 levels per tile pass):

#      N   path
#  1..3, 100   k_she_schoolbook (N < 4 or not a power of two)
#  4..512      k_she_fwd_tile<true> / k_she_inv_tile<true>, 1024 / N polynomials per tile
#  1024        the same, one polynomial per tile
#  2048        k_she_gather, 1 global level (log_t 10) each way, k_she_inv_global<true> alone
#  4096        2 global levels: log_t 11, 10 forward; k_she_inv_global<false> once, then <true>
#  8192        3 global levels
#  16384       4 global levels: log_t 13 .. 10; k_she_inv_global<false> three times
"""
import functools
import random

import numpy as np
import pytest

import she_cases as SC
import zkref as O
import zk_mpc_amd as Z
import zk_mpc_amd.convert as cv
from zk_mpc_amd import _lib

pytestmark = pytest.mark.gpu

P12 = cv.fq753_to_mont([O.R_MOD])[0]


def flat(rows) -> list:
    return [x for r in rows for x in r]


def up(ctx, rows):
    return ctx.upload(SC.words(flat(rows)))


def down(ctx, buf, count):
    return ctx.download(buf, (count, 12))


def hold(got, want_rows, n, label):
    """The downloaded words against the canonical reference rows: reduced, and bit-equal."""
    assert SC.all_below_q(got), "%s: an output word pattern is not below q" % label
    bad = SC.mismatch(got, SC.words(flat(want_rows)), n)
    assert bad is None, "%s: %s" % (label, bad)


def device_mul(ctx, a_rows, b_rows, n):
    batch = len(a_rows)
    da, db, out = up(ctx, a_rows), up(ctx, b_rows), ctx.alloc(batch * n * 96)
    try:
        ctx.encodedtext_mul_dev(da.ptr, db.ptr, out.ptr, n, batch)
        return down(ctx, out, batch * n)
    finally:
        for d in (da, db, out):
            d.free()


@functools.lru_cache(maxsize=None)
def random_pair(n, i):
    """Row i of the random operands of size n and their product; computed once, shared by the batch, interleave and grid-stride
    tests, never modified (tuples)."""
    a, b = SC.family("random", n, 10 + 2 * i), SC.family("random", n, 11 + 2 * i)
    return tuple(a), tuple(b), tuple(SC.ring_mul(a, b))


# ---- a. the negacyclic product at every transform size ---------------------------------------------------------------------
PRODUCT_CASES = [(k, case) for k in range(2, 15) for case in SC.product_cases(1 << k)]


@pytest.mark.parametrize("log_n,case", PRODUCT_CASES, ids=["2^%d-%s-x-%s" % (k, c[0], c[1]) for k, c in PRODUCT_CASES])
def test_product_every_size(ctx, log_n, case):
    """zk_she_negacyclic_mul_dev == ring_mul (the oracle's product below 4, Kronecker substitution up to 4096, the plain transform
    above), whole polynomial.  Uniform operands in [0, q) -- not products of Fr draws; every coefficient q - 1, which drives the
    lazy butterflies with maximal operands through all levels; the element stored as the words of q - 1; q - 1 / 1 alternating
    times a 0 / q - 1 mask; X^k for k = 0, 1, N / 2, N - 1.  Where the pair has a closed form (2k + 2 - N; the signed rotation)
    the reference is held against it too, so both stand on the definition."""
    n = 1 << log_n
    a, b = SC.case_operands(case, n)
    want = SC.ring_mul(a, b)
    closed = SC.closed_form(case, n, a, b)
    assert closed is None or closed == want
    hold(device_mul(ctx, [a], [b], n), [want], n, "%s x %s at N = %d" % (case[0], case[1], n))


# ---- b. batches and tile seams ---------------------------------------------------------------------------------------------
def random_rows(n, batch, first=0):
    pairs = [random_pair(n, first + i) for i in range(batch)]
    return [p[0] for p in pairs], [p[1] for p in pairs], [p[2] for p in pairs]


@pytest.mark.parametrize("n,batch", [(4, 300), (512, 3), (1024, 3), (2048, 3), (4096, 2), (16384, 2), (3, 5), (100, 3), (1, 4)])
def test_product_batches(ctx, n, batch):
    """Another polynomial in every row: 256 polynomials per tile with a partial last tile; a pair per tile and a half-filled
    tile; one per tile; the row index g >> (log_n - 1) of the global kernels at one, two and four global levels; schoolbook."""
    a, b, want = random_rows(n, batch)
    hold(device_mul(ctx, a, b, n), want, n, "N = %d, batch %d" % (n, batch))


def test_interleaved_sizes_regrow_scratch():
    """One fresh context, sizes and batches interleaved and growing: she_fa, she_fb and she_inv_work are freed and allocated again
    between calls while the per-size tables stay cached."""
    c = Z.Context(0)
    try:
        for n, batch in ((2048, 1), (4096, 1), (2048, 3), (512, 2), (4096, 2), (2048, 2), (1024, 3)):
            a, b, want = random_rows(n, batch)
            hold(device_mul(c, a, b, n), want, n, "N = %d, batch %d (interleaved)" % (n, batch))
    finally:
        c.close()


# ---- c. the grid-stride loops ----------------------------------------------------------------------------------------------
def test_grid_stride():
    """N = 2048, 1025 rows: 1 049 600 butterflies per level and 2 099 200 elements, past the 4096 x 256 threads a launch is capped
    at, so the loops of k_she_gather, k_she_fwd_global, k_she_inv_global and k_she_vec_op go round again.  Row r holds pair
    r mod 3 of three random ones (1025 = 1 mod 3: a row index taken modulo 1024 would put pair 0 where pair 1 belongs).  About
    1.2 GB of device memory, on a context of its own that gives it back."""
    n, rows, reps = 2048, 1025, 342
    pairs = [random_pair(n, i) for i in range(3)]
    tiled = lambda polys: np.tile(np.stack([SC.words(list(p)) for p in polys]), (reps, 1, 1))[:rows].reshape(rows * n, 12)
    wa, wb = tiled([p[0] for p in pairs]), tiled([p[1] for p in pairs])
    c = Z.Context(0)
    try:
        da, db, out = c.upload(wa), c.upload(wb), c.alloc(rows * n * 96)
        c.encodedtext_mul_dev(da.ptr, db.ptr, out.ptr, n, rows)
        bad = SC.mismatch(down(c, out, rows * n), tiled([p[2] for p in pairs]), n)
        assert bad is None, "product: %s" % bad
        for op, f in ((_lib.OP_SUB, lambda x, y: (x - y) % SC.Q), (_lib.OP_MUL, lambda x, y: x * y % SC.Q)):
            c.she_vec_op_dev(op, da.ptr, db.ptr, out.ptr, rows * n)
            bad = SC.mismatch(down(c, out, rows * n), tiled([[f(x, y) for x, y in zip(p[0], p[1])] for p in pairs]), n)
            assert bad is None, "vec op %d: %s" % (op, bad)
    finally:
        c.close()


# ---- d. ciphertext product, encrypt, decrypt across the tile -----------------------------------------------------------------
def ct_rows(cts):
    return [flat(ct) for ct in cts]


@pytest.mark.parametrize("n,batch", [(4, 3), (512, 3), (1024, 3), (2048, 3), (4096, 1), (16384, 1), (3, 2), (100, 2)])
def test_ciphertext_ops(ctx, n, batch):
    """The callers of the row maps rpg = 2 / gstride = 3n and gstride = 0, of the two-product and the negated k_she_inv_tile, and
    above the tile of k_she_gather with those maps, of k_she_inv_global<true> writing through row_elem, and of the canon = 1
    forward of decrypt.  A dense uniform public key; r dense uniform in row 0 (u p and w p on full-width operands) and small in
    the other rows; ciphertext i times ciphertext i + 1 (mod batch); decrypt of the fresh ciphertexts (c2 = 0) and of the
    degree-2 products."""
    rng = random.Random(730 + n)
    sk = [rng.randrange(11) for _ in range(n)]
    pk_a, pk_b = SC.uniform_q(rng, n), SC.uniform_q(rng, n)
    e = [SC.uniform_q(rng, n) for _ in range(batch)]
    r = [SC.uniform_q(rng, 3 * n) if i == 0 else [rng.randrange(11) for _ in range(3 * n)] for i in range(batch)]
    dsk, dpa, dpb, de, dr = up(ctx, [sk]), up(ctx, [pk_a]), up(ctx, [pk_b]), up(ctx, e), up(ctx, r)
    ct, prod, dec = ctx.alloc(batch * 3 * n * 96), ctx.alloc(batch * 3 * n * 96), ctx.alloc(batch * n * 96)
    try:
        ctx.ciphertext_encrypt_from_dev(de.ptr, dpa.ptr, dpb.ptr, dr.ptr, P12, ct.ptr, n, batch)
        want_ct = [SC.ct_encrypt(e[i], pk_a, pk_b, r[i]) for i in range(batch)]
        hold(down(ctx, ct, batch * 3 * n), ct_rows(want_ct), n, "encrypt")
        ctx.ciphertext_decrypt_dev(ct.ptr, dsk.ptr, dec.ptr, n, batch)
        hold(down(ctx, dec, batch * n), [SC.ct_decrypt(c, sk) for c in want_ct], n, "decrypt of a fresh ciphertext")
        drot = up(ctx, ct_rows([want_ct[(i + 1) % batch] for i in range(batch)]))
        ctx.ciphertext_mul_dev(ct.ptr, drot.ptr, prod.ptr, n, batch)
        drot.free()
        want_prod = [SC.ct_mul(want_ct[i], want_ct[(i + 1) % batch]) for i in range(batch)]
        hold(down(ctx, prod, batch * 3 * n), ct_rows(want_prod), n, "ciphertext product")
        ctx.ciphertext_decrypt_dev(prod.ptr, dsk.ptr, dec.ptr, n, batch)
        hold(down(ctx, dec, batch * n), [SC.ct_decrypt(c, sk) for c in want_prod], n, "decrypt of a product")
    finally:
        for d in (dsk, dpa, dpb, de, dr, ct, prod, dec):
            d.free()


@pytest.mark.parametrize("n,batch", [(1024, 3), (2048, 3)])
def test_ciphertext_mul_maximal(ctx, n, batch):
    """q - 1 in every component of both ciphertexts: c1 = x0 y1 + x1 y0 is then the largest sum f7l_red takes after the pointwise
    stage, and c2 goes through f7l_negate.  All rows are equal, so this says nothing about rows; test_ciphertext_ops does."""
    top = ([SC.Q - 1] * n,) * 3
    want = SC.ct_mul(top, top)
    assert want[0] == SC.all_top_squared(n) and want[2] == O.texts_neg(want[0]) and want[1] == O.texts_add(want[0], want[0])
    dx, prod = up(ctx, ct_rows([top] * batch)), ctx.alloc(batch * 3 * n * 96)
    try:
        ctx.ciphertext_mul_dev(dx.ptr, dx.ptr, prod.ptr, n, batch)
        hold(down(ctx, prod, batch * 3 * n), ct_rows([want] * batch), n, "all q - 1")
    finally:
        dx.free()
        prod.free()


# ---- e. encode and decode --------------------------------------------------------------------------------------------------
def chunks(vectors, batch):
    """Lists of `batch` vectors; the last one filled up with the first vector."""
    out = [vectors[i:i + batch] for i in range(0, len(vectors), batch)]
    out[-1] = out[-1] + [vectors[0]] * (batch - len(out[-1]))
    return out


@pytest.mark.parametrize("batch", [1, 3])
@pytest.mark.parametrize("n", [1, 2, 4, 1024, 2048, 16384])
def test_encode_decode(ctx, n, batch):
    """zk_she_encode_dev == encode_fast on random slots, all r - 1, all equal (only coefficient 0 is non-zero) and one non-zero
    slot; zk_she_decode_dev == decode_fast on those encodings (the round trip), on uniform Fq coefficients and on the ends of the
    centred lift and of the 26-limb fold: 0, 1, q/2 - 1, q/2, q/2 + 1, q - 1, q - (q mod r), q mod r, r, r - 1."""
    rng = random.Random(740 + n)
    single = [0] * n
    single[n // 3] = rng.randrange(1, SC.R)
    slots = [SC.uniform_r(rng, n), [SC.R - 1] * n, [rng.randrange(1, SC.R)] * n, single, SC.uniform_r(rng, n), SC.uniform_r(rng, n)]
    want_enc = [SC.encode_fast(v) for v in slots]
    assert not any(want_enc[2][1:]) and want_enc[2][0] == slots[2][0]
    enc, back = ctx.alloc(batch * n * 96), ctx.alloc(batch * n * 32)
    try:
        for vs, ws in zip(chunks(slots, batch), chunks(want_enc, batch)):
            dpt = ctx.upload(cv.fr_to_mont(flat(vs)))
            ctx.plaintexts_encode_dev(dpt.ptr, enc.ptr, n, batch)
            dpt.free()
            hold(down(ctx, enc, batch * n), ws, n, "encode")
            ctx.encodedtext_decode_dev(enc.ptr, back.ptr, n, batch)
            bad = SC.mismatch(ctx.download(back, (batch * n, 4)), cv.fr_to_mont(flat(vs)), n)
            assert bad is None, "round trip: %s" % bad
        ends = [[SC.LIFT_ENDS[(i * n + j) % len(SC.LIFT_ENDS)] for j in range(n)] for i in range(-(-len(SC.LIFT_ENDS) // n))]
        assert set(flat(ends)) == set(SC.LIFT_ENDS)
        coeffs = [SC.uniform_q(rng, n), SC.uniform_q(rng, n)] + ends
        for cs in chunks(coeffs, batch):
            dq = up(ctx, cs)
            ctx.encodedtext_decode_dev(dq.ptr, back.ptr, n, batch)
            dq.free()
            bad = SC.mismatch(ctx.download(back, (batch * n, 4)), cv.fr_to_mont(flat([SC.decode_fast(c) for c in cs])), n)
            assert bad is None, "decode: %s" % bad
    finally:
        enc.free()
        back.free()


# ---- f. aliasing -----------------------------------------------------------------------------------------------------------
def ring_calls(ctx, n, batch):
    """name -> (input sizes in elements, output size, call(input pointers, out pointer))."""
    return {
        "zk_she_negacyclic_mul_dev": ([batch * n, batch * n], batch * n,
                                      lambda p, o: ctx.encodedtext_mul_dev(p[0], p[1], o, n, batch)),
        "zk_she_ciphertext_mul_dev": ([batch * 3 * n, batch * 3 * n], batch * 3 * n,
                                      lambda p, o: ctx.ciphertext_mul_dev(p[0], p[1], o, n, batch)),
        "zk_she_encrypt_dev": ([batch * n, n, n, batch * 3 * n], batch * 3 * n,
                               lambda p, o: ctx.ciphertext_encrypt_from_dev(p[0], p[1], p[2], p[3], P12, o, n, batch)),
        "zk_she_decrypt_dev": ([batch * 3 * n, n], batch * n,
                               lambda p, o: ctx.ciphertext_decrypt_dev(p[0], p[1], o, n, batch)),
    }


@pytest.mark.parametrize("name", ["zk_she_negacyclic_mul_dev", "zk_she_ciphertext_mul_dev", "zk_she_encrypt_dev", "zk_she_decrypt_dev"])
@pytest.mark.parametrize("n", [3, 1024])
def test_ring_calls_refuse_overlap(ctx, name, n):
    """The four ring calls with the output on top of each input (the first, the second, ...), one element into it from either
    side, and just touching its last element: each is refused with an error that names the call, on the schoolbook path and on
    the transform path alike, and leaves every input as it was.  The same call with the output next to the inputs passes.  All
    ranges lie inside one allocation with room for the output before and after the inputs."""
    batch = 2
    sizes, out_elems, call = ring_calls(ctx, n, batch)[name]
    rng = random.Random(n)
    image = SC.words(SC.uniform_q(rng, 2 * out_elems + sum(sizes)))
    arena = ctx.upload(image)
    try:
        ptrs, at = [], out_elems
        for s in sizes:
            ptrs.append(arena.ptr + 96 * at)
            at += s
        for p, s in zip(ptrs, sizes):
            for out in (p, p + 96, p - 96, p + 96 * (s - 1), p - 96 * (out_elems - 1)):
                with pytest.raises(Z.ZkError, match=name):
                    call(ptrs, out)
        assert SC.mismatch(down(ctx, arena, len(image)), image, n) is None, "a refused call wrote"
        call(ptrs, arena.ptr)                                  # the room before the inputs: no overlap
        got = down(ctx, arena, len(image))
        assert SC.mismatch(got[out_elems:], image[out_elems:], n) is None
        assert not np.array_equal(got[:out_elems], image[:out_elems])
    finally:
        arena.free()


def test_elementwise_in_place(ctx):
    """zk_she_vec_op_dev and zk_she_vec_scale_dev stay legal in place: out on a, out on b."""
    n = 300
    rng = random.Random(7)
    a, b, k = SC.uniform_q(rng, n), SC.uniform_q(rng, n), rng.randrange(SC.Q)
    a[0], b[0], a[1], b[1] = SC.Q - 1, SC.Q - 1, 0, SC.Q - 1
    ops = ((_lib.OP_ADD, lambda x, y: (x + y) % SC.Q), (_lib.OP_SUB, lambda x, y: (x - y) % SC.Q),
           (_lib.OP_MUL, lambda x, y: x * y % SC.Q))
    for op, f in ops:
        for on_a in (True, False):
            da, db = up(ctx, [a]), up(ctx, [b])
            ctx.she_vec_op_dev(op, da.ptr, db.ptr, (da if on_a else db).ptr, n)
            hold(down(ctx, da if on_a else db, n), [[f(x, y) for x, y in zip(a, b)]], n, "op %d in place" % op)
            hold(down(ctx, db if on_a else da, n), [b if on_a else a], n, "the other operand of op %d" % op)
            da.free()
            db.free()
    da = up(ctx, [a])
    ctx.she_vec_op_dev(_lib.OP_NEG, da.ptr, None, da.ptr, n)
    hold(down(ctx, da, n), [O.texts_neg(a)], n, "neg in place")
    ctx.she_vec_scale_dev(da.ptr, SC.words([k])[0], da.ptr, n)
    hold(down(ctx, da, n), [O.encodedtext_scale(O.texts_neg(a), k)], n, "scale in place")
    da.free()
