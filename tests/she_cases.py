"""References, operand families and closed forms for the SHE ring kernels (csrc/she.hip), shared by test_she_model.py (the
references against the oracle and against each other, on the CPU) and test_gpu_she_exact.py (the device against them).  No GPU
code here.  Everything is a list of canonical python integers: coefficients of F_q[X] / (X^N + 1) below q = the MNT4-753 base
prime, or Fr slots below r.  The oracle's own product (zkref.encodedtext_mul) is O(N^2) on 753-bit integers -- 3 s at N = 1024 --
so two exact products that reach N = 2^14 stand next to it:

  kron_mul   Kronecker substitution: one big-integer product, no root of unity anywhere (a different algorithm from the kernel's)
  ntt_mul    a plain recursive negacyclic transform: twist by psi^i, radix-2 DFT in natural order, pointwise product, inverse;
             no lazy domain, no bit reversal, no tiling (the kernel's algorithm, none of its schedule)

The transform is generic over the modulus: over Fr with the root of zkref.cyclotomic_moduli it IS Plaintexts::encode /
Encodedtext::decode, because forward(a)[k] = a(psi^(2k+1)) and the slots sit at zeta^(2i+1) in natural order."""
import random

import numpy as np

import zkref as O
import zk_mpc_amd.convert as cv

Q = O.Q753
R = O.R_MOD
Q_GENERATOR = O.Q753_GENERATOR          # 17, a generator of F_q^*
MONT_R_INV = pow(1 << 768, -1, Q)
RESIDUE_TOP = (Q - 1) * MONT_R_INV % Q  # the element stored as the words of q - 1


def is_pow2(n: int) -> bool:
    return n > 0 and not n & (n - 1)


def transform_path(n: int) -> bool:
    """The sizes she.hip sends through the negacyclic transform; every other N takes the O(N^2) schoolbook kernel."""
    return is_pow2(n) and 4 <= n <= 1 << 14


# ---- the plain transform --------------------------------------------------------------------------------------------------
def psi_q(n: int) -> int:
    """A primitive 2N-th root of unity of F_q."""
    assert (Q - 1) % (2 * n) == 0
    return pow(Q_GENERATOR, (Q - 1) // (2 * n), Q)


def zeta_r(n: int) -> int:
    """The primitive 2N-th root of Fr whose odd powers are the slots (zkref.cyclotomic_moduli, natural order)."""
    return O.cyclotomic_moduli(n)[0]


def _powers(w: int, n: int, mod: int) -> list:
    out, x = [1] * n, 1
    for i in range(1, n):
        x = x * w % mod
        out[i] = x
    return out


def _dft(v, tw, stride, mod, wrong_top=False):
    """out[k] = sum_i v[i] w^(i k), natural order in and out; tw[j] = w_top^j, this level's root is w_top^stride."""
    n = len(v)
    if n == 1:
        return list(v)
    e = _dft(v[0::2], tw, 2 * stride, mod)
    o = _dft(v[1::2], tw, 2 * stride, mod)
    h = n // 2
    out = [0] * n
    for k in range(h):
        x = o[k] * tw[((k ^ 1) if wrong_top and h > 1 else k) * stride] % mod
        out[k] = (e[k] + x) % mod
        out[k + h] = (e[k] - x) % mod
    return out


def forward(a, mod=Q, psi=None, defect=None) -> list:
    """y[k] = a(psi^(2k+1)), k < N: the negacyclic transform of a, natural order.  defect "twiddle": the last (top) level of the
    DFT reads its neighbour's twiddle, index k ^ 1 for k."""
    n = len(a)
    psi = psi_q(n) if psi is None else psi
    tw = _powers(psi, n, mod)
    return _dft([x * t % mod for x, t in zip(a, tw)], _powers(psi * psi % mod, max(n // 2, 1), mod), 1, mod, defect == "twiddle")


def inverse(y, mod=Q, psi=None) -> list:
    n = len(y)
    psi_inv = pow(psi_q(n) if psi is None else psi, -1, mod)
    v = _dft(y, _powers(psi_inv * psi_inv % mod, max(n // 2, 1), mod), 1, mod)
    ninv = pow(n, -1, mod)
    return [x * t % mod * ninv % mod for x, t in zip(v, _powers(psi_inv, n, mod))]


# ---- products -------------------------------------------------------------------------------------------------------------
def ntt_mul(a, b, defect=None) -> list:
    """a * b mod (X^N + 1, q) through the plain transform (N a power of two)."""
    fa, fb = forward(a, defect=defect), forward(b, defect=defect)
    return inverse([x * y % Q for x, y in zip(fa, fb)])


def kron_mul(a, b) -> list:
    """a * b mod (X^N + 1, q) by Kronecker substitution: a coefficient of the integer product is below N q^2 < 2^(2 753 + log2 N),
    so slots of that many bits (rounded up to bytes, two to spare) never carry into each other."""
    n = len(a)
    nb = (2 * 753 + max(n - 1, 1).bit_length() + 2 + 7) // 8
    pack = lambda v: int.from_bytes(b"".join(x.to_bytes(nb, "little") for x in v), "little")
    raw = (pack(a) * pack(b)).to_bytes(2 * n * nb, "little")
    c = [int.from_bytes(raw[i * nb:(i + 1) * nb], "little") for i in range(2 * n)]
    return [(c[i] - c[i + n]) % Q for i in range(n)]


def ring_mul(a, b) -> list:
    n = len(a)
    assert len(b) == n
    if not transform_path(n):
        return O.encodedtext_mul(a, b)
    return kron_mul(a, b) if n <= 4096 else ntt_mul(a, b)


DEFECTS = ("twiddle", "c2_sign", "row")
# twiddle   forward(): the top level reads twiddle k ^ 1 (k_she_fwd_global loading psi[m + (i ^ 1)])
# c2_sign   ct_mul(): c2 = x1 y1, the negation dropped (k_she_inv_tile ignoring `negate`)
# row       batch_mul(): row i reads operand row i mod (batch - 1), a row index taken modulo the wrong length


def batch_mul(a_rows, b_rows, defect=None) -> list:
    """Row i of the result is a_rows[i] * b_rows[i]."""
    m = len(a_rows) - 1 if defect == "row" and len(a_rows) > 1 else len(a_rows)
    mul = ring_mul if defect is None else (lambda x, y: ntt_mul(x, y, defect))
    return [mul(a_rows[i % m], b_rows[i % m]) for i in range(len(a_rows))]


# ---- ciphertexts: (c0, c1, c2), the formulas of zkref.ciphertext_{mul, encrypt_from, decrypt} --------------------------------
# With mul=None the products of a transform size share their forward transforms (a ciphertext product is 4 forward and 3 inverse
# transforms, not 4 products = 12): at (2048, 3) that is the difference between a few seconds and half a minute of reference.
# test_she_model.py holds this form against the restatement over ring_mul (mul=ring_mul) and against the oracle.
def _pw(x, y):
    return [u * v % Q for u, v in zip(x, y)]


def ct_mul(x, y, mul=None, defect=None) -> tuple:
    """c0 = x0 y0, c1 = x0 y1 + x1 y0, c2 = (-x1) y1."""
    n = len(x[0])
    keep = defect == "c2_sign"
    if mul is None and not transform_path(n):
        mul = ring_mul
    if mul is not None:
        c1 = O.texts_add(mul(x[0], y[1]), mul(x[1], y[0]))
        return mul(x[0], y[0]), c1, mul(x[1] if keep else O.texts_neg(x[1]), y[1])
    fx0, fx1 = forward(x[0], defect=defect), forward(x[1], defect=defect)
    fy0, fy1 = (fx0, fx1) if y is x else (forward(y[0], defect=defect), forward(y[1], defect=defect))
    c2 = inverse(_pw(fx1, fy1))
    return inverse(_pw(fx0, fy0)), inverse(O.texts_add(_pw(fx0, fy1), _pw(fx1, fy0))), c2 if keep else O.texts_neg(c2)


def ct_encrypt(e, pk_a, pk_b, r, p=R, mul=None) -> tuple:
    """r = u | v | w:  c0 = b v + w p + e,  c1 = a v + u p,  c2 = 0."""
    n = len(e)
    u, v, w = r[:n], r[n:2 * n], r[2 * n:3 * n]
    if mul is None and not transform_path(n):
        mul = ring_mul
    if mul is not None:
        bv, av = mul(pk_b, v), mul(pk_a, v)
    else:
        fv = forward(v)
        bv, av = inverse(_pw(forward(pk_b), fv)), inverse(_pw(forward(pk_a), fv))
    return O.texts_add(O.texts_add(bv, O.encodedtext_scale(w, p)), e), O.texts_add(av, O.encodedtext_scale(u, p)), [0] * n


def ct_decrypt(ct, sk, mul=None) -> list:
    """c0 - s c1 - (s s) c2."""
    n = len(sk)
    if mul is None and not transform_path(n):
        mul = ring_mul
    if mul is not None:
        return O.texts_sub(O.texts_sub(ct[0], mul(sk, ct[1])), mul(mul(sk, sk), ct[2]))
    fs = forward(sk)
    t = _pw(fs, forward(ct[1]))
    if any(ct[2]):
        t = O.texts_add(t, _pw(_pw(fs, fs), forward(ct[2])))
    return O.texts_sub(ct[0], inverse(t))


# ---- encode / decode --------------------------------------------------------------------------------------------------------
def encode_fast(vals) -> list:
    """Plaintexts::encode: the polynomial over Fr with p(zeta^(2i+1)) = vals[i], its coefficients read as integers below q."""
    return inverse(vals, R, zeta_r(len(vals)))


def centred_lift(c: int) -> int:
    """Encodedtext::decode's lift of an Fq coefficient to Fr: c above q / 2 stands for c - q."""
    return (c - Q % R if c > Q // 2 else c) % R


def decode_fast(vals) -> list:
    return forward([centred_lift(c) for c in vals], R, zeta_r(len(vals)))


LIFT_ENDS = (0, 1, Q // 2 - 1, Q // 2, Q // 2 + 1, Q - 1, Q - Q % R, Q % R, R, R - 1)


# ---- operand families -------------------------------------------------------------------------------------------------------
DELTAS = ("delta_0", "delta_1", "delta_half", "delta_last")
FAMILIES = ("random", "all_q-1", "alt_q-1_1", "mask_0_q-1", "residue_top") + DELTAS


def uniform_q(rng: random.Random, n: int) -> list:
    return [rng.randrange(Q) for _ in range(n)]


def uniform_r(rng: random.Random, n: int) -> list:
    return [rng.randrange(R) for _ in range(n)]


def delta_index(name: str, n: int) -> int:
    return {"delta_0": 0, "delta_1": 1, "delta_half": n // 2, "delta_last": n - 1}[name]


def family(name: str, n: int, seed: int = 0) -> list:
    if name == "random":
        return uniform_q(random.Random(1000 * n + seed), n)
    if name == "all_q-1":
        return [Q - 1] * n
    if name == "alt_q-1_1":
        return [Q - 1 if i % 2 == 0 else 1 for i in range(n)]
    if name == "mask_0_q-1":
        rng = random.Random(2000 * n + seed)
        return [(Q - 1) * rng.randrange(2) for _ in range(n)]
    if name == "residue_top":
        return [RESIDUE_TOP] * n
    if name in DELTAS:
        out = [0] * n
        out[delta_index(name, n)] = 1
        return out
    raise KeyError(name)


def product_cases(n: int) -> list:
    """The (family of a, family of b) pairs test_gpu_she_exact.py multiplies at the transform size N."""
    cases = [("random", "random"), ("all_q-1", "all_q-1"), ("residue_top", "random")]
    if n >= 8192:
        return cases[:2]
    if n < 4096:
        cases += [("alt_q-1_1", "mask_0_q-1")] + [(d, "random") for d in DELTAS]
    return cases


def case_operands(case, n: int):
    return family(case[0], n, 1), family(case[1], n, 2)


# ---- closed forms that need no reference product ----------------------------------------------------------------------------
def all_top_squared(n: int) -> list:
    """(sum_i -X^i)^2 mod X^N + 1: coefficient k gets k + 1 products + 1 and N - 1 - k wrapped ones - 1."""
    return [(2 * k + 2 - n) % Q for k in range(n)]


def delta_times(k: int, a) -> list:
    """X^k a mod X^N + 1: a rotated by k, the wrapped coefficients negated."""
    n = len(a)
    return [(-x) % Q for x in a[n - k:]] + list(a[:n - k])


def closed_form(case, n: int, a, b):
    """The product of the pair from its definition, or None where there is none."""
    if case == ("all_q-1", "all_q-1"):
        return all_top_squared(n)
    if case[0] in DELTAS:
        return delta_times(delta_index(case[0], n), b)
    return None


# ---- device words -----------------------------------------------------------------------------------------------------------
def words(vals) -> np.ndarray:
    """Canonical integers -> (n, 12) uint64 Montgomery words, as the library reads them."""
    return cv.fq753_to_mont(vals)


def stored_ints(arr) -> list:
    """The integers the words spell, Montgomery factor left in (below q for a reduced element)."""
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 96], "little") for i in range(0, len(raw), 96)]


def all_below_q(arr) -> bool:
    return all(v < Q for v in stored_ints(arr))


def mismatch(got: np.ndarray, want: np.ndarray, n: int):
    """None when the two word arrays (rows * n, 12) are bit-equal; else where they differ: how many elements, and the row and
    coefficient of the first."""
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    if np.array_equal(got, want):
        return None
    bad = np.flatnonzero((got != want).any(axis=1))
    first = int(bad[0])
    return "%d of %d elements differ, first at row %d coefficient %d (rows hit: %s)" % (
        len(bad), got.shape[0], first // n, first % n, np.unique(bad // n)[:8].tolist())
