"""Inputs, closed forms, the launch plan and an index-level model of the device NTT, shared by test_gpu_ntt_exact.py (device
against the C oracle), test_oracle.py (the C oracle against closed forms) and test_ntt_model.py (would the comparison notice a
wrong kernel?).  Everything is a canonical residue vector: (N, 4) uint64, little-endian limbs of a value below r, read by the
library and the oracle as Montgomery forms (x R mod r, R = 2^256)."""
from itertools import accumulate, repeat

import numpy as np

import zkref as O

R = O.R_MOD
MONT = (1 << 256) % R                     # the residue of the field element 1
KINDS = ((0, 0), (1, 0), (0, 1), (1, 1))  # (inverse, coset)
KIND_NAME = {(0, 0): "fft", (1, 0): "ifft", (0, 1): "coset_fft", (1, 1): "coset_ifft"}
_RL = [(R >> (64 * k)) & (2**64 - 1) for k in range(4)]


def limbs(vals) -> np.ndarray:
    """ints below 2^256 -> (n, 4) uint64 (through bytes: a vector of 2^24 takes seconds, not minutes)."""
    buf = b"".join(v.to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(-1, 4).astype(np.uint64)


def ints(arr) -> list:
    raw = np.ascontiguousarray(arr, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def mont(x: int) -> int:
    return x % R * MONT % R


def below_r(a: np.ndarray) -> np.ndarray:
    lt = np.zeros(a.shape[0], dtype=bool)
    eq = np.ones(a.shape[0], dtype=bool)
    for k in (3, 2, 1, 0):
        lt |= eq & (a[:, k] < np.uint64(_RL[k]))
        eq &= a[:, k] == np.uint64(_RL[k])
    return lt


def uniform(rs: np.random.RandomState, n: int) -> np.ndarray:
    """Uniform below r: 253 random bits, redrawn where they are not below r."""
    a = np.frombuffer(rs.bytes(32 * n), dtype="<u8").reshape(n, 4).astype(np.uint64)
    a[:, 3] &= np.uint64((1 << 61) - 1)
    while True:
        bad = np.flatnonzero(~below_r(a))
        if not len(bad):
            return a
        b = np.frombuffer(rs.bytes(32 * len(bad)), dtype="<u8").reshape(-1, 4).astype(np.uint64)
        b[:, 3] &= np.uint64((1 << 61) - 1)
        a[bad] = b


def geometric(start: int, ratio: int, n: int) -> np.ndarray:
    """start * ratio^i mod r, i < n, as residues (python integers only: independent of the C oracle)."""
    return limbs(accumulate(repeat(ratio, n - 1), lambda x, q: x * q % R, initial=start % R))


def root(log_n: int) -> int:
    return O.Domain(1 << log_n).group_gen


def delta_index(log_n: int) -> int:
    """An index with many set bits: all of them but one."""
    n = 1 << log_n
    return n - 1 - (n >> 3 if log_n >= 3 else 0)


def geometric_m(log_n: int) -> int:
    """An odd exponent step near N / 3."""
    return ((1 << log_n) // 3) | 1


FAMILIES = ("random", "all_r-1", "mask_0_r-1", "alt_r-1_1", "delta", "geometric")


def family(name: str, log_n: int) -> np.ndarray:
    n = 1 << log_n
    top = limbs([R - 1])[0]
    if name == "random":
        return uniform(np.random.RandomState(1000 + log_n), n)
    if name == "all_r-1":
        return np.tile(top, (n, 1))
    if name == "mask_0_r-1":
        out = np.zeros((n, 4), dtype=np.uint64)
        out[np.random.RandomState(2000 + log_n).rand(n) < 0.5] = top
        return out
    if name == "alt_r-1_1":
        out = np.tile(top, (n, 1))
        out[1::2] = limbs([1])[0]
        return out
    if name == "delta":
        out = np.zeros((n, 4), dtype=np.uint64)
        out[delta_index(log_n)] = limbs([MONT])[0]
        return out
    if name == "geometric":
        return geometric(MONT, pow(root(log_n), geometric_m(log_n), R), n)
    raise KeyError(name)


def closed_form_mismatch(name: str, log_n: int, inverse: int, coset: int, out: np.ndarray):
    """`out` against the transform of the delta (at j) or geometric (w^(m i)) family from its definition, python integers only;
    None when it holds, as mismatch().  With g the coset generator and F[k] = sum_i v[i] w^(ik):
      delta:      fft w^(jk);  ifft w^(-jk) / N;  coset fft g^j w^(jk);  coset ifft (g^-1 w^-j)^k / N -- geometric columns;
      geometric:  fft N at k = -m;  ifft 1 at k = m;  coset ifft g^-m at k = m;  zero elsewhere;
                  coset fft sum_i (g w^(m+k))^i = (g^N - 1) / (g w^(m+k) - 1), checked as F[k] (g w^(m+k) - 1) == g^N - 1."""
    n = 1 << log_n
    w, g = root(log_n), O.FR_GENERATOR
    wi, gi, ninv = pow(w, -1, R), pow(g, -1, R), pow(n, -1, R)
    if name == "delta":
        j = delta_index(log_n)
        start = (1, ninv, pow(g, j, R), ninv)[inverse + 2 * coset]
        ratio = (pow(w, j, R), pow(wi, j, R), pow(w, j, R), gi * pow(wi, j, R) % R)[inverse + 2 * coset]
        return mismatch(out, geometric(mont(start), ratio, n))
    assert name == "geometric"
    m = geometric_m(log_n)
    if (inverse, coset) == (0, 1):
        rhs = mont(pow(g, n, R) - 1)
        fac = accumulate(repeat(w, n - 1), lambda x, q: x * q % R, initial=g * pow(w, m, R) % R)
        bad = [k for k, (f, x) in enumerate(zip(ints(out), fac)) if f >= R or f * (x - 1) % R != rhs]
        return "%d of %d elements miss the closed form, first at %s" % (len(bad), n, bad[:8]) if bad else None
    want = np.zeros((n, 4), dtype=np.uint64)
    if inverse:
        want[m % n] = limbs([mont(pow(gi, m, R) if coset else 1)])[0]
    else:
        want[(n - m) % n] = limbs([mont(n)])[0]
    return mismatch(out, want)


def delta_forward_at(log_n: int, ks) -> np.ndarray:
    """The forward transform of the delta family at the positions ks alone: w^(j k), one pow each."""
    w, j = root(log_n), delta_index(log_n)
    return limbs(mont(pow(w, j * int(k), R)) for k in ks)


def mismatch(got: np.ndarray, want: np.ndarray):
    """None when the two vectors are bit-equal; else a description of where they differ (count, first indices).  The one
    comparator of every exact NTT test."""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return "shape %s != %s" % (got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    return "%d of %d elements differ, first at %s" % (len(bad), got.shape[0], bad[:8].tolist())


# ---- the launch plan, as ntt_run (csrc/ntt.hip) derives it ----------------------------------------------------------------
def plan(log_n: int) -> dict:
    """passes, logM per pass, logE (tile = 2^logE elements, C = 2^(logE - logM) columns) and tiles per pass."""
    if log_n == 0:
        return {"passes": 0, "logM": [], "logE": 0, "tiles": 0}
    passes = (log_n + 9) // 10
    base, extra = divmod(log_n, passes)
    log_e = (log_n - 8 if log_n > 8 else 0) if log_n < 20 else (10 if passes >= 3 else 12)
    log_e = max(log_e, base + (1 if extra else 0))
    if passes == 1:
        log_e = log_n
    return {"passes": passes, "logM": [base + (1 if p < extra else 0) for p in range(passes)], "logE": log_e,
            "tiles": 1 << (log_n - log_e)}


# ---- an index-level model of the device schedule --------------------------------------------------------------------------
def _brev(x: int, bits: int) -> int:
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


DEFECTS = ("twiddle", "eb", "post")


def model_ntt(v, log_n: int, inverse: int, coset: int, defect: str = None) -> list:
    """The device transform restated on python integers (canonical field elements in, canonical out): the same passes, columns,
    radix-2 / radix-4 stages, twiddle exponents, inter-pass twiddles and bit-reversed scatter with its post-scale as k_ntt_pass,
    without the lazy ranges.  `defect` plants one single-line mistake:
      "twiddle": the inter-pass twiddle of one (l, q) pair of the first pass has exponent + 1;
      "eb":      the inverse transform does not negate eb (the twiddle of x1 - x3);
      "post":    the coset inverse's post-scale table is read at idx, not at dst (the bit-reversed position)."""
    n = 1 << log_n
    n1 = n - 1
    w = root(log_n)
    tw = list(accumulate(repeat(w, n - 1), lambda x, q: x * q % R, initial=1))
    g = O.FR_GENERATOR
    data = [x % R for x in v]
    if coset and not inverse:
        data = [x * s % R for x, s in zip(data, accumulate(repeat(g, n - 1), lambda x, q: x * q % R, initial=1))]
    post = None
    if inverse:
        ninv = pow(n, -1, R)
        gi = pow(g, -1, R) if coset else 1
        post = list(accumulate(repeat(gi, n - 1), lambda x, q: x * q % R, initial=ninv))
    neg = (lambda e: (-e) & n1) if inverse else (lambda e: e)
    pl = plan(log_n)
    remaining = log_n
    for p, log_m in enumerate(pl["logM"]):
        log_s = remaining - log_m
        log_b = log_s + log_m
        m_sz, s_mask, tsh = 1 << log_m, (1 << log_s) - 1, log_n - log_m
        out = [0] * n
        for col in range(n >> log_m):
            base = ((col >> log_s) << log_b) + (col & s_mask)
            x = [data[base + (m << log_s)] for m in range(m_sz)]
            s = 0
            if log_m & 1:
                half = m_sz >> 1
                for j in range(half):
                    a, b = x[j], x[j + half]
                    x[j], x[j + half] = (a + b) % R, (a - b) * tw[neg(j << tsh)] % R
                s = 1
            while s < log_m:
                lg_a = log_m - 1 - s
                lg_b = lg_a - 1
                gb = 1 << lg_b
                for j in range(m_sz >> 2):
                    jj = j & (gb - 1)
                    m0 = ((j >> lg_b) << (lg_a + 1)) | jj
                    ea = (jj << s) << tsh
                    eb, ec = ea + (n >> 2), ea << 1
                    eb = eb if (defect == "eb" and inverse) else neg(eb)
                    ea, ec = neg(ea), neg(ec)
                    x0, x1, x2, x3 = x[m0], x[m0 + gb], x[m0 + 2 * gb], x[m0 + 3 * gb]
                    s0, d0 = x0 + x2, (x0 - x2) * tw[ea] % R
                    s1, d1 = x1 + x3, (x1 - x3) * tw[eb & n1] % R
                    x[m0], x[m0 + 2 * gb] = (s0 + s1) % R, (d0 + d1) % R
                    x[m0 + gb], x[m0 + 3 * gb] = (s0 - s1) * tw[ec] % R, (d0 - d1) * tw[ec] % R
                s += 2
            for m in range(m_sz):
                idx = base + (m << log_s)
                val = x[m]
                if log_s:
                    l, q = col & s_mask, _brev(m, log_m)
                    ex = (l * q) << (log_n - log_b)
                    if defect == "twiddle" and p == 0 and l == s_mask and q == m_sz - 1:
                        ex += 1
                    out[idx] = val * tw[neg(ex & n1)] % R
                else:
                    dst = _brev(idx, log_n)
                    if post is not None:
                        val = val * post[idx if (defect == "post" and coset) else dst] % R
                    out[dst] = val
        data = out
        remaining = log_s
    if log_n == 0 and post is not None:
        data = [data[0] * post[0] % R]
    return data


def model_residues(v: np.ndarray, log_n: int, inverse: int, coset: int, defect: str = None) -> np.ndarray:
    """model_ntt on a residue vector: the transform is linear, so the Montgomery factor R rides through it unchanged."""
    return limbs(model_ntt(ints(v), log_n, inverse, coset, defect))
