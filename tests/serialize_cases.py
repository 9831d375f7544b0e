"""Point bytes with their expected reading, for the (de)serialization tests (host and device), and the rule as a model.

Everything here is computed on the CPU from the oracle (zkref.py) in Python integers, seeded, once per session.  Nothing reads the
library.  A point is None (infinity) or an affine pair; G2 coordinates are pairs (c0, c1) of Fq2 = Fq[u]/(u^2 + 5).

THE RULE (include/zkmpc_hip.h states it next to zk_bases_deserialize_compressed; `classify` is the same rule in integers):
 1. every base-field element on the wire is below q, whatever the flags say                                       -> noncanonical
 2. flag bits exist only in the last byte of the last element: bit 7 of any other element's last byte is zero     -> flags
    (its bit 6 already makes the value at least q                                                                 -> noncanonical)
 3. both flags at once (0xC0)                                                                                      -> flags
 4. the infinity flag stands over exactly what the serializer writes: x = 0 compressed, (0, 1) uncompressed, else -> flags
 5. uncompressed: the sign flag is refused (flags); (x, y) satisfies the curve equation, else                      -> curve
 6. compressed: x^3 + b is a square, else curve; y is the root whose "greater than its negative" bit equals the sign flag (y = 0
    has the bit 0 and, as in the reference's get_point_from_x, comes out under either flag)
A string that breaks several rules has the class of the first in the order noncanonical, flags, curve.
"""
import functools
import random
from types import SimpleNamespace

import zkref as O
import subgroup_cases as sc

Q = O.Q_MOD
STATUS = {"ok": 0, "noncanonical": 1, "flags": 2, "curve": 3}       # the numbering of ZK_POINT_*
B2 = O.G2_COEFF_B
INV2 = pow(2, -1, Q)
TS_T = (Q - 1) >> 46
assert TS_T & 1 and TS_T << 46 == Q - 1


# ---- field helpers ------------------------------------------------------------------------------------------------------------
def legendre(a):
    a %= Q
    return 0 if a == 0 else (1 if pow(a, (Q - 1) // 2, Q) == 1 else -1)


def fq2_sqrt(a):
    return sc.fq2_sqrt(a)


def rhs(group, x):
    if group == 1:
        return (x * x % Q * x + 1) % Q
    return O.fq2_add(O.fq2_mul(O.fq2_sqr(x), x), B2)


def gt_neg(group, y):
    return O._fq_gt_neg(y) if group == 1 else O._fq2_gt_neg(y)


def neg(group, y):
    return (Q - y) % Q if group == 1 else O.fq2_neg(y)


def on_curve(group, P):
    return O.ec_is_on_curve(P, O.FqOps if group == 1 else O.Fq2Ops)


def ts_order_log2(a):
    """k with a^t of order 2^k, q - 1 = 2^46 t: how many squarings the first pass of Tonelli-Shanks makes (46: a non-residue);
    None for a = 0, which leaves before any of it."""
    if a % Q == 0:
        return None
    b, k = pow(a % Q, TS_T, Q), 0
    while b != 1:
        b, k = b * b % Q, k + 1
    return k


def fq2_sqrt_exit(a):
    """Which of the four exits of serialize.hip::fq2_sqrt the value a takes, decided in integers.  The root alpha of the norm that
    the oracle finds may be the negative of the device's, and delta(-alpha) = delta(alpha) - alpha: exactly one of the pair is a
    residue (their product is -5 a1^2 / 4, a non-residue), so `delta_qr` / `delta_nqr` name the residuosity of the ORACLE's delta;
    the device leaves at its first try for one of the two patterns and through the fallback for the other."""
    a0, a1 = a[0] % Q, a[1] % Q
    if a1 == 0:
        return "c1zero_qr" if legendre(a0) >= 0 else "c1zero_nqr"
    alpha = O.fq_sqrt((a0 * a0 + 5 * a1 * a1) % Q)
    if alpha is None:
        return "norm_nqr"
    d1, d2 = (alpha + a0) * INV2 % Q, (a0 - alpha) * INV2 % Q
    assert legendre(d1) * legendre(d2) == -1
    return "delta_qr" if legendre(d1) == 1 else "delta_nqr"


# ---- bytes --------------------------------------------------------------------------------------------------------------------
def elements(group, compressed):
    """names of the 48-byte elements of one point, in wire order"""
    co = ["x"] if group == 1 else ["x.c0", "x.c1"]
    if not compressed:
        co += ["y"] if group == 1 else ["y.c0", "y.c1"]
    return co


def point_size(group, compressed):
    return 48 * len(elements(group, compressed))


def serialize(group, compressed, P):
    f = {(1, True): O.g1_serialize, (1, False): O.g1_serialize_uncompressed,
         (2, True): O.g2_serialize, (2, False): O.g2_serialize_uncompressed}[(group, bool(compressed))]
    return f(P)


def raw_bytes(values, flags=0):
    """elements given as integers below 2^384, flags OR-ed into the last byte"""
    b = bytearray(b"".join(int(v).to_bytes(48, "little") for v in values))
    b[-1] |= flags
    return bytes(b)


def classify(group, compressed, data):
    """("ok", point_or_None) | ("noncanonical",) | ("flags",) | ("curve",) by the rule above, in Python integers."""
    return _classify(group, bool(compressed), bytes(data))


@functools.lru_cache(maxsize=None)
def _classify(group, compressed, data):
    ne = len(elements(group, compressed))
    assert len(data) == 48 * ne
    els = [data[48 * i:48 * i + 48] for i in range(ne)]
    flags = els[-1][47] & 0xC0
    vals = [int.from_bytes(e, "little") & ((1 << 383) - 1) for e in els[:-1]] + [int.from_bytes(els[-1], "little") & ((1 << 382) - 1)]
    if any(v >= Q for v in vals):
        return ("noncanonical",)
    if any(e[47] & 0x80 for e in els[:-1]) or flags == 0xC0:
        return ("flags",)
    half = ne // 2 if not compressed else ne
    x = vals[0] if group == 1 else (vals[0], vals[1])
    zero, one = (0, 1) if group == 1 else ((0, 0), (1, 0))
    if compressed:
        if flags & 0x40:
            return ("ok", None) if x == zero else ("flags",)
        y = O.fq_sqrt(rhs(1, x)) if group == 1 else fq2_sqrt(rhs(2, x))
        if y is None:
            return ("curve",)
        if gt_neg(group, y) != bool(flags & 0x80):
            y = neg(group, y)
        return ("ok", (x, y))
    y = vals[half] if group == 1 else (vals[half], vals[half + 1])
    if flags & 0x80:
        return ("flags",)
    if flags & 0x40:
        return ("ok", None) if (x, y) == (zero, one) else ("flags",)
    return ("ok", (x, y)) if on_curve(group, (x, y)) else ("curve",)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _case(kind, name, data, expect, canonical=False, subgroup=None):
    """canonical: the bytes are what the serializer writes for the point (so they round-trip); subgroup: the oracle's r P == O"""
    return SimpleNamespace(kind=kind, name=name, data=data, expect=expect, canonical=canonical, subgroup=subgroup)


@functools.lru_cache(maxsize=None)
def subgroup_points(group):
    """512 (G1) / 256 (G2) subgroup points as a running sum P += G from a seeded start, each followed by its negative."""
    rng = O.Prng(0x5E71A1 + group)
    gen, add, mul = (O.G1_GEN, O.g1_add, O.g1_mul) if group == 1 else (O.G2_GEN, O.g2_add, O.g2_mul)
    P = mul(gen, rng.fr())
    out = []
    for _ in range(512 if group == 1 else 256):
        out += [P, (P[0], neg(group, P[1]))]
        P = add(P, gen)
    return out


@functools.lru_cache(maxsize=None)
def g2_c1_zero_abscissae():
    """16 abscissae x = (x0, x1) of the twist with (x^3 + b).c1 = 0: 8 whose c0 is a residue (y = (s, 0)) and 8 whose c0 is not
    (y = (0, s)).  x1 = 1, 2, ...; 3 x0^2 x1 - 5 x1^3 + b1 = 0 gives x0^2 = (5 x1^3 - b1) / (3 x1)."""
    got = {1: [], -1: []}
    x1 = 0
    while min(len(v) for v in got.values()) < 8:
        x1 += 1
        x0 = O.fq_sqrt((5 * x1 ** 3 - B2[1]) * pow(3 * x1, -1, Q) % Q)
        if x0 is None:
            continue
        r = rhs(2, (x0, x1))
        assert r[1] == 0 and r[0] == (x0 ** 3 - 15 * x0 * x1 * x1) % Q and r[0] != 0
        if len(got[legendre(r[0])]) < 8:
            got[legendre(r[0])].append((x0, x1))
    return got[1] + got[-1]


def _fq2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = O.fq2_mul(r, a)
        a, e = O.fq2_sqr(a), e >> 1
    return r


@functools.lru_cache(maxsize=None)
def g2_half_points():
    """Points of the twist whose y.c1 is (q - 1) / 2, the largest value that is NOT greater than its negative, each with its
    negative (y.c1 = (q + 1) / 2): the boundary of the sign bit, reachable by decompression.  y = (y0, (q - 1) / 2) for
    y0 = 0, 1, ... until x^3 = y^2 - b has a root; 9 does not divide q^2 - 1, so a cube t has the root t^(1/3 mod (q^2 - 1)/3).
    (G1 has no such point: -3/4 is no cube in Fq.)"""
    h = (Q - 1) // 2
    m = (Q * Q - 1) // 3
    assert m % 3 and pow(-3 * pow(4, -1, Q) % Q, (Q - 1) // 3, Q) != 1
    out, y0 = [], 0
    while len(out) < 4:
        y = (y0, h)
        t = O.fq2_sub(O.fq2_sqr(y), B2)
        x = _fq2_pow(t, pow(3, -1, m))
        if O.fq2_mul(O.fq2_sqr(x), x) == t:
            assert on_curve(2, (x, y))
            out += [(x, y), (x, O.fq2_neg(y))]
        y0 += 1
    return out


@functools.lru_cache(maxsize=None)
def non_square_abscissae(group):
    """64 abscissae with x^3 + b a non-square: a subgroup point's x plus 1, 2, ... until it is one (G2: added to c0)."""
    out = []
    for P in subgroup_points(group)[::2][:64]:
        d = 1
        while True:
            x = (P[0] + d) % Q if group == 1 else ((P[0][0] + d) % Q, P[0][1])
            r = rhs(group, x)
            if legendre(r) == -1 if group == 1 else fq2_sqrt_exit(r) == "norm_nqr":
                out.append(x)
                break
            d += 1
    return out


def _flat(group, P):
    """a point's coordinates as the integers of its uncompressed elements"""
    return [P[0], P[1]] if group == 1 else [P[0][0], P[0][1], P[1][0], P[1][1]]


@functools.lru_cache(maxsize=None)
def point_cases(group, compressed):
    """The accepted points and the abscissae off the curve."""
    ops = O.FqOps if group == 1 else O.Fq2Ops
    out = []
    ser = lambda P: serialize(group, compressed, P)
    pts = subgroup_points(group)
    mid = len(pts) // 2
    out.append(_case("infinity", "infinity first", ser(None), ("ok", None), True, True))
    for i, P in enumerate(pts):
        if i == mid:
            out.append(_case("infinity", "infinity middle", ser(None), ("ok", None), True, True))
        out.append(_case("subgroup", "subgroup %d" % i, ser(P), ("ok", P), True, True))
    if group == 1:
        for P in ((0, 1), (0, Q - 1), (Q - 1, 0)):
            out.append(_case("special", "special %r" % (P,) if P[0] == 0 else "special (q-1, 0)", ser(P), ("ok", P), True, False))
        if compressed:       # y = 0 under the sign flag: the reference's get_point_from_x gives (x, 0) again; not the serializer's bytes
            out.append(_case("y0_sign", "(q-1, 0) with the sign flag", raw_bytes([Q - 1], 0x80), ("ok", (Q - 1, 0)), False, False))
    else:
        for x in g2_c1_zero_abscissae():
            y = fq2_sqrt(rhs(2, x))
            assert y is not None and 0 in y
            for yy in (y, O.fq2_neg(y)):
                P = (x, yy)
                assert on_curve(2, P)
                out.append(_case("c1zero", "rhs.c1 = 0, x1 = %d, y = %s" % (x[1], "(s, 0)" if yy[1] == 0 else "(0, s)"), ser(P), ("ok", P), True,
                                 sc.oracle_in_subgroup(P, ops)))
        for P in g2_half_points():
            out.append(_case("half", "y.c1 = (q %s 1) / 2" % ("-" if P[1][1] < Q // 2 + 1 else "+"), ser(P), ("ok", P), True,
                             sc.oracle_in_subgroup(P, ops)))
    for P, inside in sc.cases(group):
        if P is not None:
            out.append(_case("subgroup_cases", "subgroup_cases point", ser(P), ("ok", P), True, bool(inside)))
    for k, x in enumerate(non_square_abscissae(group)):
        xs = [x] if group == 1 else list(x)
        if compressed:
            for fl in (0, 0x80) if k < 4 else (0x80 * (k & 1),):
                out.append(_case("curve", "non-square %d flag %#x" % (k, fl), raw_bytes(xs, fl), ("curve",)))
        else:
            ys = [1 + k] if group == 1 else [k, 1 + k]
            out.append(_case("curve", "non-square %d" % k, raw_bytes(xs + ys), ("curve",)))
    if not compressed:       # x on the curve with another point's y, and a good point with one bit of y changed
        a, b = pts[0], pts[2]
        out.append(_case("curve", "x of one point, y of another", raw_bytes(_flat(group, (a[0], b[1]))), ("curve",)))
        fl = _flat(group, a)
        fl[-1] ^= 1
        out.append(_case("curve", "one bit of y changed", raw_bytes(fl), ("curve",)))
    out.append(_case("infinity", "infinity last", ser(None), ("ok", None), True, True))
    return out


VALUE_KINDS = ("=q", "=q+1", "=q+x", "=x+2^377", "|bit381", "=all382")


def _value_mutations(v):
    return (("=q", Q), ("=q+1", Q + 1), ("=q+x", Q + v), ("=x+2^377", v + (1 << 377)), ("|bit381", v | (1 << 381)), ("=all382", (1 << 382) - 1))


def malformed_kinds(group, compressed):
    """every kind of malformed string that malformed_cases(group, compressed) must hold"""
    els = elements(group, compressed)
    kinds = [e + k for e in els for k in VALUE_KINDS]
    kinds += ["0xC0 over a point", "0xC0 over zeros", "0x40 over x >= q"]
    kinds += [e + " bit 7" for e in els[:-1]] + [e + " bit 6" for e in els[:-1]]
    if compressed:
        kinds += ["0x40 over a valid x"]
    else:
        kinds += ["0x40 over (0, 0)", "0x40 over (0, 2)", "0x40 over a point", "0x40 over (0, 1)", "0x80 over a point"]
    return kinds


@functools.lru_cache(maxsize=None)
def malformed_cases(group, compressed):
    """Four base points (two with the sign flag, two without), every kind of malformed_kinds on each."""
    pts = subgroup_points(group)
    bases = [pts[0], pts[1], pts[6], pts[9]]
    assert {gt_neg(group, P[1]) for P in bases} == {True, False}
    els = elements(group, compressed)
    out = []
    add = lambda kind, vals, flags, cls, n: out.append(_case(kind, "%s, base %d" % (kind, n), raw_bytes(vals, flags), (cls,) if cls != "ok" else ("ok", None)))
    zero_xy = [0] * len(els)
    for n, P in enumerate(bases):
        vals = _flat(group, P)[:len(els)]
        sign = 0x80 if compressed and gt_neg(group, P[1]) else 0
        for i, e in enumerate(els):
            for k, v in _value_mutations(vals[i]):
                add(e + k, vals[:i] + [v] + vals[i + 1:], sign, "noncanonical", n)
            if i < len(els) - 1:
                add(e + " bit 7", vals[:i] + [vals[i] | 1 << 383] + vals[i + 1:], sign, "flags", n)
                add(e + " bit 6", vals[:i] + [vals[i] | 1 << 382] + vals[i + 1:], sign, "noncanonical", n)
        add("0xC0 over a point", vals, 0xC0, "flags", n)
        add("0xC0 over zeros", zero_xy, 0xC0, "flags", n)
        add("0x40 over x >= q", vals[:-1] + [Q + n] if compressed else [Q + n] + vals[1:], 0x40, "noncanonical", n)
        if compressed:
            add("0x40 over a valid x", vals, 0x40, "flags", n)
        else:
            h = len(els) // 2
            y_is = lambda c: zero_xy[:h] + [c] + zero_xy[h + 1:]
            add("0x40 over (0, 0)", zero_xy, 0x40, "flags", n)
            add("0x40 over (0, 2)", y_is(2), 0x40, "flags", n)
            add("0x40 over a point", vals, 0x40, "flags", n)
            add("0x40 over (0, 1)", y_is(1), 0x40, "ok", n)
            add("0x80 over a point", vals, 0x80, "flags", n)
    assert {c.kind for c in out} == set(malformed_kinds(group, compressed))
    return out


@functools.lru_cache(maxsize=None)
def cases(group, compressed):
    return point_cases(group, compressed) + malformed_cases(group, compressed)


@functools.lru_cache(maxsize=None)
def accepted(group, compressed):
    """the cases whose bytes the serializer writes: ([points], bytes, [in subgroup])"""
    cs = [c for c in cases(group, compressed) if c.canonical]
    return [c.expect[1] for c in cs], b"".join(c.data for c in cs), [c.subgroup for c in cs]


def one_bad_per_kind(group, compressed):
    """one refused case of every malformed kind and of `curve`: [(kind, class, bytes)]"""
    seen, out = set(), []
    for c in cases(group, compressed):
        if c.expect[0] != "ok" and c.kind not in seen:
            seen.add(c.kind)
            out.append((c.kind, c.expect[0], c.data))
    return out


# ---- proofs -------------------------------------------------------------------------------------------------------------------
def _add_to_element(proof, offset, delta):
    """the 48-byte element at `offset` of the proof with delta added to its low 382 bits, flag bits kept"""
    b = bytearray(proof)
    v = int.from_bytes(b[offset:offset + 48], "little")
    fl, v = v >> 382, v & ((1 << 382) - 1)
    assert v + delta < 1 << 382
    b[offset:offset + 48] = ((v + delta) | fl << 382).to_bytes(48, "little")
    return bytes(b)


def altered_proofs(proof):
    """{name: bytes}: the proof (A 48 | B 96 | C 48 bytes) read as the same three points by a decoder that drops what the rule asks
    for -- A.x + q, B.x.c0 + 2^377, C under both flags."""
    c = bytearray(proof)
    c[191] |= 0xC0
    return {"A.x + q": _add_to_element(proof, 0, Q), "B.c0 + 2^377": _add_to_element(proof, 48, 1 << 377), "C flags 0xC0": bytes(c)}
