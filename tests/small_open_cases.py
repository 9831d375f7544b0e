"""Cases for tests/test_small_open_host.py: one small open of the collaborative provers (csrc/sharednet.hpp) played on the host by
zk_diag_small_open_host.  A message is nf scalars, n1 G1 and n2 G2 points in the ABI's (= the wire's) form: 4 / 18 / 36 words per
item, `fr | g1 | g2`.  Every value, every encoding and every expected sum here comes from the oracle's field and group law
(oracle/zkref.py); nothing reads the library but `play`.
"""
import ctypes as C
import functools
import itertools

import numpy as np

import zkref as O
from marlin_verify_cases import cofactor_torsion_point
from subgroup_cases import g2_cofactor_torsion_point, oracle_in_subgroup

ZK_OK, ZK_ERR_ARG, ZK_ERR_STATE, ZK_ERR_MAC = 0, -2, -4, -5
Q, R = O.Q_MOD, O.R_MOD
OPS = {1: O.FqOps, 2: O.Fq2Ops}
COUNTS = [(2, 3, 1),      # the Groth16 fused open
          (0, 1, 0),      # the reveal of C
          (2, 0, 0), (0, 2, 0), (0, 0, 1)]


def words(nf, n1, n2):
    return 4 * nf + 18 * n1 + 36 * n2


# ---- the wire form, from the oracle's Montgomery constants --------------------------------------------------------------------------
def _w(v, n):
    assert 0 <= v < 1 << (64 * n)
    return [(v >> (64 * i)) & (2 ** 64 - 1) for i in range(n)]


def fr_words(v):
    return _w(O.fr_to_mont(v), 4)


def _fq(group, c):
    """one coordinate: an Fq (G1) or an Fq2 pair (G2) -> Montgomery words"""
    return _w(O.fq_to_mont(c), 6) if group == 1 else _w(O.fq_to_mont(c[0]), 6) + _w(O.fq_to_mont(c[1]), 6)


def _one(group):
    return 1 if group == 1 else (1, 0)


def _zero(group):
    return 0 if group == 1 else (0, 0)


def jacobian_words(group, x, y, z):
    return _fq(group, x) + _fq(group, y) + _fq(group, z)


def point_words(group, P):
    """the normalised form a party writes: Z = 1, infinity = (1, 1, 0)"""
    if P is None:
        return jacobian_words(group, _one(group), _one(group), _zero(group))
    return jacobian_words(group, P[0], P[1], _one(group))


def message_words(items):
    """items = (scalars, G1 points, G2 points)"""
    fr, g1, g2 = items
    return [w for v in fr for w in fr_words(v)] + [w for P in g1 for w in point_words(1, P)] + [w for P in g2 for w in point_words(2, P)]


# ---- values ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pool(group):
    """a few multiples of the generator (the oracle's scalar multiplication is slow: the cases draw from these)"""
    rng = O.Prng(0x5a11 + group)
    gen = O.G1_GEN if group == 1 else O.G2_GEN
    return [O.ec_mul(gen, rng.fr(), OPS[group]) for _ in range(7)]


def _sum_points(group, pts):
    acc = None
    for P in pts:
        acc = O.ec_add(acc, P, OPS[group])
    return acc


# How the parties' shares of ONE point item relate; each names what the sum has to get right.
PATTERNS = ["random",
            "share_at_infinity",          # party 0 holds infinity
            "sum_is_infinity",            # the shares cancel over all parties
            "equal",                      # every party holds the same point: P + P
            "opposite"]                   # the first two parties hold P and -P: P + (-P) inside the sum


def point_shares(group, pattern, parties, k):
    F, pts = OPS[group], pool(group)
    sh = [pts[(k + 2 * p) % len(pts)] for p in range(parties)]
    if pattern == "share_at_infinity":
        sh[0] = None
    elif pattern == "sum_is_infinity":
        sh[-1] = O.ec_neg(_sum_points(group, sh[:-1]), F)
    elif pattern == "equal":
        sh = [sh[0]] * parties
    elif pattern == "opposite" and parties >= 2:
        sh[1] = O.ec_neg(sh[0], F)
    return sh


def resharing(group, total, parties, k):
    """another additive sharing of the same total: the MAC lane under the key alpha = 1"""
    if group == 0:
        rng = O.Prng(0x3ac + k)
        sh = [rng.fr() for _ in range(parties - 1)]
        return sh + [(total - sum(sh)) % R]
    pts = pool(group)
    sh = [pts[(k + 3 * p + 1) % len(pts)] for p in range(parties - 1)]
    return sh + [O.ec_add(total, O.ec_neg(_sum_points(group, sh), OPS[group]), OPS[group])]


class Case:
    """shares[lane][party] = (scalars, G1 points, G2 points); opened = the oracle's sums; inject = [(lane, party, word offset, raw
    words)] written over the encoded messages; verdict = what every party that validates the injected slot must say."""

    def __init__(self, name, parties, lanes, counts, shares, opened, verdict=ZK_OK, inject=(), patterns=(), subgroup=None, note=None):
        self.name, self.parties, self.lanes, self.counts, self.shares, self.opened = name, parties, lanes, counts, shares, opened
        self.verdict, self.inject, self.patterns, self.note = verdict, list(inject), tuple(patterns), note
        self.subgroup = (lanes == 2) if subgroup is None else subgroup

    def __repr__(self):
        return self.name

    def share_words(self):
        out = np.array([[message_words(self.shares[l][p]) for p in range(self.parties)] for l in range(self.lanes)], dtype=np.uint64)
        for lane, party, off, raw in self.inject:
            out[lane, party, off:off + len(raw)] = np.array(raw, dtype=np.uint64)
        return out

    def opened_words(self):
        return np.array(message_words(self.opened), dtype=np.uint64)


def honest(parties, lanes, counts, salt=0):
    nf, n1, n2 = counts
    rng = O.Prng(0x09e4 + 97 * parties + 13 * lanes + salt + 1000 * words(*counts))
    fr = [[rng.fr() for _ in range(nf)] for _ in range(parties)]
    pat = [[PATTERNS[(salt + j + g) % len(PATTERNS)] for j in range(n)] for g, n in ((1, n1), (2, n2))]
    cols = [[point_shares(g, pat[g - 1][j], parties, salt + 3 * j) for j in range(n)] for g, n in ((1, n1), (2, n2))]
    lane0 = [(fr[p], [c[p] for c in cols[0]], [c[p] for c in cols[1]]) for p in range(parties)]
    opened = ([sum(f[i] for f in fr) % R for i in range(nf)], [_sum_points(1, c) for c in cols[0]], [_sum_points(2, c) for c in cols[1]])
    shares = [lane0]
    if lanes == 2:
        mf = [resharing(0, v, parties, salt + i) for i, v in enumerate(opened[0])]
        m1 = [resharing(1, v, parties, salt + i) for i, v in enumerate(opened[1])]
        m2 = [resharing(2, v, parties, salt + i) for i, v in enumerate(opened[2])]
        shares.append([([c[p] for c in mf], [c[p] for c in m1], [c[p] for c in m2]) for p in range(parties)])
    name = "sum-P%d-lanes%d-%d.%d.%d-salt%d" % ((parties, lanes) + tuple(counts) + (salt,))
    return Case(name, parties, lanes, counts, shares, opened, patterns=pat[0] + pat[1])


@functools.lru_cache(maxsize=None)
def sum_cases():
    # every party count, lane count and shape; the salts walk every pattern over the G1 items and over the G2 item
    out = [honest(P, lanes, counts, salt) for P, lanes, counts in itertools.product((1, 2, 3), (1, 2), COUNTS) for salt in (0, 2)]
    out += [honest(2, 1, (0, 2, 0), salt) for salt in (1, 3, 4)] + [honest(P, 2, (0, 0, 1), salt) for P in (2, 3) for salt in (1, 3, 4)]
    for g in (1, 2):                                        # every pattern meets a G1 item and a G2 item, among 2 and among 3 parties
        seen = {(c.parties, p) for c in out for p in (c.patterns[:c.counts[1]] if g == 1 else c.patterns[c.counts[1]:])}
        for pattern in PATTERNS:
            assert (2, pattern) in seen and (3, pattern) in seen, (g, pattern)
    for P, lanes, counts in itertools.product((1, 2, 3), (1, 2), COUNTS):
        assert any((c.parties, c.lanes, c.counts) == (P, lanes, counts) for c in out)
    # the oracle's own view of the patterns
    for c in out:
        col = lambda g, j: [c.shares[0][p][g][j] for p in range(c.parties)]
        items = [(1, j) for j in range(c.counts[1])] + [(2, j) for j in range(c.counts[2])]
        for (g, j), pattern in zip(items, c.patterns):
            if pattern == "share_at_infinity":
                assert col(g, j)[0] is None
            if pattern == "sum_is_infinity":
                assert c.opened[g][j] is None and (c.parties == 1 or col(g, j)[0] is not None)
            if pattern == "equal" and c.parties == 2:
                assert col(g, j)[0] == col(g, j)[1] and c.opened[g][j] == O.ec_add(col(g, j)[0], col(g, j)[0], OPS[g])
            if pattern == "opposite" and c.parties == 2:
                assert col(g, j)[1] == O.ec_neg(col(g, j)[0], OPS[g]) and c.opened[g][j] is None
    return out


# ---- the MAC check ---------------------------------------------------------------------------------------------------------------------
def item_list(counts):
    """[(group, index)] in wire order; group 0 = scalar"""
    return [(g, j) for g, n in enumerate(counts) for j in range(n)]


def moved_mac(parties, counts, group, index, party):
    """the honest SPDZ open with ONE item's MAC share moved at one party: + 1, or + the generator"""
    c = honest(parties, 2, counts, salt=1)
    mac = [(list(f), list(a), list(b)) for f, a, b in c.shares[1]]
    if group == 0:
        mac[party][0][index] = (mac[party][0][index] + 1) % R
    else:
        mac[party][group][index] = O.ec_add(mac[party][group][index], O.G1_GEN if group == 1 else O.G2_GEN, OPS[group])
    name = "mac-P%d-%d.%d.%d-%s%d-party%d" % ((parties,) + tuple(counts) + ("fr g1 g2".split()[group], index, party))
    return Case(name, parties, 2, counts, [c.shares[0], mac], c.opened, verdict=ZK_ERR_MAC, note=(group, index))


@functools.lru_cache(maxsize=None)
def mac_cases():
    out = []
    for parties, counts in ((2, (2, 3, 1)), (3, (2, 3, 1)), (2, (0, 1, 0)), (1, (2, 3, 1))):
        for group, index in item_list(counts):
            out.append(moved_mac(parties, counts, group, index, parties - 1))
    out += [moved_mac(3, (2, 3, 1), group, 0, 0) for group in (0, 1, 2)]          # the leader's share
    # every item of the fused open is moved alone in some case: a G1-only and a G2-only catch among them
    assert {c.note for c in out if c.counts == (2, 3, 1) and c.parties == 2} == set(item_list((2, 3, 1)))
    assert any(c.note[0] == 1 for c in out) and any(c.note[0] == 2 for c in out) and any(c.note[0] == 0 for c in out)
    return out


# ---- what a peer may send --------------------------------------------------------------------------------------------------------------
def _affine_of(group, x, y, z):
    """the affine point of Jacobian coordinates, by the oracle's field"""
    F = OPS[group]
    zi = F.inv(z)
    zi2 = F.mul(zi, zi)
    return (F.mul(x, zi2), F.mul(y, F.mul(zi2, zi)))


def _raw_point(group, x, y, z):
    """coordinates given as raw word PATTERNS (integers below 2^384 per Fq), not field values"""
    flat = [x, y, z] if group == 1 else [x[0], x[1], y[0], y[1], z[0], z[1]]
    return [w for v in flat for w in _w(v, 6)]


@functools.lru_cache(maxsize=None)
def payload_cases():
    """[(category, Case, self)]: P = 3, additive lanes, the fused open's shape; one item of party 1's message is replaced.  Read from
    party `self`: 0 and 2 are peers of party 1 and validate its slot."""
    counts, parties, bad = (2, 3, 1), 3, 1
    base = honest(parties, 1, counts, salt=0)
    nf, n1, n2 = counts
    off_fr = lambda i: 4 * i
    off_g = {1: lambda j: 4 * nf + 18 * j, 2: lambda j: 4 * nf + 18 * n1 + 36 * j}
    out = []

    def refuse(category, name, off, raw, subgroup=False):
        out.append((category, Case("peer-" + name, parties, 1, counts, base.shares, base.opened, verdict=ZK_ERR_STATE,
                                   inject=[(0, bad, off, raw)], subgroup=subgroup)))

    refuse("scalar_r", "scalar-r", off_fr(1), _w(R, 4))
    refuse("scalar_r", "scalar-max", off_fr(0), _w(2 ** 256 - 1, 4))
    # a coordinate word pattern >= q: every coordinate of G1, every Fq2 half of G2 (q itself, and all ones)
    mont = O.fq_to_mont
    for group, j in ((1, 2), (2, 0)):
        P = base.shares[0][bad][group][j]
        assert P is not None
        coords = [P[0], P[1], 1] if group == 1 else [P[0][0], P[0][1], P[1][0], P[1][1], 1, 0]
        for k in range(len(coords)):
            for pattern in (Q, 2 ** 384 - 1):
                raw = [mont(c) for c in coords]
                raw[k] = pattern
                assert raw[k] >= Q and all(v < Q for i, v in enumerate(raw) if i != k)
                refuse("g%d_coordinate" % group, "g%d-coord%d-%s" % (group, k, "q" if pattern == Q else "ones"), off_g[group](j),
                       [w for v in raw for w in _w(v, 6)])
    for group, j in ((1, 0), (2, 0)):
        F = OPS[group]
        P = pool(group)[5]
        two = 2 if group == 1 else (2, 0)
        # Z = 2 with otherwise valid Jacobian coordinates: the same point as (x, y, 1), but not the wire's normal form
        x2, y2 = F.mul(P[0], F.mul(two, two)), F.mul(P[1], F.mul(two, F.mul(two, two)))
        assert _affine_of(group, x2, y2, two) == P and O.ec_is_on_curve(P, F) and oracle_in_subgroup(P, F)
        refuse("z_two", "g%d-z2" % group, off_g[group](j), jacobian_words(group, x2, y2, two))
        off_curve = (P[0], F.add(P[1], _one(group)))
        assert not O.ec_is_on_curve(off_curve, F)
        refuse("off_curve", "g%d-off-curve" % group, off_g[group](j), point_words(group, off_curve))
        # on the curve, outside the prime-order subgroup: refused by the malicious-security provers only
        T = cofactor_torsion_point() if group == 1 else g2_cofactor_torsion_point()
        assert T is not None and O.ec_is_on_curve(T, F) and not oracle_in_subgroup(T, F)
        refuse("outside_subgroup", "g%d-torsion-checked" % group, off_g[group](j), point_words(group, T), subgroup=True)
        shares = [[(list(f), list(a), list(b)) for f, a, b in base.shares[0]]]
        shares[0][bad][group][j] = T
        opened = (base.opened[0], list(base.opened[1]), list(base.opened[2]))
        opened[group][j] = _sum_points(group, [shares[0][p][group][j] for p in range(parties)])
        out.append(("outside_subgroup_unchecked", Case("peer-g%d-torsion-unchecked" % group, parties, 1, counts, shares, opened, subgroup=False)))
    for category in ("scalar_r", "g1_coordinate", "g2_coordinate", "z_two", "off_curve", "outside_subgroup", "outside_subgroup_unchecked"):
        assert any(c == category for c, _ in out), category
    assert any(c == "outside_subgroup" and "g1" in case.name for c, case in out)
    return out, bad


# ---- the library ----------------------------------------------------------------------------------------------------------------------
def play(case, me, subgroup=None):
    """zk_diag_small_open_host as party `me` -> (return code, verdict, opened words)"""
    from zk_mpc_amd import _lib
    sh = np.ascontiguousarray(case.share_words())
    n = words(*case.counts)
    assert sh.shape == (case.lanes, case.parties, n)
    opened = np.zeros(n, dtype=np.uint64)
    verdict = C.c_int(12345)
    rc = _lib.load().zk_diag_small_open_host(case.parties, me, case.lanes, int(case.subgroup if subgroup is None else subgroup), *case.counts,
                                             sh.ctypes.data_as(C.c_void_p), opened.ctypes.data_as(C.c_void_p), C.byref(verdict))
    return rc, verdict.value, opened
