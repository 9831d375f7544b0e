"""Inputs that make the rare branches of the group law common inside the MSM kernels (no GPU here).

Every table entry is a small multiple m_i * P of ONE random subgroup point, m_i in [-J, J] and m_i = 0 the point at infinity (a
ninth of every table).  Every partial sum anywhere in an MSM over such a table -- a segment, a fold tree, a row, column or bit sum,
the host's Horner chain -- is a multiple of P again, so an addition meets a doubling (acc == point), a cancellation (acc == -point)
or an infinity with a probability of order 1 / J instead of 2^-250, and the result is the closed form (sum s_i m_i mod r) * P: one
scalar multiplication in the oracle.

The scalar sets (lists of ints below r, one per table entry):
  uniform   full-width scalars: every window and stage, collisions by chance everywhere
  equal     one full-width value for all: one bucket per window holds everything and is cut into segments whose sums are small
            multiples -- the light fold, the heavy fold and, past FOLD_GROUP segments, the two-level fold
  boolean   mostly 0 and 1 with a full-width scalar now and then: the same for one very heavy bucket
  certain   built from the job's window plan: every scalar has ONE non-zero digit, and whole buckets are laid out so that the
            event happens whatever order the sort leaves the entries in (certain_scalars)

The window plan is what csrc/msm.hip::make_plan and csrc/fixed_base.hip::precompute_window_bits compute; model_plan restates them so
that the sets can be built and counted on the CPU (test_msm_degenerate_model.py).  The GPU test builds the certain set from the
record of the job itself (Context.msm_plans) and checks that the two agree.
"""
import bisect
import itertools

import numpy as np

import zkref as O
import zk_mpc_amd.convert as cv

J = 4
R = O.R_MOD
KINDS = ("dbl_pair", "neg_pair", "neg_triple", "dbl_triple")
CERTAIN_TARGET = 240           # buckets per kind where the table has the entries for them (six index orders in equal shares)
# (a, b, a + b): a doubling when a and b come first; (a, b, -(a + b)): a cancellation at the third entry in every order.  No two
# of a triple are equal or opposite, so nothing else happens on the way.
_TRIPLES = ((1, 2), (-1, -2), (1, 3), (-1, -3))


# ---- the table ---------------------------------------------------------------------------------------------------------------------
def multiples(n, seed):
    """m_i, uniform on [-J, J]: a ninth of the entries are at infinity."""
    return np.random.RandomState(seed).randint(-J, J + 1, size=n).astype(np.int64)


def base_point(group, seed):
    k = O.Prng(0xD06E + seed).fr() or 1
    return O.g1_mul(O.G1_GEN, k) if group == 1 else O.g2_mul(O.G2_GEN, k)


def small_multiples(group, P):
    """[m * P for m in -J .. J] as oracle points (None in the middle)."""
    mul, neg = (O.g1_mul, O.g1_neg) if group == 1 else (O.g2_mul, O.g2_neg)
    pos = [mul(P, m) for m in range(1, J + 1)]
    return [neg(p) for p in reversed(pos)] + [None] + pos


def table(group, n, seed):
    """-> (ms, point array in the ABI's form, P).  The 2J + 1 distinct rows are converted once and indexed."""
    ms = multiples(n, seed)
    P = base_point(group, seed)
    rows = (cv.g1_affine_to_array if group == 1 else cv.g2_affine_to_array)(small_multiples(group, P))
    return ms, np.ascontiguousarray(rows[ms + J]), P


def table_points(group, ms, P):
    """The table as oracle points (small n only)."""
    rows = small_multiples(group, P)
    return [rows[int(m) + J] for m in ms]


def expected(group, P, ms, scalars, off=0, m=None):
    """sum_{i < m} scalars[i] * table[off + i] in closed form: an affine oracle point, or None."""
    m = len(scalars) if m is None else m
    e = sum(int(s) * int(k) for s, k in zip(scalars[:m], ms[off:off + m])) % R
    return (O.g1_mul if group == 1 else O.g2_mul)(P, e)


def to_mont(scalars):
    """ints below r -> (n, 4) uint64 in the reference's Montgomery form (cv.fr_to_mont, without a Python loop per limb)."""
    f = cv._FR_R
    raw = b"".join((int(s) * f % R).to_bytes(32, "little") for s in scalars)
    return np.frombuffer(raw, dtype="<u8").reshape(-1, 4).copy()


# ---- the window plan (csrc/msm.hip::make_plan, csrc/fixed_base.hip::precompute_window_bits) --------------------------------------------
def _round_log2(n):
    lg = 0
    while (3 << lg) <= 2 * n:
        lg += 1
    return lg


def precompute_window_bits(n):
    lg = _round_log2(n)
    c0 = 20 if lg >= 19 else 17 if lg >= 16 else (min(lg + 1, 15) if lg >= 13 else lg + 2)
    if lg == 16 and n < 65000:
        c0 = 15
    lo, hi = (13, 20) if lg >= 16 else (9, 16)
    c0 = min(max(c0, lo), hi)
    need = min(10, max(3, lg - 3))
    for t in (0, -1, 1, -2, 2, -3, 3, 4, 5):
        c = c0 + t
        if c < lo - 1 or c > 20:
            continue
        W = (255 + c - 1) // c
        if 255 - c * (W - 1) >= need:
            return c
    return 16


def model_plan(n, merged, vectors=1, n_cu=256):
    """What the library plans for one vector of n scalars: plain table (per-window bucket sets, the 255 bits spread evenly) or a table
    of window multiples (merged: one bucket set, uniform windows).  The keys are those of Context.msm_plans()."""
    if merged:
        c = precompute_window_bits(n)
        W = (255 + c - 1) // c
        off = [w * c for w in range(W + 1)]
    else:
        lg = _round_log2(n)
        c = min(max(lg - (2 if lg <= 15 else 4), 4), 16)
        W = (255 + c - 1) // c
        base, extra = divmod(255, W)
        off = [0]
        for w in range(W):
            off.append(off[-1] + base + (1 if w < extra else 0))
        c = base + (1 if extra else 0)
    digits = n * W * vectors
    lanes = n_cu * 4 * 64 * 2
    seg = 8 if digits <= 1 << 19 else 32
    while seg < (digits + lanes - 1) // lanes and seg < 4096:
        seg <<= 1
    return {"n": n * vectors, "c": c, "W": W, "off": off, "NB": 1 << (c - 1), "Wb": vectors * (1 if merged else W), "seg": seg,
            "table": "limbs" if merged else "plain", "vectors": vectors}


def plan_digits(plan, scalars):
    """The signed window digits of the scalars under the plan's windows (csrc/msm_digits.cuh): an (n, W) int64 array."""
    off, W = plan["off"], plan["W"]
    bias = sum(1 << (off[w + 1] - 1) for w in range(W))
    limbs = np.frombuffer(b"".join((int(s) + bias).to_bytes(40, "little") for s in scalars), dtype="<u8").reshape(-1, 5)
    out = np.empty((len(scalars), W), dtype=np.int64)
    for w in range(W):
        cw, li, sh = off[w + 1] - off[w], off[w] // 64, off[w] % 64
        v = limbs[:, li] >> np.uint64(sh)
        if sh + cw > 64:
            v = v | (limbs[:, li + 1] << np.uint64(64 - sh))
        out[:, w] = (v & np.uint64((1 << cw) - 1)).astype(np.int64) - (1 << (cw - 1))
    return out


# ---- the scalar sets -----------------------------------------------------------------------------------------------------------------
def _wide(rs):
    return int.from_bytes(rs.bytes(40), "little") % R


def uniform_scalars(n, seed):
    rs = np.random.RandomState(seed)
    return [_wide(rs) for _ in range(n)]


def equal_scalars(n, seed):
    return [_wide(np.random.RandomState(seed)) or 1] * n


def boolean_scalars(n, seed):
    rs = np.random.RandomState(seed)
    bits = rs.randint(0, 2, size=n)
    return [_wide(rs) if i % 61 == 60 else int(bits[i]) for i in range(n)]


def _bucket_cap(plan):
    """How many buckets _bucket_of can name."""
    W, off = plan["W"] - 1, plan["off"]
    if plan["table"] != "plain":
        return plan["NB"] - 1
    return W * ((1 << (min(off[w + 1] - off[w] for w in range(W)) - 1)) - 1)


def _bucket_of(plan, t):
    """The t-th bucket the certain set uses -> (window, digit).  The top window is left alone (a scalar stays below r).  Over a table
    of window multiples all windows share one bucket set and an entry is the point 2^(c w) m P: the buckets are told apart by the
    digit alone, and all entries of one bucket sit in one window."""
    W = plan["W"] - 1
    if t >= _bucket_cap(plan):
        raise ValueError("the plan has %d buckets for the certain set, bucket %d asked for" % (_bucket_cap(plan), t))
    return t % W, 1 + (t if plan["table"] != "plain" else t // W)


def certain_count(n, target=CERTAIN_TARGET):
    """Buckets per kind over a table of n entries: ten entries per four buckets, and every triple takes one of the n / 9 entries
    +-P and one of the n / 9 entries +-3 P -- a twentieth of n, in whole sixes."""
    return min(target, n // 20 // 6 * 6)


def certain_layout(plan, ms, seed, target=CERTAIN_TARGET):
    """-> (buckets, filler): buckets = [(kind, (window, digit), [table indices])] in which the event is certain; filler = table
    indices left over.  Kinds, with k buckets each (k = target where the table has the entries, else as many sixes as it has):
      dbl_pair    {m, m}: a doubling in either order
      neg_pair    {m, -m}: a cancellation in either order
      neg_triple  {a, b, -(a + b)}: a cancellation on an accumulator with zz != 1 in every order
      dbl_triple  {a, b, a + b}: a doubling on an accumulator with zz != 1 when a + b comes last -- the entries' table indices are
                  laid out in each of the six orders for a sixth of the buckets, so that is a third of them whatever order the
                  sort keeps"""
    k = certain_count(len(ms), target)
    free = {v: [int(i) for i in np.nonzero(ms == v)[0]] for v in range(-J, J + 1) if v}

    def take(v, after=-1):
        lst = free[v]
        pos = bisect.bisect_right(lst, after)
        return lst.pop(pos) if pos < len(lst) else None

    def put_back(pairs):
        for v, i in pairs:
            bisect.insort(free[v], i)

    def take_ordered(values):
        """one index per value, increasing in the order given"""
        got, last = [], -1
        for v in values:
            i = take(v, last)
            if i is None:
                put_back(got)
                return None
            got.append((v, i))
            last = i
        return [i for _, i in got]

    buckets = []
    perms = list(itertools.permutations(range(3)))
    for kind in ("neg_triple", "dbl_triple", "dbl_pair", "neg_pair"):      # (every triple needs a +-1 and a +-3: they choose first)
        made, tries = 0, 0
        while made < k and tries < 8 * k + 64:
            var = tries
            tries += 1
            if kind == "dbl_pair":
                m = (var % J + 1) * (1 if (var // J) % 2 == 0 else -1)
                idx = take_ordered((m, m))
            elif kind == "neg_pair":
                m = (var % J + 1) * (1 if (var // J) % 2 == 0 else -1)
                idx = take_ordered((m, -m))
            else:
                a, b = _TRIPLES[var % len(_TRIPLES)]
                vals = (a, b, a + b if kind == "dbl_triple" else -(a + b))
                order = perms[made % 6]                          # the values in increasing table index
                idx = take_ordered([vals[j] for j in order])
            if idx is None:
                continue
            buckets.append((kind, _bucket_of(plan, len(buckets)), idx))
            made += 1
    filler = sorted(i for lst in free.values() for i in lst) + [int(i) for i in np.nonzero(ms == 0)[0]]
    return buckets, filler


def certain_scalars(plan, ms, seed, target=CERTAIN_TARGET):
    """One non-zero digit per scalar (certain_layout); the entries left over get one random digit in a bucket of their own range, the
    entries at infinity included."""
    n = len(ms)
    off = plan["off"]
    buckets, filler = certain_layout(plan, ms, seed, target)
    out = [0] * n
    for _, (w, d), idx in buckets:
        for i in idx:
            out[i] = d << off[w]
    rs = np.random.RandomState(seed)
    t0, cap = len(buckets), _bucket_cap(plan)
    assert cap > t0, "no bucket left for the entries outside the certain buckets"
    for i in filler:
        w, d = _bucket_of(plan, int(rs.randint(t0, cap)))
        out[i] = d << off[w]
    assert all(0 <= s < R for s in out)
    return out


def scalar_sets(plan, ms, seed):
    """name -> scalars, for one job of the plan's (single-vector) length"""
    n = len(ms)
    return {"uniform": uniform_scalars(n, seed + 1), "equal": equal_scalars(n, seed + 2), "boolean": boolean_scalars(n, seed + 3),
            "certain": certain_scalars(plan, ms, seed + 4)}


# ---- the integer model of the accumulate kernel ---------------------------------------------------------------------------------------
def count_events(plan, ms, scalars, order, seed=0):
    """Run the accumulate kernel's chains on running MULTIPLES: the non-zero digits go to their buckets (entries in ascending,
    descending or shuffled table order), a bucket is cut into segments of plan["seg"] entries, and every segment is one chain that
    starts at infinity.  The accumulator a meets the entry m (a table entry at infinity is skipped, as the kernels skip it): a
    restart if a == 0, a doubling if a == m, a cancellation if a == -m, else a += m.  depth counts the points the accumulator is
    made of; an event with depth >= 2 is on an accumulator that is not fresh (zz != 1).  Over a table of window multiples the entry
    of window w is the point 2^(c w) m P and a is kept per window: equal only if equal window by window (never over-counts).
    -> dict of counts."""
    n, W, seg = len(ms), plan["W"], plan["seg"]
    merged = plan["table"] != "plain"
    dg = plan_digits(plan, scalars)
    ii, ww = np.nonzero(dg)
    d = dg[ii, ww]
    key = (np.abs(d) - 1) if merged else ww * plan["NB"] + np.abs(d) - 1
    val = ms[ii] * np.sign(d)
    if order == "ascending":
        rank = ii * W + ww
    elif order == "descending":
        rank = -(ii * W + ww)
    else:
        rank = np.random.RandomState(seed).permutation(len(ii))
    o = np.lexsort((rank, key))
    key, val, ww = key[o], val[o], ww[o]
    first = np.r_[0, np.nonzero(np.diff(key))[0] + 1]            # start of every bucket
    pos = np.arange(len(key)) - np.repeat(first, np.diff(np.r_[first, len(key)]))
    chain = np.cumsum((pos % seg) == 0) - 1                      # segment number of every entry
    step = pos % seg
    nchain = int(chain[-1]) + 1 if len(chain) else 0
    D = W if merged else 1
    acc = np.zeros((nchain, D), dtype=np.int64)
    depth = np.zeros(nchain, dtype=np.int64)
    res = dict(restart=0, inf_entry=0, dbl=0, neg=0, dbl_deep=0, neg_deep=0, add=0)
    for k in range(int(step.max()) + 1 if len(step) else 0):
        sel = np.nonzero(step == k)[0]
        ch, m, col = chain[sel], val[sel], (ww[sel] if merged else np.zeros(len(sel), dtype=np.int64))
        live = m != 0
        res["inf_entry"] += int((~live).sum())
        ch, m, col = ch[live], m[live], col[live]
        a = acc[ch]
        here = a[np.arange(len(ch)), col]
        others_zero = (np.abs(a).sum(axis=1) - np.abs(here)) == 0
        empty = others_zero & (here == 0)
        same = others_zero & (here == m) & ~empty
        opp = others_zero & (here == -m) & ~empty
        deep = depth[ch] >= 2
        res["restart"] += int(empty.sum())
        res["dbl"] += int(same.sum()); res["dbl_deep"] += int((same & deep).sum())
        res["neg"] += int(opp.sum()); res["neg_deep"] += int((opp & deep).sum())
        res["add"] += int((~empty & ~same & ~opp).sum())
        acc[ch, col] = here + m
        depth[ch] = np.where(opp, 0, np.where(empty, 1, depth[ch] + 1))
    return res


# ---- the kernel paths and the smallest shapes that reach them ------------------------------------------------------------------------
# layout: 0 = the plain table, 1 .. 3 = Bases.precompute(layout) (packed, one point per line, limbs with both signs); jobs > 1: a
# group through Context.msm_batch_dev; vectors > 1: one job through Context.msm_multi_dev.  want: what the job's record must say
# (the jobs in its accumulate launch and the vectors in the job among it).
def _case(id, group, n, layout=0, jobs=1, vectors=1, **want):
    return dict(id=id, group=group, n=n, layout=layout, jobs=jobs, vectors=vectors, want=dict(want, jobs=jobs, vectors=vectors))


_SINGLE = dict(accum_launch="single", fold_launch="single")
_G1_SINGLE = dict(_SINGLE, accum_lanes=1, fold_lanes=1)
_GROUP = dict(accum_launch="group", fold_launch="group")
CASES = [
    _case("g1-plain-counting-dual", 1, 300, table="plain", sort="counting", reduce="RedG1Dual", **_G1_SINGLE),
    _case("g1-plain-bucket-red1", 1, 24576, table="plain", sort="bucket", reduce="RedG1", **_G1_SINGLE),
    _case("g1-limbs-oneblock", 1, 512, 3, table="limbs", sort="one_block", reduce="RedG1Dual", **_G1_SINGLE),
    _case("g1-packed-oneblock", 1, 512, 1, table="packed", sort="one_block", reduce="RedG1Dual", **_G1_SINGLE),
    _case("g1-line-oneblock", 1, 512, 2, table="line", sort="one_block", reduce="RedG1Dual", **_G1_SINGLE),
    _case("g1-limbs-bucket", 1, 8192, 3, table="limbs", sort="bucket", reduce="RedG1Dual", **_G1_SINGLE),
    _case("g1-group-limbs-dual", 1, 512, 3, jobs=3, table="limbs", sort="one_block_group", accum_lanes=2, fold_lanes=2, reduce="RedG1Dual", **_GROUP),
    _case("g1-group-packed-dual", 1, 512, 1, jobs=3, table="packed", sort="one_block_group", accum_lanes=2, fold_lanes=2, reduce="RedG1Dual", **_GROUP),
    _case("g1-group-limbs-lane", 1, 8192, 3, jobs=2, table="limbs", accum_lanes=1, fold_lanes=2, reduce="RedG1Dual", **_GROUP),
    _case("g1-group-packed-lane", 1, 8192, 1, jobs=2, table="packed", accum_lanes=1, fold_lanes=2, reduce="RedG1Dual", **_GROUP),
    _case("g1-group-red1", 1, 65536, 3, jobs=2, table="limbs", accum_lanes=1, fold_lanes=1, reduce="RedG1", **_GROUP),
    _case("g1-multi-plain", 1, 1024, 0, vectors=5, table="plain", sort="bucket", **_G1_SINGLE),
    _case("g1-multi-limbs", 1, 1024, 3, vectors=5, table="limbs", sort="bucket", **_G1_SINGLE),
    _case("g2-plain-quad", 2, 300, table="plain", accum_lanes=4, fold_lanes=4, reduce="RedG2Quad", **_SINGLE),
    _case("g2-packed-quad", 2, 512, 1, table="packed", accum_lanes=4, fold_lanes=4, reduce="RedG2Quad", **_SINGLE),
    _case("g2-plain-pair-redquad", 2, 6000, table="plain", accum_lanes=2, fold_lanes=2, reduce="RedG2Quad", **_SINGLE),
    _case("g2-plain-pair-redpair", 2, 24576, table="plain", sort="bucket", accum_lanes=2, fold_lanes=2, reduce="RedG2Pair", **_SINGLE),
    _case("g2-multi-plain", 2, 1024, 0, vectors=5, table="plain", sort="bucket", **_SINGLE),
]


def case_plan(case, n_cu=256):
    """The model's plan for one vector of a case (its seg is that of the whole job: all vectors)."""
    return model_plan(case["n"], case["layout"] != 0, case["vectors"], n_cu) | {"n": case["n"], "table": ("plain", "packed", "line", "limbs")[case["layout"]]}
