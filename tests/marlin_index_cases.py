"""The constraint systems the tests of Marlin::index as one call (zk_marlin_index_build) run on, given as the circuit gives them --
neither padded nor square -- and what the oracle (oracle/marlin_ref.py) makes of them.  Shared by tests/test_marlin_shape_host.py
(the integer shaping, no device) and tests/test_gpu_marlin_index.py."""
import marlin_ref as M
import zkref as O
from helpers import csr, marlin_test_system

# the systems of tests/test_gpu_marlin.py::test_rounds_match_oracle, under its seeds
GPU_MARLIN_SYSTEMS = [3, 6, 13, 40, "tiny5", "tiny11", "dense5", "dense6"]


def seed_of(n):
    return 800 + (n if isinstance(n, int) else len(n) * 7 + int(n[-1]))


def _hand(ni, nw, a, b, c):
    return O.R1CS(ni, nw, a, b, c), [1] + [(7 * i + 3) % O.R_MOD for i in range(1, ni + nw)]


def hand_built(name):
    """Small systems that pin one property each (the assignments satisfy nothing: shaping reads no value)."""
    if name == "more_constraints":          # 10 constraints over 2 + 3 variables: squaring adds witnesses
        rows = lambda k: [[(3 + r + k, (r + k) % 5)] for r in range(10)]
        return _hand(2, 3, rows(0), rows(1), rows(2))
    if name == "three_instance":            # instance of 3: one zero is inserted, witness columns move up
        a = [[(2, 0), (3, 3)], [(5, 2), (7, 4), (11, 1)], [(13, 5)]]
        b = [[(1, 4)], [(1, 1)], [(17, 3), (19, 2)]]
        c = [[(1, 5)], [(23, 0), (29, 3)], [(1, 4)]]
        return _hand(3, 3, a, b, c)
    if name == "swap_some":                 # densities 6 / 4: rows 0 and 1 change places, then B is the denser one
        a = [[(2, 0), (3, 1)], [(5, 2), (7, 3)], [(11, 4)], [(13, 5)]]
        b = [[(17, 1)], [(19, 2)], [(23, 3)], [(29, 4)]]
        c = [[(1, 5)], [(1, 4)], [(1, 3)], [(1, 2)]]
        return _hand(2, 4, a, b, c)
    if name == "swap_none":                 # A is the sparser matrix from the start
        a = [[(2, 0)], [(3, 1)], [(5, 2)], [(7, 3)]]
        b = [[(11, 1), (13, 2)], [(17, 2), (19, 3)], [(23, 3), (29, 4)], [(31, 4), (37, 5)]]
        c = [[(1, 5)], [(1, 4)], [(1, 3)], [(1, 2)]]
        return _hand(2, 4, a, b, c)
    if name == "empty_c":                   # a matrix with no entries
        a = [[(2, 0), (3, 1)], [(5, 2)], [(7, 3)]]
        b = [[(11, 1)], [(13, 2)], [(17, 3)]]
        return _hand(2, 2, a, b, [[], [], []])
    if name == "repeated_column":           # a row that names column 3 twice, out of order: the sort must be stable
        a = [[(5, 3), (7, 1), (9, 3), (4, 0)], [(2, 2)], [(3, 4), (6, 4)]]
        b = [[(11, 1)], [(13, 3), (15, 3)], [(17, 0)]]
        c = [[(1, 4)], [(1, 2)], [(21, 5), (22, 2), (23, 5)]]
        return _hand(2, 4, a, b, c)
    raise KeyError(name)


HAND_BUILT = ["more_constraints", "three_instance", "swap_some", "swap_none", "empty_c", "repeated_column"]


def system(name):
    """-> (R1CS as the circuit gives it, its assignment)."""
    if name in HAND_BUILT:
        return hand_built(name)
    return marlin_test_system(name, O.Prng(seed_of(name)))


def host_arrays(r1cs):
    """The unpadded system as Context.r1cs_upload / NativeIndex / shape_host take it."""
    return (r1cs.num_instance, r1cs.num_witness, csr(r1cs.a), csr(r1cs.b), csr(r1cs.c))


def oracle_shape(r1cs, z):
    """pad_and_square, balance_matrices, every row sorted by column (stable), the transposes as calculate_t walks them, the
    sizes.  -> (info dict, [A, B, C, At, Bt, Ct] as rows of (coeff, index), the swap flag of every row, the padded assignment)."""
    sq, zz = M.pad_and_square(r1cs, z)
    a, b, c = [list(r) for r in sq.a], [list(r) for r in sq.b], [list(r) for r in sq.c]
    rows_before = list(a)                   # (the row objects themselves: balance_matrices moves them)
    nnz = max(sum(len(r) for r in m) for m in (a, b, c))
    M.balance_matrices(a, b)
    swapped = [a[k] is not rows_before[k] for k in range(len(a))]
    mats = [[sorted(row, key=lambda t: t[1]) for row in m] for m in (a, b, c)]
    h, k, x = M.next_pow2(sq.num_constraints), M.next_pow2(nnz), sq.num_instance
    for m in list(mats):
        t = [[] for _ in range(h)]
        for r, row in enumerate(m):
            for coeff, col in row:
                t[M.reindex_by_subdomain(h, x, col)].append((coeff, r))
        mats.append(t)
    info = {"num_instance_in": r1cs.num_instance, "num_witness_in": r1cs.num_witness, "num_constraints_in": r1cs.num_constraints,
            "num_instance": sq.num_instance, "num_witness": sq.num_witness, "num_constraints": sq.num_constraints,
            "num_non_zero": nnz, "h_size": h, "k_size": k, "b_size": M.next_pow2(3 * k - 3), "x_size": x,
            # AHPForR1CS::max_degree (ahp/mod.rs:75-97) with zk_bound = 1
            "max_degree_needed": max(2 * h + 1 - 2, 3 * h + 2 - 3, h, 3 * k - 3)}
    return info, mats, swapped, zz
