"""GPU parity, exact: the whole NTT (csrc/ntt.hip) against the C oracle's ref_fft, element for element, at every size from 2^0
to 2^24 and for all four kinds; the witness map's batched transforms against the oracle's witness map.  No tolerance anywhere:
every check is bit equality of 4 x u64 residues, which also proves the device's outputs canonical.

The launch plan per size, as ntt_run derives it (ntt_cases.plan restates it; C = 2^logC columns per tile; "remap" = the grid is a
multiple of 8 and takes the XCD tile remap):

#  log_n  passes  logM      logE  logC      tiles  remap
#      0       0  -           0  -             0  no      nothing runs (the inverse kinds: k_bitrev_scale's scale only)
#      1       1  1           1  0             1  no      the radix-2 level alone (nst == 1), emits from the first level
#      2       1  2           2  0             1  no      one radix-4 stage, first && last
#      3       1  3           3  0             1  no      radix-2 level, then a stage that is last but not first
#      4       1  4           4  0             1  no      two stages (first, last)
#      5       1  5           5  0             1  no
#      6       1  6           6  0             1  no      a middle stage (neither first nor last)
#      7       1  7           7  0             1  no
#      8       1  8           8  0             1  no
#      9       1  9           9  0             1  no
#     10       1  10         10  0             1  no      the largest transform with the separate k_bitrev_scale
#     11       2  6+5         6  0/1          32  yes     two passes from here: inter-pass twiddles, scatter in the last pass
#     12       2  6+6         6  0/0          64  yes
#     13       2  7+6         7  0/1          64  yes
#     14       2  7+7         7  0/0         128  yes
#     15       2  8+7         8  0/1         128  yes
#     16       2  8+8         8  0/0         256  yes
#     17       2  9+8         9  0/1         256  yes
#     18       2  9+9        10  1/1         256  yes
#     19       2  10+9       11  1/2         256  yes
#     20       2  10+10      12  2/2         256  yes     4 096-element tiles, 10-level passes
#     21       3  7+7+7      10  3/3/3      2048  yes     three passes from here, 1 024-element tiles
#     22       3  8+7+7      10  2/3/3      4096  yes
#     23       3  8+8+7      10  2/2/3      8192  yes
#     24       3  8+8+8      10  2/2/2     16384  yes
"""
import numpy as np
import pytest

import ntt_cases as NC
import zkref as O
import zkref_c as OC
import zk_mpc_amd as Z
from helpers import circuit_system, csr

pytestmark = pytest.mark.gpu


def device_ntt(ctx, v, log_n, inverse, coset):
    d = ctx.upload(v)
    try:
        ctx.ntt_dev(d.ptr, log_n, bool(inverse), bool(coset))
        return ctx.download(d, (1 << log_n, 4))
    finally:
        d.free()


def check(ctx, v, log_n, inverse, coset, label):
    want = OC.fft(v, log_n, inverse, coset, threads=OC.num_threads())
    bad = NC.mismatch(device_ntt(ctx, v, log_n, inverse, coset), want)
    assert bad is None, "%s %s at log_n %d: %s (plan %s)" % (label, NC.KIND_NAME[inverse, coset], log_n, bad, NC.plan(log_n))
    return want


@pytest.mark.parametrize("log_n", range(25))
def test_ntt_equals_oracle(ctx, log_n):
    """zk_fr_ntt_dev == ref_fft on the whole vector, for all four kinds.  Families (ntt_cases.family): uniform random below r;
    every element r - 1; a random 0 / r - 1 mask; r - 1 at even and 1 at odd indices; a delta at an index with all bits but one
    set; the geometric vector w^(m j), m odd near N / 3.  The r - 1 families push the lazy ranges of the radix-4 stages (sums of
    maximal residues, differences of 0 and r - 1) through every level and pass, where random data stays in the middle.  For the
    delta and the geometric vector the forward transform is also held against its closed form (a twiddle column; N at one bin),
    computed with python integers alone.
    Up to 2^22 every family runs in every kind.  At 2^23 and 2^24 random and all-(r - 1) run in every kind and the delta forward
    only, its closed form held at 4 096 + 3 positions (both ends, the middle, random ones) instead of all.  With every family at
    those two sizes this file took 97 s on an MI355X host (35 s at 2^24, 17 s at 2^23, much of it python loops building 2^24-term
    geometric vectors) next to 16 s for the Fr vector, polynomial and NTT tests that existed; it takes 77 s now.  The families
    of these two sizes were cut first; no size is left out, and up to 2^22 nothing is cut.
    log_n 25 .. 28 stay out: a buffer, its scratch copy and the three 36-byte tables per element are tens of GB, and nothing
    benchmarks those sizes."""
    big = log_n >= 23
    for name in NC.FAMILIES:
        if big and name in ("mask_0_r-1", "alt_r-1_1", "geometric"):
            continue
        v = NC.family(name, log_n)
        assert NC.below_r(v).all()
        closed = name in ("delta", "geometric")
        for inverse, coset in NC.KINDS:
            if big and closed and (inverse, coset) != (0, 0):
                continue
            want = check(ctx, v, log_n, inverse, coset, name)
            if not closed or (inverse, coset) != (0, 0):
                continue
            # device == oracle is asserted above: this holds both to the definition
            if big:
                ks = np.concatenate([[0, (1 << log_n) // 2, (1 << log_n) - 1], np.random.RandomState(log_n).randint(0, 1 << log_n, 4096)])
                bad = NC.mismatch(want[ks], NC.delta_forward_at(log_n, ks))
            else:
                bad = NC.closed_form_mismatch(name, log_n, 0, 0, want)
            assert bad is None, "%s: closed form at log_n %d: %s" % (name, log_n, bad)


@pytest.mark.parametrize("log_n", [3, 10, 12, 17])
@pytest.mark.parametrize("coset_first", [False, True])
def test_ntt_table_order(log_n, coset_first):
    """get_domain builds the coset tables on the first coset call of a size: a fresh context per order of first use."""
    kinds = sorted(NC.KINDS, key=lambda k: k[1], reverse=coset_first)
    c = Z.Context(0)
    try:
        for name in ("random", "mask_0_r-1"):
            v = NC.family(name, log_n)
            for inverse, coset in kinds:
                check(c, v, log_n, inverse, coset, "%s (coset %s)" % (name, "first" if coset_first else "last"))
    finally:
        c.close()


@pytest.mark.parametrize("n,log_n", [((1 << 17) - 5, 17), ((1 << 20) + 1, 21)])
def test_ntt_host_vector_zero_padding(ctx, n, log_n):
    """zk_fr_fft_in_place pads n < 2^log_n elements with zeros on the device, at a two-pass and a three-pass size."""
    v = NC.uniform(np.random.RandomState(n), n)
    padded = np.zeros((1 << log_n, 4), dtype=np.uint64)
    padded[:n] = v
    fns = {(0, 0): ctx.fft_in_place, (1, 0): ctx.ifft_in_place, (0, 1): ctx.coset_fft_in_place, (1, 1): ctx.coset_ifft_in_place}
    for (inverse, coset), fn in fns.items():
        bad = NC.mismatch(fn(v, log_n), OC.fft(padded, log_n, inverse, coset, threads=OC.num_threads()))
        assert bad is None, "%s: %s" % (NC.KIND_NAME[inverse, coset], bad)
        assert np.array_equal(padded[:n], v)


def check_witness_map(ctx, dr, cr, dz, z, k):
    assert dr.domain_log == k == cr.domain_log
    dh = ctx.alloc(32 << k)
    try:
        ctx.witness_map_dev(dr, dz.ptr, dh.ptr)
        bad = NC.mismatch(ctx.download(dh, (1 << k, 4)), OC.witness_map(cr, z, OC.num_threads()))
        assert bad is None, "witness map at 2^%d: %s (plan %s)" % (k, bad, NC.plan(k))
    finally:
        dh.free()


@pytest.mark.parametrize("k", range(2, 22))
def test_witness_map_mul_chain_exact(ctx, k):
    """zk_groth16_witness_map_dev runs zk_ntt_launch_batch with three transforms per launch (inverse, then coset) around the
    fused (ab - c) / Z: the whole h vector against the oracle's, for the mul-chain of 2^k - 2 constraints (domain exactly 2^k)."""
    n = (1 << k) - 2
    rng = O.Prng(9000 + k)
    w0, w1 = NC.limbs([NC.mont(rng.fr())])[0], NC.limbs([NC.mont(rng.fr())])[0]
    dr = ctx.r1cs_mul_chain(n)
    dz = ctx.mul_chain_assignment_dev(n, w0, w1)
    try:
        z = ctx.download(dz, (n + 3, 4))
        check_witness_map(ctx, dr, OC.R1cs(2, n + 1, *OC.mul_chain_csr(n)), dz, z, k)
    finally:
        dz.free()
        dr.free()


@pytest.mark.parametrize("k", [4, 10, 11, 16])
def test_witness_map_circuit_shaped_exact(ctx, k):
    """The same on matrices that are not the chain's: several terms per row, non-unit coefficients (tools/synth_r1cs.py)."""
    r1cs, z = circuit_system((10, 3, 2) if k == 4 else k, 700 + k)
    mats = [csr(m) for m in (r1cs.a, r1cs.b, r1cs.c)]
    dr = ctx.r1cs_upload(r1cs.num_instance, r1cs.num_witness, *mats)
    zm = NC.limbs(NC.mont(x) for x in z)
    dz = ctx.upload(zm)
    try:
        check_witness_map(ctx, dr, OC.R1cs(r1cs.num_instance, r1cs.num_witness, *mats), dz, zm, k)
    finally:
        dz.free()
        dr.free()
