"""GPU: the transform over G1 points (csrc/g1_ntt.hip) through zk_diag_g1_ntt_dev against the discrete-log identity -- the input is
k_i G, the expected output (DFT of k over Fr) G with both sets of points from zk_fixed_base_g1_dev (an independently tested kernel) --
and, up to 2^6, word for word against the host twin and the oracle's points.  2^6 -> 2^7 crosses one wave of butterflies; 2^10 spans
several blocks and every level."""
import numpy as np
import pytest

import zk_mpc_amd.convert as cv
from zk_mpc_amd import api
from helpers import mont1
import g1_ntt_cases as NC

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 6, 7, 10]
_POINTS = {}


def dev_points(ctx, k):
    """k_i G from the fixed-base kernel (a zero scalar gives infinity), cached per scalar vector"""
    key = tuple(k)
    if key not in _POINTS:
        dk = ctx.upload(cv.fr_to_mont(list(k)))
        b = ctx.fixed_base(dk.ptr, len(k), 1, mont1(1))
        _POINTS[key] = b.download()
        b.free(); dk.free()
    return _POINTS[key]


@pytest.mark.parametrize("inverse_root", [False, True])
@pytest.mark.parametrize("log_n", SIZES)
@pytest.mark.parametrize("case", NC.CASES)
def test_device_transform_is_the_scalar_transform_in_the_exponent(ctx, case, log_n, inverse_root):
    k = NC.scalars(case, log_n, inverse_root)
    want = NC.transformed(k, inverse_root)
    pts = dev_points(ctx, k)
    assert pts.shape == (1 << log_n, 12)
    if case in ("zeros", "unit"):
        assert not pts[-1].any()                                       # infinity in the last slot
    if case == "zero_output":
        assert want[-1] == 0
    got = ctx.g1_ntt(pts, inverse_root)
    assert np.array_equal(got, dev_points(ctx, want))
    if log_n <= 6:
        assert np.array_equal(pts, NC.points_of(k))
        assert np.array_equal(got, api.g1_ntt_host(pts, inverse_root))
        assert np.array_equal(got, NC.points_of(want))


@pytest.mark.parametrize("log_n", SIZES)
def test_two_vectors_share_the_twiddles(ctx, log_n):
    a, b = NC.scalars("random", log_n), NC.scalars("zeros", log_n)
    got = ctx.g1_ntt(np.stack([dev_points(ctx, a), dev_points(ctx, b)]), True)
    assert got.shape == (2, 1 << log_n, 12)
    assert np.array_equal(got[0], dev_points(ctx, NC.transformed(a, True)))
    assert np.array_equal(got[1], dev_points(ctx, NC.transformed(b, True)))
    if log_n <= 6:
        assert np.array_equal(got, api.g1_ntt_host(np.stack([NC.points_of(a), NC.points_of(b)]), True))


def test_the_hook_refuses_what_it_cannot_take(ctx):
    import ctypes as C
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    pts = NC.points_of(NC.scalars("random", 1))
    out = np.zeros_like(pts)
    lib = ctx.lib
    assert lib.zk_diag_g1_ntt_dev(ctx.h, p(pts), 1, 1, 0, p(out)) == 0
    assert lib.zk_diag_g1_ntt_dev(ctx.h, None, 1, 1, 0, p(out)) == -2
    assert lib.zk_diag_g1_ntt_dev(ctx.h, p(pts), 1, 1, 0, None) == -2
    assert lib.zk_diag_g1_ntt_dev(None, p(pts), 1, 1, 0, p(out)) == -2
    assert lib.zk_diag_g1_ntt_dev(ctx.h, p(pts), 13, 1, 0, p(out)) == -2
    bad = pts.copy()
    bad[0, 6:] = np.uint64(0xffffffffffffffff)
    assert lib.zk_diag_g1_ntt_dev(ctx.h, p(bad), 1, 1, 0, p(out)) == -2
