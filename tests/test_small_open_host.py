"""CPU: the small open of the collaborative provers (csrc/sharednet.hpp: wire layout `fr | g1 | g2`, validation of what peers sent,
sums, SPDZ MAC check) played on the host by zk_diag_small_open_host, against the oracle's field and group law.  The cases and what
they expect are tests/small_open_cases.py's; nothing expected here comes from the library."""
import ctypes as C

import numpy as np
import pytest

import small_open_cases as SC
from small_open_cases import ZK_ERR_ARG, ZK_ERR_MAC, ZK_ERR_STATE, ZK_OK


def test_the_wire_layout_is_the_python_partys():
    """4 / 18 / 36 words per scalar / G1 / G2 item, in that order: mpc.py: Party._open_many packs the same"""
    import zkref as O
    assert [SC.words(*c) for c in SC.COUNTS] == [98, 18, 8, 36, 36]
    m = SC.message_words(([5], [O.G1_GEN], [None]))
    assert len(m) == 4 + 18 + 36 and m[:4] == SC.fr_words(5) and m[4:22] == SC.point_words(1, O.G1_GEN) and m[22:] == SC.point_words(2, None)
    assert m[22 + 24:] == [0] * 12 and m[22:28] == SC._w(O.fq_to_mont(1), 6) and m[28:34] == [0] * 6        # infinity: (1, 1, 0)


@pytest.mark.parametrize("case", SC.sum_cases(), ids=repr)
def test_opened_values_are_the_oracles_sums_for_every_party(case):
    """additive (1 lane) and SPDZ (2 lanes, consistent MAC shares): verdict OK, and every party reads the same opened words"""
    want = case.opened_words()
    for me in range(case.parties):
        rc, verdict, opened = SC.play(case, me)
        assert (rc, verdict) == (ZK_OK, ZK_OK), (me, rc, verdict)
        assert np.array_equal(opened, want), me


@pytest.mark.parametrize("case", SC.mac_cases(), ids=repr)
def test_one_moved_mac_share_fails_the_check_for_every_party(case):
    assert case.verdict == ZK_ERR_MAC
    for me in range(case.parties):
        rc, verdict, opened = SC.play(case, me)
        assert (rc, verdict) == (ZK_OK, ZK_ERR_MAC), (me, rc, verdict)
        assert np.array_equal(opened, case.opened_words())          # the share lane opened as usual; it is the check that fails


def _payloads():
    cases, bad = SC.payload_cases()
    return [(category, case, bad) for category, case in cases]


@pytest.mark.parametrize("category,case,bad", _payloads(), ids=lambda v: repr(v) if isinstance(v, SC.Case) else None)
def test_a_peers_payload_is_validated_and_ones_own_is_not(category, case, bad):
    peers = [p for p in range(case.parties) if p != bad]
    assert len(peers) == 2
    for me in peers:
        rc, verdict, opened = SC.play(case, me)
        assert (rc, verdict) == (ZK_OK, case.verdict), (category, me, rc, verdict)
        if case.verdict == ZK_OK:                                    # (outside the subgroup, unchecked: a sum like any other)
            assert np.array_equal(opened, case.opened_words())
    # the same message in the reader's own slot is its own output: not refused
    rc, verdict, opened = SC.play(case, bad)
    assert (rc, verdict) == (ZK_OK, ZK_OK), (category, rc, verdict)
    if category == "outside_subgroup":
        # refused with the subgroup test only: without it the torsion point is a group element like any other
        for me in peers:
            assert SC.play(case, me, subgroup=False)[:2] == (ZK_OK, ZK_OK)
    if category == "outside_subgroup_unchecked":
        for me in peers:
            assert SC.play(case, me, subgroup=True)[:2] == (ZK_OK, ZK_ERR_STATE)


def test_under_spdz_a_peers_torsion_point_is_refused_before_any_mac_arithmetic():
    """2 lanes: the subgroup test is on by the case's own default, and the first exchange already refuses"""
    base = SC.honest(2, 2, (2, 3, 1), salt=0)
    bad = SC.Case("spdz-torsion", 2, 2, base.counts, base.shares, base.opened, verdict=ZK_ERR_STATE,
                  inject=[(0, 1, 4 * 2 + 18, SC.point_words(1, SC.cofactor_torsion_point()))])
    assert bad.subgroup and SC.play(bad, 0)[:2] == (ZK_OK, ZK_ERR_STATE)


def test_the_hook_refuses_what_it_cannot_take():
    from zk_mpc_amd import _lib
    lib = _lib.load()
    case = SC.honest(2, 1, (2, 0, 0))
    sh = np.ascontiguousarray(case.share_words())
    out = np.zeros(8, dtype=np.uint64)
    v = C.c_int(0)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    assert lib.zk_diag_small_open_host(2, 0, 1, 0, 2, 0, 0, p(sh), p(out), C.byref(v)) == ZK_OK and v.value == ZK_OK
    assert lib.zk_diag_small_open_host(2, 2, 1, 0, 2, 0, 0, p(sh), p(out), C.byref(v)) == ZK_ERR_ARG       # self outside the parties
    assert lib.zk_diag_small_open_host(2, 0, 3, 0, 2, 0, 0, p(sh), p(out), C.byref(v)) == ZK_ERR_ARG       # lanes
    assert lib.zk_diag_small_open_host(2, 0, 1, 0, 0, 0, 0, p(sh), p(out), C.byref(v)) == ZK_ERR_ARG       # no items
    assert lib.zk_diag_small_open_host(2, 0, 1, 0, 2, 0, 0, None, p(out), C.byref(v)) == ZK_ERR_ARG
    assert lib.zk_diag_small_open_host(2, 0, 1, 0, 2, 0, 0, p(sh), None, C.byref(v)) == ZK_ERR_ARG
    assert lib.zk_diag_small_open_host(2, 0, 1, 0, 2, 0, 0, p(sh), p(out), None) == ZK_ERR_ARG
