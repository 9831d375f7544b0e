"""The point-bytes cases test themselves (serialize_cases.py): conditions on the case table, not measurements.  Each case's expected
class is set where the case is constructed; `classify`, the rule in Python integers, must find the same for every one, and the table
must reach every branch of the decoders that the device and host tests then run it through."""
import collections

import pytest

import zkref as O
import serialize_cases as sc

FORMS = [(g, c) for g in (1, 2) for c in (True, False)]


@pytest.mark.parametrize("group,compressed", FORMS)
def test_classify_agrees_with_every_case_as_constructed(group, compressed):
    for c in sc.cases(group, compressed):
        assert len(c.data) == sc.point_size(group, compressed)
        assert sc.classify(group, compressed, c.data) == c.expect, c.name


@pytest.mark.parametrize("group,compressed", FORMS)
def test_accepted_points_round_trip_through_the_oracles_serializers(group, compressed):
    pts, data, inside = sc.accepted(group, compressed)
    size = sc.point_size(group, compressed)
    assert len(pts) >= (512 if group == 2 else 1024) and len(data) == size * len(pts)
    assert pts[0] is None and pts[-1] is None and None in pts[1:-1]
    assert any(inside) and not all(inside)
    for i, P in enumerate(pts):
        assert sc.on_curve(group, P)
        assert sc.serialize(group, compressed, P) == data[size * i:size * i + size]
        assert sc.classify(group, compressed, sc.serialize(group, compressed, P)) == ("ok", P)
    # the same points in both forms, so that a table read in one form can be compared with the other's bytes
    assert pts == sc.accepted(group, not compressed)[0]


def test_every_exit_of_the_fq2_square_root_has_cases():
    exits = collections.Counter(sc.fq2_sqrt_exit(sc.rhs(2, sc.classify(2, False, c.data)[1][0]))
                                for c in sc.point_cases(2, False) if c.expect[0] == "ok" and c.expect[1] is not None)
    for e in ("c1zero_qr", "c1zero_nqr", "delta_qr", "delta_nqr"):
        assert exits[e] >= 8, exits
    assert exits["norm_nqr"] == 0
    off = [sc.fq2_sqrt_exit(sc.rhs(2, x)) for x in sc.non_square_abscissae(2)]
    assert off == ["norm_nqr"] * 64
    # y = (s, 0) and (0, s): the sign falls through to c0 for the first kind only
    ys = [c.expect[1][1] for c in sc.point_cases(2, True) if c.kind == "c1zero"]
    assert sum(1 for y in ys if y[1] == 0) >= 16 and sum(1 for y in ys if y[0] == 0) >= 16


def test_first_pass_of_tonelli_shanks_takes_many_lengths():
    ks = collections.Counter(sc.ts_order_log2(sc.rhs(1, c.expect[1][0])) for c in sc.point_cases(1, True) if c.expect[0] == "ok" and c.expect[1])
    assert ks.pop(None) >= 1               # rhs = 0 at (q - 1, 0): out before the exponentiation
    assert ks.pop(0) >= 2                  # rhs = 1 at x = 0: the loop is not entered
    assert len(ks) >= 6 and max(ks) <= 45, ks
    assert all(sc.ts_order_log2(sc.rhs(1, x)) == 46 for x in sc.non_square_abscissae(1))


@pytest.mark.parametrize("group,compressed", FORMS)
def test_enough_curve_cases_and_every_malformed_kind(group, compressed):
    cs = sc.cases(group, compressed)
    assert sum(1 for c in cs if c.expect == ("curve",)) >= 64
    per_kind = collections.Counter(c.kind for c in sc.malformed_cases(group, compressed))
    for kind in sc.malformed_kinds(group, compressed):
        assert per_kind[kind] >= 4, kind
    classes = {c.expect[0] for c in cs}
    assert classes == {"ok", "noncanonical", "flags", "curve"}
    assert {k for k, _, _ in sc.one_bad_per_kind(group, compressed)} == set(sc.malformed_kinds(group, compressed)) - {"0x40 over (0, 1)"} | {"curve"}


def test_the_oracles_own_g1_deserialize_reads_no_case_differently():
    reasons = {"non-canonical x": {"noncanonical"}, "x is not on the curve": {"curve"},
               "infinity with a non-zero x": {"flags", "noncanonical"}, "not in the prime-order subgroup": {"ok"}}
    seen = collections.Counter()
    for c in sc.cases(1, True):
        try:
            P = O.g1_deserialize(c.data)
        except AssertionError as e:
            assert c.expect[0] in reasons[str(e)], (c.name, str(e))
            seen[str(e)] += 1
        else:
            assert c.expect == ("ok", P), c.name
            seen["ok"] += 1
    assert seen["ok"] >= 1024 and seen["non-canonical x"] >= 24 and seen["x is not on the curve"] >= 64 and seen["infinity with a non-zero x"] >= 8


def test_altered_proofs_differ_from_the_proof_only_where_the_rule_looks():
    from pairing_cases import golden_verifier
    v = golden_verifier()
    good = O.proof_serialize(*v.proof)
    alt = sc.altered_proofs(good)
    assert sc.classify(1, True, alt["A.x + q"][:48]) == ("noncanonical",)
    assert sc.classify(2, True, alt["B.c0 + 2^377"][48:144]) == ("noncanonical",)
    assert sc.classify(1, True, alt["C flags 0xC0"][144:]) == ("flags",)
    for name, data in alt.items():
        assert len(data) == 192 and data != good
        parts = [(data[:48], good[:48]), (data[48:144], good[48:144]), (data[144:], good[144:])]
        assert sum(1 for a, b in parts if a != b) == 1, name
