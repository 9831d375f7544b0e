"""Point bytes through the HOST instantiation of csrc/serialize.hip (zk_points_deserialize_host: decompress_point and the
uncompressed decoder, the same code the kernels run) and through zk_groth16_verify_host.  The expected reading of every byte string
is `classify` of serialize_cases.py: the rule in Python integers.  No device."""
import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import api
from pairing_cases import golden_verifier
import serialize_cases as sc

FORMS = [(g, c) for g in (1, 2) for c in (True, False)]


def _points(group, arr):
    return cv.g1_array_to_affine(arr) if group == 1 else cv.g2_array_to_affine(arr)


@pytest.mark.parametrize("group,compressed", FORMS)
def test_status_and_point_of_every_case_equal_the_model(group, compressed):
    cs = sc.cases(group, compressed)
    pts, status = api.points_deserialize_host(b"".join(c.data for c in cs), len(cs), group, compressed)
    got = _points(group, pts)
    wrong = []
    for c, st, P in zip(cs, status, got):
        want = sc.classify(group, compressed, c.data)
        if int(st) != sc.STATUS[want[0]] or P != (want[1] if want[0] == "ok" else None):
            wrong.append((c.name, want[0], int(st)))
    assert not wrong, "%d of %d cases, by kind: %s; first: %s" % (len(wrong), len(cs), sorted({w[0].split(",")[0] for w in wrong}), wrong[:5])


def test_status_numbers_are_the_headers():
    assert (api.POINT_OK, api.POINT_NONCANONICAL, api.POINT_FLAGS, api.POINT_CURVE) == tuple(sc.STATUS[k] for k in ("ok", "noncanonical", "flags", "curve"))
    pts, status = api.points_deserialize_host(b"", 0, 1, True)
    assert pts.shape == (0, 12) and status.shape == (0,)
    with pytest.raises(api.ZkError):
        api.points_deserialize_host(O.g1_serialize(O.G1_GEN), 1, 3, True)


@pytest.mark.parametrize("check_subgroup", [False, True])
def test_a_proof_has_one_byte_string(check_subgroup):
    """A decoder that drops bits 377.. of an abscissa or tests the infinity bit first reads each altered proof as the golden one:
    the verifier must answer False, with no error; the untouched proof still verifies."""
    v = golden_verifier()
    inp = cv.fr_to_mont(v.inputs)
    good = O.proof_serialize(*v.proof)
    assert api.groth16_verify_host(inputs_mont=inp, proof=good, check_subgroup=check_subgroup, **v.vk) is True
    for name, data in sc.altered_proofs(good).items():
        assert api.groth16_verify_host(inputs_mont=inp, proof=data, check_subgroup=check_subgroup, **v.vk) is False, name
