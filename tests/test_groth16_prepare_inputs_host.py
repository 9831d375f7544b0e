"""prepare_inputs through the HOST form (zk_groth16_prepare_inputs_host) on keys with 0, 1, 2, 3, 8 and 33 public inputs: for every
named input vector of groth16_verify_cases.py -- inputs of 0, 1 and r - 1, a term equal or opposite to the running sum, the sum at
infinity -- the point is the generator times the prepared input's discrete log, which the key's trapdoor gives."""
import ctypes as C

import numpy as np
import pytest

import zkref as O
import zk_mpc_amd.convert as cv
from zk_mpc_amd import _lib, api
import groth16_verify_cases as G

ZK_ERR_ARG = -2


@pytest.mark.parametrize("ninp", G.NINPS)
def test_every_named_vector_gives_the_point_of_its_discrete_log(ninp):
    k = G.host_key(ninp + 1)
    rng = O.Prng(0x9E9A + ninp)
    at_infinity = 0
    for name in G.vector_names(ninp):
        x = G.vector(name, k.pks, rng)
        want = O.g1_mul(k.g1, G.prepared(k.pks, x))
        got = api.groth16_prepare_inputs_host(inputs_mont=G.inputs_mont([x])[0], **k.vk)
        assert got.tolist() == cv.g1_affine_to_array([want])[0].tolist(), name
        if G.prepared(k.pks, x) == 0:
            assert not got.any(), name
            at_infinity += 1
    assert at_infinity == (1 if ninp else 0)            # cancel@last


def test_refusals():
    k = G.host_key(4)
    lib = _lib.load()
    vk, _abc = api._vk_host(**k.vk)
    inp = G.inputs_mont([[1, 2, 3]])[0]
    out = np.zeros(12, dtype=np.uint64)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    call = lambda vk_, inp_, n, out_: lib.zk_groth16_prepare_inputs_host(C.byref(vk_) if vk_ is not None else None, p(inp_), n, p(out_))
    assert call(vk, inp, 3, out) == _lib.ZK_OK and out.any()
    assert call(None, inp, 3, out) == ZK_ERR_ARG and call(vk, None, 3, out) == ZK_ERR_ARG and call(vk, inp, 3, None) == ZK_ERR_ARG
    assert call(vk, inp, 2, out) == ZK_ERR_ARG and call(vk, inp, 4, out) == ZK_ERR_ARG
    at_r = inp.copy()
    at_r[2] = cv.fr_raw([O.R_MOD])[0]
    assert call(vk, at_r, 3, out) == ZK_ERR_ARG
    k0 = G.host_key(1)
    vk0, _abc0 = api._vk_host(**k0.vk)
    assert call(vk0, None, 0, out) == _lib.ZK_OK
    assert out.tolist() == k0.vk["gamma_abc_g1"][0].tolist()
