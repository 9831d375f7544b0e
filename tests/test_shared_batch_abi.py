"""The collaborative batch entry points (zk_groth16_prove_shared_batch, zk_groth16_prove_shared_spdz_batch) are exported, declared to
ctypes, and refuse a null context with ZK_ERR_ARG, without a GPU."""
import ctypes as C

import zk_mpc_amd
from zk_mpc_amd import _lib

ZK_ERR_ARG = -2


def test_shared_batch_entry_points_reject_a_null_context():
    lib = zk_mpc_amd.load()
    buf = C.create_string_buffer(4096)
    p = C.cast(buf, C.c_void_p)
    lanes = (C.c_void_p * 2)(p.value, p.value)
    assert lib.zk_groth16_prove_shared_batch(None, p, p, 2, p, p, p, None, None, None, None, p, None) == ZK_ERR_ARG
    assert lib.zk_groth16_prove_shared_spdz_batch(None, p, p, 2, lanes, lanes, lanes, None, None, None, None, p, None) == ZK_ERR_ARG


def test_shared_batch_prototypes_take_the_count_as_a_size():
    for name in ("zk_groth16_prove_shared_batch", "zk_groth16_prove_shared_spdz_batch"):
        restype, argtypes = _lib.PROTOTYPES[name]
        assert restype is C.c_int and len(argtypes) == 13 and argtypes[3] is C.c_size_t
